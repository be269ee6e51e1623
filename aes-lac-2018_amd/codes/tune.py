"""Grid search over the LM fusion weights on the device (not in the reference, which has no LM).

``LMTuner`` decodes one batch of probabilities under many (alpha, beta) pairs per launch
(``ops.ctc_beam_search_rows``: one workgroup per (grid point, utterance) row) and counts every row's word and character
errors on the device (``ops.edit_stats``), summed per grid point.  Nothing crosses to the host until ``result()``.
``parse_grid`` and ``best_point`` are the CLI's (``tune_lm.py``) list syntax and ranking.
"""
import torch

from ds2hip import ops

from .decoder import DeviceBeamCTCDecoder
from .metrics import rates, target_layout

MAX_GRID_POINTS = 4096


def parse_grid(text, flag):
    """``'0,0.5,1'`` or ``'lo:hi:step'`` (inclusive of hi up to rounding) -> list of floats; ``flag`` names the option in
    the ValueError a malformed or empty list raises."""
    text = (text or '').strip()
    bad = ValueError('%s: %r is neither a comma list of numbers nor lo:hi:step' % (flag, text))
    try:
        if ':' in text:
            parts = [float(v) for v in text.split(':')]
            if len(parts) != 3:
                raise bad
            lo, hi, step = parts
            if not (step > 0 and hi >= lo) or any(v != v or v in (float('inf'), float('-inf')) for v in parts):
                raise bad
            count = int((hi - lo) / step + 1e-9) + 1
            if count > MAX_GRID_POINTS:
                raise ValueError('%s: %r makes %d values, more than %d' % (flag, text, count, MAX_GRID_POINTS))
            vals = [round(lo + k * step, 10) for k in range(count)]
        else:
            vals = [float(v) for v in text.split(',')] if text else []
    except ValueError as e:
        raise e if e is bad or str(e).startswith(flag) else bad
    if not vals:
        raise ValueError('%s: the list is empty' % flag)
    if any(v != v or v in (float('inf'), float('-inf')) for v in vals):
        raise bad
    if len(vals) > MAX_GRID_POINTS:
        raise ValueError('%s: %d values, more than %d' % (flag, len(vals), MAX_GRID_POINTS))
    return vals


def best_point(grid):
    """The entry with the fewest word edits, then the fewest char edits, then the lowest alpha, then the lowest beta."""
    return min(grid, key=lambda e: (e['word_dist'], e['char_dist'], e['alpha'], e['beta']))


class LMTuner(object):
    """Error counts of the device beam search with ``lm`` at every (alpha, beta) of a full grid.

    ``add_batch(probs (B,T,A), sizes (B,), targets (flat), target_sizes (B,))`` decodes the batch under as many grid points
    per ``ops.ctc_beam_search_rows`` launch as fit in ``rows_per_launch`` rows (at least one point) and follows each launch
    with one ``ops.edit_stats`` launch grouped by grid point; nothing waits on the stream.  ``result()`` reads the
    (points, 10) table back once.  A row's labels are bit-identical to ``DeviceBeamCTCDecoder(alpha, beta).decode``'s."""

    def __init__(self, label_encoder, lm, beam_width, alphas, betas, rows_per_launch=2048, blank_index=0, log_input=False):
        if lm is None:
            raise ValueError('LMTuner tunes the weights of a language model: lm is None')
        self._dec = DeviceBeamCTCDecoder(label_encoder, blank_index, beam_width, lm=lm, log_input=log_input)
        self.alphas, self.betas = [float(a) for a in alphas], [float(b) for b in betas]
        if not self.alphas or not self.betas:
            raise ValueError('LMTuner needs at least one alpha and one beta')
        self.points = [(a, b) for a in self.alphas for b in self.betas]          # alpha-major
        if len(self.points) > MAX_GRID_POINTS:
            raise ValueError('%d grid points, more than %d' % (len(self.points), MAX_GRID_POINTS))
        if rows_per_launch < 1:
            raise ValueError('rows_per_launch must be >= 1')
        self.rows_per_launch = int(rows_per_launch)
        self.lm, self.beam_width, self.space_id = lm, int(beam_width), self._dec.space_id
        self._totals = self._ref_len = self._alpha = self._beta = None
        self._index = {}             # (B, points per launch) -> (utt, point offset per row) on the device
        self.utterances = 0
        self.launches = 0

    def _rows(self, bsz, k, dev):
        key = (bsz, k)
        if key not in self._index:
            utt = torch.arange(bsz, dtype=torch.int32, device=dev).repeat(k).contiguous()
            point = torch.arange(k, dtype=torch.int32, device=dev).repeat_interleave(bsz).contiguous()
            self._index[key] = (utt, point)
        return self._index[key]

    def add_batch(self, probs, sizes, targets, target_sizes):
        if not probs.is_cuda:
            raise RuntimeError('LMTuner.add_batch runs on device tensors only')
        dev = probs.device
        npts = len(self.points)
        if self._totals is None:
            self._totals = torch.zeros((npts, 10), dtype=torch.int64, device=dev)
            self._ref_len = torch.zeros((), dtype=torch.int64, device=dev)
            self._alpha = torch.tensor([p[0] for p in self.points], dtype=torch.float32, device=dev)
            self._beta = torch.tensor([p[1] for p in self.points], dtype=torch.float32, device=dev)
        probs = probs.detach().contiguous().float()
        bsz = int(probs.shape[0])
        sizes_d = torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).contiguous()
        ref, offsets, lens, max_len = target_layout(targets, target_sizes, dev)
        per = max(1, self.rows_per_launch // max(bsz, 1))
        for p0 in range(0, npts, per):
            k = min(per, npts - p0)
            utt, point = self._rows(bsz, k, dev)
            group = point + p0 if p0 else point
            alpha = self._alpha[p0:p0 + k].repeat_interleave(bsz)
            beta = self._beta[p0:p0 + k].repeat_interleave(bsz)
            labels, _, hyp_len, _, _ = ops.ctc_beam_search_rows(
                probs, sizes_d, utt, alpha, beta, self.beam_width, self._dec.blank_index, self._dec.log_input, self.lm,
                self.space_id)
            ops.edit_stats(labels, hyp_len, ref, offsets, lens, max_len, self.space_id, ref_index=utt, group=group,
                           totals=self._totals)
            self.launches += 1
        self._ref_len += lens.sum()
        self.utterances += bsz

    def result(self):
        """{'utterances', 'ref_words', 'ref_chars', 'ref_len', 'grid': [...], 'best': {...}}: one entry per grid point in
        alpha-major order with alpha, beta, wer, cer and the ten counts (``metrics.rates``: ``test.py``'s definitions;
        ``ref_chars`` counts non-space labels, ``ref_len`` every reference label, the CER's denominator).  One
        device-to-host copy."""
        npts = len(self.points)
        if self._totals is None:
            table, ref_len = [[0] * 10 for _ in range(npts)], 0
        else:
            flat = torch.cat([self._totals.reshape(-1), self._ref_len.reshape(1)]).cpu().tolist()
            table, ref_len = [flat[10 * p:10 * p + 10] for p in range(npts)], flat[-1]
        grid = []
        for (a, b), row in zip(self.points, table):
            entry = {'alpha': a, 'beta': b}
            entry.update(rates(list(row) + [ref_len]))
            grid.append(entry)
        return {'utterances': self.utterances, 'ref_words': grid[0]['ref_words'], 'ref_chars': grid[0]['ref_chars'],
                'ref_len': int(ref_len), 'grid': grid, 'best': best_point(grid)}
