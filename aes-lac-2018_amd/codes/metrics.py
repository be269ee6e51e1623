"""Corpus error rates accumulated on the device (the reference's ``codes/metrics.py`` holds its ignite metrics; this
project has no ignite, and its one metric here counts on the GPU).

``DeviceErrorRate`` scores label rows as the decoders' ``decode_labels`` return them against the loader's flat targets with
``ops.edit_stats`` (``ds2_edit_stats``): no strings, no host loop, one readback in ``compute()``.  WER and CER follow
``test.py``'s definitions, so the numbers are the ones its ``Test Summary`` line prints.
"""
import torch

from ds2hip import ops


def rates(total):
    """The report of one row of ten summed ``ops.EDIT_FIELDS`` counts plus the reference length with spaces
    (``test.py:81-104``): WER = 100 * word edits / max(1, reference words); CER = 100 * char edits (spaces removed) /
    max(1, reference characters INCLUDING spaces)."""
    out = {k: int(v) for k, v in zip(ops.EDIT_FIELDS, total[:10])}
    out['ref_len'] = int(total[10])
    out['wer'] = 100.0 * out['word_dist'] / max(1, out['ref_words'])
    out['cer'] = 100.0 * out['char_dist'] / max(1, out['ref_len'])
    return out


def word_matches(hyp_words, ref_words):
    """Which hypothesis words does a minimal word alignment keep: ``[bool]`` as long as ``hyp_words``.  The Levenshtein
    table over words is back-traced from its end; at each cell the diagonal is taken if it keeps the distance, then the step
    that drops a hypothesis word, then the step that drops a reference word.  A hypothesis word is correct if and only if
    it lies on a diagonal step with equal words."""
    hyp, ref = list(hyp_words), list(ref_words)
    m, n = len(hyp), len(ref)
    d = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        d[i][0] = i
    for j in range(n + 1):
        d[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            d[i][j] = min(d[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
    correct = [False] * m
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and d[i][j] == d[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]):
            correct[i - 1] = hyp[i - 1] == ref[j - 1]
            i, j = i - 1, j - 1
        elif i > 0 and d[i][j] == d[i - 1][j] + 1:
            i -= 1
        else:
            j -= 1
    return correct


def target_layout(targets, target_sizes, device):
    """The loader's flat ``targets`` and ``target_sizes`` as the device tensors ``ops.edit_stats`` takes:
    (ref, ref_offsets, ref_lens, max_ref_len).  The one host step is the maximum over the HOST sizes."""
    sizes = torch.as_tensor(target_sizes).to(dtype=torch.int32).reshape(-1)
    max_len = int(sizes.max()) if sizes.numel() and not sizes.is_cuda else None
    lens = sizes.to(device)
    if max_len is None:
        max_len = ops.EDIT_MAX_ITEMS        # device sizes: no readback; the kernel's own limit bounds every length
    offsets = (torch.cumsum(lens, 0, dtype=torch.int32) - lens).contiguous()
    ref = torch.as_tensor(targets).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    if ref.numel() == 0:
        ref = torch.zeros((1,), dtype=torch.int32, device=device)
    return ref, offsets, lens.contiguous(), max_len


class DeviceErrorRate(object):
    """Corpus WER / CER of label rows on the device.  ``space_id``: the label of ' ' (-1: none).

    ``update(hyp (B,stride) int32, hyp_len (B,), targets (flat), target_sizes (B,))`` adds one batch without a
    synchronisation; ``compute()`` reads the sums back once."""

    def __init__(self, space_id):
        self.space_id = int(space_id)
        self.reset()

    def reset(self):
        self._totals = None          # (1, 10) int64 on the device
        self._ref_len = None         # () int64 on the device: the reference characters including spaces
        self.utterances = 0

    def update(self, hyp, hyp_len, targets, target_sizes):
        dev = hyp.device
        if self._totals is None:
            self._totals = torch.zeros((1, 10), dtype=torch.int64, device=dev)
            self._ref_len = torch.zeros((), dtype=torch.int64, device=dev)
        ref, offsets, lens, max_len = target_layout(targets, target_sizes, dev)
        rows = int(hyp.shape[0])
        group = torch.zeros((rows,), dtype=torch.int32, device=dev)
        ops.edit_stats(hyp.contiguous(), hyp_len.contiguous(), ref, offsets, lens, max_len, self.space_id, group=group,
                       totals=self._totals)
        self._ref_len += lens.sum()
        self.utterances += rows

    def compute(self):
        """{'wer', 'cer', the ten summed counts, 'ref_len', 'utterances'}; one device-to-host copy."""
        if self._totals is None:
            out = rates([0] * 11)
        else:
            out = rates(torch.cat([self._totals.reshape(-1), self._ref_len.reshape(1)]).cpu().tolist())
        out['utterances'] = self.utterances
        return out
