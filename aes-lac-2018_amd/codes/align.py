"""CTC forced alignment: when was each character and word of a KNOWN transcript spoken, and how well does it fit
(not in the reference).  The decoders' ``offsets`` time what the model itself would have written; this takes the
transcript as the constraint: ``ds2_ctc_align`` (``csrc/ctc_align.hip``) finds the best single alignment of every
utterance of a minibatch in one launch, and the host part below turns its frames into characters, words and seconds.
"""
import math

import numpy as np
import torch

from ds2hip import lib, ops

from .preprocessing import OrderedLabelEncoder

FRAME_SHIFT_S = 0.01                # the spectrogram's hop: 160 samples at 16 kHz (codes/transforms.py)


def group_words(chars):
    """chars: [(char, start_frame, end_frame)] -> [(word, start, end)]: the runs between spaces, each from its first
    character's start to its last character's end.  Leading, trailing and repeated spaces make no word."""
    words, run = [], []
    for c, s, e in list(chars) + [(' ', -1, -1)]:
        if c == ' ':
            if run:
                words.append((''.join(r[0] for r in run), run[0][1], run[-1][2]))
            run = []
        else:
            run.append((c, s, e))
    return words


class ForcedAligner(object):
    """``align(probs (B,T,A), sizes, targets, target_sizes)`` with the evaluator's tensors (``probs`` on the device, flat
    ``targets``) returns one dict per utterance: ``score`` (log-score of the best alignment, -inf if there is none),
    ``score_per_frame`` (score / frames; the figure to prune mis-transcribed clips by), ``chars`` [(char, start_frame,
    end_frame)] and ``words`` [(word, start_frame, end_frame)], frames inclusive; an utterance without an alignment has
    empty lists.  ``log_input=True`` if ``probs`` are log-probabilities."""

    def __init__(self, label_encoder, blank_index=0, log_input=False):
        if isinstance(label_encoder, str):
            label_encoder = list(label_encoder)
        if isinstance(label_encoder, (set, list)):
            label_encoder = OrderedLabelEncoder().fit(label_encoder)
        self.label_encoder = label_encoder
        self.blank_index, self.log_input = int(blank_index), bool(log_input)

    @staticmethod
    def frame_to_seconds(t):
        """Centre of the model's output step ``t`` in seconds: (2 t + 5) * 0.01.

        conv2 (time stride 1, 11 taps, no padding) centres step t on conv1 step t + 5; conv1 (time stride 2, padding 10,
        11 taps) centres its step u on spectrogram frame 2 u - 10 + 5 = 2 u - 5; so step t sits on frame 2 (t + 5) - 5 =
        2 t + 5.  Spectrogram frames are 10 ms apart and centred on their sample (``center=True``), so frame f is at
        f * 0.01 s and the resolution is 20 ms.  The same geometry gives ``ops.conv_out_frames``: t1 = (t_in + 20 - 11)
        // 2 + 1 conv1 steps and t1 - 10 output steps; with 2 t1 <= t_in + 11 the last step's centre 2 (t1 - 11) + 5 is at
        most frame t_in - 6, so every centre lies inside the clip."""
        return (2 * int(t) + 5) * FRAME_SHIFT_S

    def _chars(self, labels, starts, ends):
        if len(labels) == 0:
            return []
        text = self.label_encoder.inverse_transform(labels)
        return [(str(c), int(s), int(e)) for c, s, e in zip(text, starts, ends)]

    def align(self, probs, sizes, targets, target_sizes):
        if not probs.is_cuda:
            raise RuntimeError('ForcedAligner.align runs on device tensors only')
        dev = probs.device
        bsz = probs.shape[0]
        lens_h = torch.as_tensor(target_sizes).to('cpu', torch.int32).reshape(-1)
        offs_h = torch.cumsum(lens_h, 0, dtype=torch.int32) - lens_h
        lmax = int(lens_h.max()) if bsz else 0
        sizes_h = torch.as_tensor(sizes).to('cpu', torch.int32).reshape(-1)
        targets_h = torch.as_tensor(targets).to('cpu', torch.int32).reshape(-1)
        states, starts, ends, score = ops.ctc_align(
            probs.detach().contiguous().float(), sizes_h.to(dev), targets_h.to(dev), offs_h.to(dev), lens_h.to(dev), lmax,
            self.blank_index, self.log_input)
        starts, ends, score = starts.cpu().numpy(), ends.cpu().numpy(), score.cpu().numpy()
        targets_n, t_max = targets_h.numpy(), int(probs.shape[1])
        out = []
        for b in range(bsz):
            n, o = int(lens_h[b]), int(offs_h[b])
            frames = min(max(int(sizes_h[b]), 0), t_max)
            sc = float(score[b])
            chars = self._chars(targets_n[o:o + n], starts[b, :n], ends[b, :n]) if np.isfinite(sc) else []
            out.append({'score': sc, 'score_per_frame': sc / max(frames, 1), 'chars': chars, 'words': group_words(chars)})
        return out


def diagonal_band(T, S, W):
    """The band that follows the diagonal of the (T, S) lattice: int64 ``lo[t] = min(max((t (S-1)) // max(T-1, 1) - W//2, 0),
    max(S - W, 0))``.  Integers only and non-decreasing; it admits states 0 / 1 at the first frame and, from two frames on,
    S - 1 at the last."""
    T, S, W = int(T), int(S), int(W)
    t = torch.arange(T, dtype=torch.int64)
    lo = torch.div(t * (S - 1), max(T - 1, 1), rounding_mode='floor') - W // 2
    return lo.clamp_(min=0).clamp_(max=max(S - W, 0))


def band_margin(states, lo, W, S):
    """The smallest distance of a state path to a band edge that actually restricts it: ``min(states - lo)`` over the frames
    with ``lo > 0`` and ``min(lo + W - 1 - states)`` over the frames with ``lo + W < S``; None when no frame is restricted.
    An indicator, not a proof: a free optimum that lies far outside the band leaves no trace in the banded path."""
    states = torch.as_tensor(states).to(torch.int64).reshape(-1)
    lo = torch.as_tensor(lo).to(states.device, torch.int64).reshape(-1)
    below, above = states - lo, lo + int(W) - 1 - states
    lower, upper = lo > 0, lo + int(W) < int(S)
    found = []
    if bool(lower.any()):
        found.append(int(below[lower].min()))
    if bool(upper.any()):
        found.append(int(above[upper].min()))
    return min(found) if found else None


def path_band(states, W, S):
    """The band that follows a state path: int64 ``lo = cummax(clamp(states - W//2, 0, max(S - W, 0)))``, integers only.  A
    path never falls and moves at most two states per frame, so this lo is non-negative, non-decreasing, rises by at most 2
    (< W) per frame and holds the path itself: a legal band, centred on the path wherever the ends of the state row let it."""
    states = torch.as_tensor(states).to(torch.int64).reshape(-1)
    lo = (states - int(W) // 2).clamp_(min=0).clamp_(max=max(int(S) - int(W), 0))
    return torch.cummax(lo, 0)[0] if lo.numel() else lo


class LongAligner(ForcedAligner):
    """Alignment of ONE long recording's probabilities to its whole transcript with ``ds2_ctc_align_banded`` on a diagonal
    band.  ``align(probs (T,A) on the device, labels)`` starts at the smallest band the library takes that is at least
    ``min(S, band_states)`` states wide (S = 2 L + 1) and doubles it while there is no alignment inside the band or the
    path comes closer than ``band_margin`` states to a restricting edge, until the band holds all S states or is the
    library's widest; the last attempt is returned as it is: ``score``, ``score_per_frame``, ``chars``, ``words`` (as
    ``ForcedAligner``), ``states`` (int32 tensor (T,) on the device, -1 without an alignment), ``band_states`` (the width
    used) and ``band_margin`` (``band_margin()`` of the path; None without an alignment or a restricting edge).

    ``gap_penalty`` (None: everything above, nothing else) aligns with ``ds2_ctc_align_banded_gap`` instead: the blanks
    between words may absorb audio the transcript does not cover, at ``gap_penalty`` nats per frame below the frame's best
    symbol.  ``space_index`` defaults to the label encoder's ``' '``, or -1 (end blanks only) if the alphabet has none.  A long
    uncovered opening moves the true path off the diagonal by more than half a band, and a diagonal band of any legal width
    then clips it; so if the doubling ends still tight with a finite score, up to ``recentre`` further launches at the same
    width use ``path_band(previous states)``, stopping at the first that is not tight.  The result gains ``gap`` (uint8
    tensor (T,) on the device: the frames the path absorbed), ``gap_frames`` and ``band_recentred`` (the number of such
    launches)."""

    def __init__(self, label_encoder, band_states=4096, band_margin=16, blank_index=0, log_input=False, gap_penalty=None,
                 space_index=None, recentre=2):
        super().__init__(label_encoder, blank_index, log_input)
        self.band_states, self.band_margin = int(band_states), int(band_margin)
        if self.band_states < 1:
            raise ValueError('LongAligner: band_states = %r is not a positive number of states' % (band_states,))
        self.gap_penalty = None if gap_penalty is None else float(gap_penalty)
        if self.gap_penalty is not None and not self.gap_penalty >= 0:
            raise ValueError('LongAligner: gap_penalty = %r is negative or not a number' % (gap_penalty,))
        if space_index is None:
            space_index = getattr(self.label_encoder, 'map_classes_', {}).get(' ', -1)
        self.space_index, self.recentre = int(space_index), int(recentre)

    def _launch(self, p, t_n, labels_d, n, lo, width):
        """One launch on the band ``lo`` -> (states, starts, ends, gap or None, score, margin, tight)."""
        dev = p.device
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)    # noqa: E731
        args = (p, i32(t_n), labels_d, i32(0), i32(n), n, lo.to(dev, torch.int32)[None], width)
        if self.gap_penalty is None:
            states, starts, ends, score = ops.ctc_align_banded(*args, self.blank_index, self.log_input)
            gap = None
        else:
            states, starts, ends, gap, score = ops.ctc_align_banded_gap(*args, self.space_index, self.gap_penalty,
                                                                        self.blank_index, self.log_input)
        sc = float(score[0])
        margin = band_margin(states[0], lo, width, 2 * n + 1) if math.isfinite(sc) and t_n else None
        tight = not math.isfinite(sc) or (margin is not None and margin < self.band_margin)
        return states, starts, ends, gap, sc, margin, tight

    def align(self, probs, labels):
        if not probs.is_cuda:
            raise RuntimeError('LongAligner.align runs on device tensors only')
        if probs.dim() != 2:
            raise ValueError('LongAligner.align takes the (T,A) probabilities of one recording')
        dev, t_n = probs.device, int(probs.shape[0])
        labels_h = torch.as_tensor(np.asarray(labels, dtype=np.int64).reshape(-1)).to(torch.int32)
        n = int(labels_h.numel())
        s_n = 2 * n + 1
        p, labels_d = probs.detach().contiguous().float()[None], labels_h.to(dev)
        width = max(lib.ALIGN_BAND_MIN, 1 << max(min(s_n, self.band_states) - 1, 0).bit_length())
        width = min(width, lib.ALIGN_BAND_MAX)
        while True:
            states, starts, ends, gap, sc, margin, tight = self._launch(p, t_n, labels_d, n, diagonal_band(t_n, s_n, width),
                                                                        width)
            if not tight or width >= s_n or width >= lib.ALIGN_BAND_MAX:
                break
            width *= 2
        recentred = 0
        while self.gap_penalty is not None and tight and math.isfinite(sc) and recentred < self.recentre:
            states, starts, ends, gap, sc, margin, tight = self._launch(p, t_n, labels_d, n,
                                                                        path_band(states[0], width, s_n), width)
            recentred += 1
        chars = self._chars(labels_h.numpy(), starts[0].cpu().numpy(), ends[0].cpu().numpy()) if math.isfinite(sc) else []
        res = {'score': sc, 'score_per_frame': sc / max(t_n, 1), 'chars': chars, 'words': group_words(chars),
               'states': states[0], 'band_states': width, 'band_margin': margin}
        if self.gap_penalty is not None:
            res.update(gap=gap[0], gap_frames=int(gap[0].sum()), band_recentred=recentred)
        return res
