"""Host reference for banded CTC alignment with gaps (``ds2_ctc_align_banded_gap``), numpy float64 over fp32 frame values.

The quantity is ``align_banded_ref``'s with another emission at the ELIGIBLE blank states (the two end blanks and the blanks
beside a ``space`` label): ``max(lp[t][blank], f[t])`` with ``f[t] = max_a lp[t][a] - g`` formed in float32, a frame where
``f[t]`` wins strictly being a gap frame.  The choice depends on (t, s) alone, so the recursion is ``align_banded_ref``'s own,
run on per-state emissions: the eligible blanks' emission is appended to the frame terms as one more column, and
``align_banded_ref._prepare`` is wrapped for the call so that the eligible states read that column.  ``masked_full`` and
``windowed`` themselves -- the band, the ties, the back-trace -- run unchanged."""
import contextlib
import itertools

import numpy as np

from tests import align_banded_ref as bref
from tests import align_ref

NEG = -np.inf


def eligible(labels, space):
    """(S,) bool: blank states (even) that are an end blank or stand beside a ``space`` label."""
    labels = [int(v) for v in labels]
    n = len(labels)
    el = np.zeros(2 * n + 1, dtype=bool)
    for s in range(0, 2 * n + 1, 2):
        el[s] = s == 0 or s == 2 * n or labels[s // 2 - 1] == space or labels[s // 2] == space
    return el


def frame_values(x, log_input, blank, g):
    """(T,A) inputs -> lp (T,A) float32 with NaN as -inf, f (T,) float32 = m - g in ONE float32 subtraction (-inf where the
    row has nothing finite), gapframe (T,) bool = f > lp[:, blank], strictly and in float32."""
    x = np.asarray(x, dtype=np.float32)
    if not log_input:
        with np.errstate(divide='ignore', invalid='ignore'):
            x = np.log(x)
    lp = np.where(np.isnan(x), np.float32(NEG), x).astype(np.float32)
    m = lp.max(axis=1) if lp.shape[0] else np.zeros(0, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        f = np.where(m == NEG, np.float32(NEG), m - np.float32(g)).astype(np.float32)
        gapframe = f > lp[:, blank]
    return lp, f, gapframe


@contextlib.contextmanager
def _per_state(el):
    """While active, ``align_banded_ref`` reads the LAST column of its frame terms at the eligible states."""
    orig = bref._prepare

    def prepare(logp, labels, lo, w, blank):
        logp = np.asarray(logp, dtype=np.float64)
        _, labels, lo, ok, s_n, ext, skip = orig(logp[:, :-1], labels, lo, w, blank)      # (label ids are judged against A)
        if ok:
            ext = ext.copy()
            ext[el] = logp.shape[1] - 1
        return logp, labels, lo, ok, s_n, ext, skip
    bref._prepare = prepare
    try:
        yield
    finally:
        bref._prepare = orig


def align_gap(x, labels, lo, w, blank, space, g, log_input=True, impl=bref.windowed):
    """(score, states (T,) int64, gap (T,) uint8) or (-inf, None, None)."""
    lp, f, gapframe = frame_values(x, log_input, blank, g)
    el = eligible(labels, space)
    eb = np.where(gapframe, f, lp[:, blank]).astype(np.float64)
    aug = np.concatenate([lp.astype(np.float64), eb[:, None]], axis=1)
    with _per_state(el):
        score, states = impl(aug, labels, lo, w, blank)
    if states is None:
        return NEG, None, None
    return score, states, (el[states] & gapframe).astype(np.uint8)


def brute_force(x, labels, lo, w, blank, space, g, log_input=True):
    """The joint maximum over every (state path, per-frame gap choice) pair: a path starts in state 0 or 1, moves by 0, 1 or
    (onto a label that differs from the one two below) 2, stays in the band and ends in S-1 or S-2; a frame spent in an
    eligible state may take f[t] instead of lp[t][blank].  Ties between paths as ``align_banded_ref.brute_force``; between
    the two choices of a frame the plain term wins.  -> (score, states, gap) or (-inf, None, None)."""
    lp, f, _ = frame_values(x, log_input, blank, g)
    lp, f = lp.astype(np.float64), f.astype(np.float64)
    labels = [int(v) for v in labels]
    t_n, s_n = lp.shape[0], 2 * len(labels) + 1
    if bref.band_is_bad(lo, w) or any(v < 0 or v >= lp.shape[1] or v == blank for v in labels):
        return NEG, None, None
    el = eligible(labels, space)
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(s_n)]
    best, best_key, best_out = NEG, None, None
    def paths(prefix):
        if len(prefix) == t_n:
            if not t_n or prefix[-1] >= s_n - 2:
                yield tuple(prefix)
            return
        nxt = (0, 1) if not prefix else (prefix[-1], prefix[-1] + 1, prefix[-1] + 2)
        for b in nxt:
            if b >= s_n or (prefix and b - prefix[-1] == 2 and not (b % 2 == 1 and ext[b] != ext[b - 2])):
                continue
            yield from paths(prefix + [b])

    for states in paths([]):
        if (t_n == 0 and s_n > 1) or not bref.in_band(states, lo, w):
            continue
        free = [t for t in range(t_n) if el[states[t]]]
        for choice in itertools.product((0, 1), repeat=len(free)):
            gap = np.zeros(t_n, dtype=np.uint8)
            gap[free] = choice
            with np.errstate(invalid='ignore'):
                sc = float(sum(f[t] if gap[t] else lp[t, ext[states[t]]] for t in range(t_n)))
            if not sc > NEG:
                continue
            key = (tuple(reversed(states)), tuple(-int(v) for v in gap))
            if sc > best or (sc == best and key > best_key):
                best, best_key, best_out = sc, key, (np.array(states, dtype=np.int64), gap)
    if best_out is None:
        return NEG, None, None
    return best, best_out[0], best_out[1]


def align_batch_banded_gap(probs, sizes, labels_list, lo, w, blank, space, g, log_input=True, max_label_len=None,
                           impl=bref.windowed):
    """The device entry point's contract on the host -> states (B,T) int32, starts / ends (B,Lmax) int32, gap (B,T) uint8,
    score (B) float64."""
    probs = np.asarray(probs)
    bsz, t_n = probs.shape[0], probs.shape[1]
    lmax = max([len(v) for v in labels_list] + [0]) if max_label_len is None else max_label_len
    states = np.full((bsz, t_n), -1, dtype=np.int32)
    starts = np.full((bsz, lmax), -1, dtype=np.int32)
    ends = np.full((bsz, lmax), -1, dtype=np.int32)
    gap = np.zeros((bsz, t_n), dtype=np.uint8)
    score = np.full(bsz, NEG, dtype=np.float64)
    for b in range(bsz):
        n, k = min(max(int(sizes[b]), 0), t_n), len(labels_list[b])
        if k > lmax:
            continue
        sc, st, gp = align_gap(probs[b, :n], labels_list[b], np.asarray(lo)[b, :n], w, blank, space, g, log_input, impl)
        score[b] = sc
        if st is not None:
            states[b, :n], gap[b, :n] = st, gp
            starts[b, :k], ends[b, :k] = align_ref.spans(st, k)
    return states, starts, ends, gap, score
