"""Host reference for banded CTC forced alignment (``ds2_ctc_align_banded``), numpy float64, in two forms.

``masked_full`` is the definition: ``align_ref.viterbi``'s recursion over all S = 2 L + 1 states, started from the virtual
row {state 0: 0, the rest -inf}, in which every cell outside frame t's band lo[t] <= s < lo[t] + W is set to -inf after the
frame, with the same tie rule and back-trace.  ``windowed`` computes the same thing with T x W work: it keeps only the band's
cells, indexed by s - lo[t], and reads a predecessor through the shift lo[t] - lo[t-1]; one that falls outside the previous
frame's window is -inf.  Both carry the bad-band rule (a negative or decreasing lo, or a step of W or more: no alignment; the
recursion alone would let a step of exactly W or W + 1 through, by the lowest state's s-1 and s-2) and take any W >= 1, so
that tiny bands can be checked against brute force; the library itself takes powers of two from 64 on."""
import itertools

import numpy as np

from tests import align_ref

NEG = -np.inf


def band_is_bad(lo, w):
    """Negative, decreasing, or a step of W or more (two consecutive bands that share no state)."""
    lo = np.asarray(lo, dtype=np.int64)
    return bool((lo < 0).any() or (np.diff(lo) < 0).any() or (np.diff(lo) >= w).any())


def _prepare(logp, labels, lo, w, blank):
    logp = np.asarray(logp, dtype=np.float64)
    labels = [int(v) for v in labels]
    lo = np.asarray(lo, dtype=np.int64).reshape(-1)
    assert lo.shape[0] == logp.shape[0]
    ok = not any(v < 0 or v >= logp.shape[1] or v == blank for v in labels) and not band_is_bad(lo, w)
    s_n = 2 * len(labels) + 1
    ext = np.full(s_n, blank, dtype=np.int64)
    ext[1::2] = labels if ok else blank
    skip = np.zeros(s_n, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return logp, labels, lo, ok, s_n, ext, skip


def _choose(x0, x1, x2):
    """stay, then s-1, then s-2, strict > in that order."""
    best, code = x0.copy(), np.zeros(x0.shape[0], dtype=np.int8)
    m = x1 > best
    best[m], code[m] = x1[m], 1
    m = x2 > best
    best[m], code[m] = x2[m], 2
    return best, code


def masked_full(logp, labels, lo, w, blank=0):
    """(score, states (T,) int64) or (-inf, None)."""
    logp, labels, lo, ok, s_n, ext, skip = _prepare(logp, labels, lo, w, blank)
    t_n = logp.shape[0]
    if not ok:
        return NEG, None
    if t_n == 0:
        return (0.0, np.zeros(0, dtype=np.int64)) if not labels else (NEG, None)
    idx = np.arange(s_n)
    bp = np.zeros((t_n, s_n), dtype=np.int8)
    v = np.full(s_n, NEG)
    v[0] = 0.0                                              # the virtual row: it admits states 0 and 1
    for t in range(t_n):
        x1, x2 = np.full(s_n, NEG), np.full(s_n, NEG)
        x1[1:] = v[:-1]
        x2[2:] = v[:-2]
        x2[~skip] = NEG
        best, code = _choose(v, x1, x2)
        with np.errstate(invalid='ignore'):
            v = np.where(best == NEG, NEG, best + logp[t, ext])
        v[(idx < lo[t]) | (idx >= lo[t] + w)] = NEG         # the band
        bp[t] = code
    s, score = s_n - 1, v[s_n - 1]
    if s_n > 1 and v[s_n - 2] > score:
        s, score = s_n - 2, v[s_n - 2]
    if not score > NEG:
        return NEG, None
    states = np.zeros(t_n, dtype=np.int64)
    for t in range(t_n - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return float(score), states


def windowed(logp, labels, lo, w, blank=0):
    """The same result with T x W work and memory."""
    logp, labels, lo, ok, s_n, ext, skip = _prepare(logp, labels, lo, w, blank)
    t_n = logp.shape[0]
    if not ok:
        return NEG, None
    if t_n == 0:
        return (0.0, np.zeros(0, dtype=np.int64)) if not labels else (NEG, None)
    off = np.arange(w)
    bp = np.zeros((t_n, w), dtype=np.int8)
    pad = np.full(w + 3, NEG)                               # cells 2 .. w+1 = the previous window; 0, 1 and w+2 stay -inf
    pad[2] = 0.0                                            # the virtual row, whose window starts at state 0
    lo_prev = 0
    for t in range(t_n):
        s = lo[t] + off
        live = s < s_n
        sc = np.minimum(s, s_n - 1)
        i0 = 2 + (lo[t] - lo_prev) + off                    # this state's cell in the previous window (from w+2 on: outside it)
        x0, x1 = pad[np.minimum(i0, w + 2)], pad[np.minimum(i0 - 1, w + 2)]
        x2 = np.where(skip[sc], pad[np.minimum(i0 - 2, w + 2)], NEG)
        best, code = _choose(x0, x1, x2)
        with np.errstate(invalid='ignore'):
            v = np.where((best == NEG) | ~live, NEG, best + logp[t, ext[sc]])
        bp[t] = code
        pad[2:w + 2] = v
        lo_prev = lo[t]

    def cell(state):
        return pad[2 + state - lo_prev] if 0 <= state - lo_prev < w else NEG
    s, score = s_n - 1, cell(s_n - 1)
    if s_n > 1 and cell(s_n - 2) > score:
        s, score = s_n - 2, cell(s_n - 2)
    if not score > NEG:
        return NEG, None
    states = np.zeros(t_n, dtype=np.int64)
    for t in range(t_n - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s - lo[t]])
    return float(score), states


def in_band(states, lo, w):
    states, lo = np.asarray(states, dtype=np.int64), np.asarray(lo, dtype=np.int64)
    return bool(((states >= lo) & (states < lo + w)).all())


def brute_force(logp, labels, lo, w, blank=0):
    """``align_ref.brute_force`` over the labellings whose state path stays in the band; ties as there."""
    logp = np.asarray(logp, dtype=np.float64)
    t_n, a_n = logp.shape
    labels = [int(v) for v in labels]
    if band_is_bad(lo, w):
        return NEG, None
    best, best_key, best_states = NEG, None, None
    for pi in itertools.product(range(a_n), repeat=t_n):
        out, states, prev = [], [], None
        for c in pi:
            if c != blank and c != prev:
                out.append(c)
            states.append(2 * len(out) if c == blank else 2 * len(out) - 1)
            prev = c
        if out != labels or not in_band(states, lo, w):
            continue
        sc = float(sum(logp[t, c] for t, c in enumerate(pi)))
        if not sc > NEG:
            continue
        key = tuple(reversed(states))
        if sc > best or (sc == best and key > best_key):
            best, best_key, best_states = sc, key, states
    return best, (None if best_states is None else np.array(best_states, dtype=np.int64))


def diagonal(t_n, s_n, w):
    """``codes.align.diagonal_band`` in numpy (the formula of the issue, integers only)."""
    t = np.arange(t_n, dtype=np.int64)
    return np.minimum(np.maximum((t * (s_n - 1)) // max(t_n - 1, 1) - w // 2, 0), max(s_n - w, 0))


def staircase(t_n, steps):
    """lo that rises by steps[t % len(steps)] after every frame, from 0."""
    inc = np.array([steps[t % len(steps)] for t in range(max(t_n - 1, 0))], dtype=np.int64)
    return np.concatenate([np.zeros(min(t_n, 1), dtype=np.int64), np.cumsum(inc)])[:t_n]


def align_batch_banded(probs, sizes, labels_list, lo, w, blank=0, log_input=False, max_label_len=None, impl=windowed):
    """The device entry point's contract on the host: probs (B,T,A), sizes (B), labels_list B sequences, lo (B,T) ->
    states (B,T) int32, starts / ends (B,Lmax) int32, score (B) float64.  Only an utterance's valid frames of lo count."""
    probs = np.asarray(probs)
    bsz, t_n = probs.shape[0], probs.shape[1]
    lmax = max([len(v) for v in labels_list] + [0]) if max_label_len is None else max_label_len
    states = np.full((bsz, t_n), -1, dtype=np.int32)
    starts = np.full((bsz, lmax), -1, dtype=np.int32)
    ends = np.full((bsz, lmax), -1, dtype=np.int32)
    score = np.full(bsz, NEG, dtype=np.float64)
    for b in range(bsz):
        n, k = min(max(int(sizes[b]), 0), t_n), len(labels_list[b])
        if k > lmax:                                        # a label_lens[b] outside 0..max: no alignment
            continue
        sc, st = impl(align_ref.frame_terms(probs[b, :n], log_input), labels_list[b], np.asarray(lo)[b, :n], w, blank)
        score[b] = sc
        if st is not None:
            states[b, :n] = st
            starts[b, :k], ends[b, :k] = align_ref.spans(st, k)
    return states, starts, ends, score
