"""Host reference for CTC forced alignment (``ds2_ctc_align``): a numpy float64 Viterbi over the extended sequence
blank, l1, blank, ..., lL, blank with the library's tie rule -- at each (t, s) stay wins, then s-1, then s-2; at the end
state 2L wins over 2L-1 -- and a brute-force enumerator of all A^T frame labellings for tiny T.

The tie rule picks, among the optimal paths, the one whose state sequence read from the LAST frame backwards is
lexicographically greatest (the back-trace prefers the highest admissible predecessor at every step); that is how the
enumerator, which knows nothing of back-pointers, names the same path.
"""
import itertools

import numpy as np

NEG = -np.inf


def frame_terms(x, log_input):
    """(T,A) inputs -> float64 per-frame terms: the input itself or its log (log 0 = -inf); NaN -> -inf."""
    x = np.asarray(x, dtype=np.float64)
    if not log_input:
        with np.errstate(divide='ignore', invalid='ignore'):
            x = np.log(x)
    return np.where(np.isnan(x), NEG, x)


def viterbi(logp, labels, blank=0):
    """logp (T,A) float64 terms of the valid frames, labels a sequence of ints -> (score, states (T,) int or None).
    T = 0 aligns only the empty transcript (score 0)."""
    logp = np.asarray(logp, dtype=np.float64)
    t_n, a_n = logp.shape[0], logp.shape[1]
    labels = [int(v) for v in labels]
    n = len(labels)
    if any(v < 0 or v >= a_n or v == blank for v in labels):
        return NEG, None
    if t_n == 0:
        return (0.0, np.zeros(0, dtype=np.int64)) if n == 0 else (NEG, None)
    s_n = 2 * n + 1
    ext = np.full(s_n, blank, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(s_n, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    bp = np.zeros((t_n, s_n), dtype=np.int8)
    v = np.full(s_n, NEG)
    v[0] = logp[0, ext[0]]
    if s_n > 1:
        v[1] = logp[0, ext[1]]
    for t in range(1, t_n):
        x1, x2 = np.full(s_n, NEG), np.full(s_n, NEG)
        x1[1:] = v[:-1]
        x2[2:] = v[:-2]
        x2[~skip] = NEG
        best, code = v.copy(), np.zeros(s_n, dtype=np.int8)
        m = x1 > best
        best[m], code[m] = x1[m], 1
        m = x2 > best
        best[m], code[m] = x2[m], 2
        with np.errstate(invalid='ignore'):
            v = np.where(best == NEG, NEG, best + logp[t, ext])
        bp[t] = code
    s, score = s_n - 1, v[s_n - 1]
    if s_n > 1 and v[s_n - 2] > score:
        s, score = s_n - 2, v[s_n - 2]
    if not score > NEG:                                     # -inf (or NaN from +inf inputs): no alignment
        return NEG, None
    states = np.zeros(t_n, dtype=np.int64)
    for t in range(t_n - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return float(score), states


def spans(states, n_labels):
    """First and last frame (inclusive) spent in each label's state (state 2l+1)."""
    starts, ends = np.full(n_labels, -1, dtype=np.int64), np.full(n_labels, -1, dtype=np.int64)
    for t, s in enumerate(states):
        if s & 1:
            if starts[s >> 1] < 0:
                starts[s >> 1] = t
            ends[s >> 1] = t
    return starts, ends


def collapse(states, labels, blank=0):
    """The labelling a state path spells: the symbol of each frame, repeats merged, blanks dropped."""
    out, prev = [], None
    for s in states:
        s = int(s)
        if s & 1 and s != prev:
            out.append(int(labels[s >> 1]))
        prev = s
    return out


def path_score(logp, states, labels, blank=0):
    """Float64 score of a state path, and the sum of |terms| along it."""
    terms = np.array([logp[t, labels[int(s) >> 1] if int(s) & 1 else blank] for t, s in enumerate(states)],
                     dtype=np.float64)
    return float(terms.sum()), float(np.abs(terms).sum())


def is_valid_path(states, n_labels, labels):
    """A CTC alignment of the transcript: starts in state 0 or 1, ends in 2L or 2L-1, moves by 0, 1, or 2 onto a label
    that differs from the one two states back."""
    states = [int(s) for s in states]
    s_n = 2 * n_labels + 1
    if not states:
        return n_labels == 0                                # no frames: only the empty transcript
    if states[0] not in (0, 1) or states[-1] not in (s_n - 1, s_n - 2) or min(states) < 0:
        return False
    for p, c in zip(states, states[1:]):
        d = c - p
        if d not in (0, 1, 2):
            return False
        if d == 2 and (not c & 1 or labels[c >> 1] == labels[(c >> 1) - 1]):
            return False
    return True


def align_batch(probs, sizes, labels_list, blank=0, log_input=False, max_label_len=None):
    """The device entry point's contract on the host: probs (B,T,A), sizes (B), labels_list B sequences ->
    states (B,T) int32, starts / ends (B,Lmax) int32, score (B) float32."""
    probs = np.asarray(probs)
    bsz, t_n = probs.shape[0], probs.shape[1]
    lmax = max([len(v) for v in labels_list] + [0]) if max_label_len is None else max_label_len
    states = np.full((bsz, t_n), -1, dtype=np.int32)
    starts = np.full((bsz, lmax), -1, dtype=np.int32)
    ends = np.full((bsz, lmax), -1, dtype=np.int32)
    score = np.full(bsz, NEG, dtype=np.float32)
    for b in range(bsz):
        n = min(max(int(sizes[b]), 0), t_n)
        sc, st = viterbi(frame_terms(probs[b, :n], log_input), labels_list[b], blank)
        score[b] = sc
        if st is not None:
            states[b, :n] = st
            starts[b, :len(labels_list[b])], ends[b, :len(labels_list[b])] = spans(st, len(labels_list[b]))
    return states, starts, ends, score


def brute_force(logp, labels, blank=0):
    """Every one of the A^T frame labellings whose collapse is ``labels``: the best score and, among the labellings that
    reach it, the state path that is greatest read from the last frame backwards.  (score, states) or (-inf, None)."""
    logp = np.asarray(logp, dtype=np.float64)
    t_n, a_n = logp.shape
    labels = [int(v) for v in labels]
    best, best_key, best_states = NEG, None, None
    for pi in itertools.product(range(a_n), repeat=t_n):
        out, states, prev = [], [], None
        for c in pi:
            if c != blank and c != prev:
                out.append(c)
            states.append(2 * len(out) if c == blank else 2 * len(out) - 1)
            prev = c
        if out != labels:
            continue
        sc = float(sum(logp[t, c] for t, c in enumerate(pi)))
        if not sc > NEG:
            continue
        key = tuple(reversed(states))
        if sc > best or (sc == best and key > best_key):
            best, best_key, best_states = sc, key, states
    return best, (None if best_states is None else np.array(best_states, dtype=np.int64))
