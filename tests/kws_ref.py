"""numpy reference of ds2_ctc_keyword_search (include/ds2hip.h, "keyword search"), written after the definition and not
after the kernel: the fp32 normalisation, the fp64 recursion with its tie order, the start carry and the clustering pass.
Frames are walked one by one and states are visited in plain Python loops."""
import numpy as np

MAX_LEN = 64                        # DS2_KWS_MAX_LEN
NEG = -np.inf


def emissions(logp, size):
    """(T,A) fp32 log-probabilities -> e (size,A) fp32: logp - max_a logp, one fp32 subtraction; a NaN counts as -inf in
    the maximum and gives -inf; so does every subtraction that has no value (-inf - -inf)."""
    x = np.asarray(logp, np.float32)[:size]
    x = np.where(np.isnan(x), np.float32(NEG), x).astype(np.float32)
    if x.shape[0] == 0:
        return x
    m = x.max(axis=1)
    with np.errstate(invalid='ignore'):
        e = (x - m[:, None]).astype(np.float32)
    return np.where(np.isnan(e), np.float32(NEG), e).astype(np.float32)


def keyword_ok(labels, n_classes, blank):
    labels = [int(v) for v in labels]
    return 1 <= len(labels) <= MAX_LEN and all(0 <= v < n_classes and v != blank for v in labels)


def ends(e, labels, blank):
    """D[t] and st[t][S-1] for every frame of the normalised emissions ``e``: float64 (T,), int (T,)."""
    labels = [int(v) for v in labels]
    n_states = 2 * len(labels) - 1
    ext = [labels[s // 2] if s % 2 == 0 else int(blank) for s in range(n_states)]
    v = [NEG] * n_states
    st = [-1] * n_states
    d_out, st_out = np.full(len(e), NEG, np.float64), np.full(len(e), -1, np.int64)
    for t in range(len(e)):
        nv, nst = [NEG] * n_states, [-1] * n_states
        for s in range(n_states):
            best, start = v[s], st[s]                                   # stay
            if s == 0:
                if 0.0 > best:                                          # a fresh start at t
                    best, start = 0.0, t
            else:
                if v[s - 1] > best:
                    best, start = v[s - 1], st[s - 1]
                if s >= 2 and s % 2 == 0 and ext[s] != ext[s - 2] and v[s - 2] > best:
                    best, start = v[s - 2], st[s - 2]
            nv[s] = np.float64(best) + np.float64(e[t][ext[s]])
            nst[s] = start
        v, st = nv, nst
        d_out[t], st_out[t] = v[-1], st[-1]
    return d_out, st_out


def cluster(d, st, min_score):
    """The streaming pass over the candidates (D[t], st[t], t) -> [(start, end, score)], every hit."""
    out, cur = [], None
    for t in range(len(d)):
        if not d[t] >= min_score:                                       # (a NaN threshold compares false)
            continue
        cand = (int(st[t]), t, float(d[t]))
        if cur is None:
            cur = cand
        elif cand[0] > cur[1]:
            out.append(cur)
            cur = cand
        elif cand[2] > cur[2] or (cand[2] == cur[2] and cand[0] == cur[0]):
            cur = cand
    if cur is not None:
        out.append(cur)
    return out


def search_pair(logp, size, labels, min_score, blank=0):
    """Every hit of one keyword in one utterance: [(start, end, score)]."""
    logp = np.asarray(logp, np.float32)
    size = min(max(int(size), 0), logp.shape[0])
    if not keyword_ok(labels, logp.shape[1], blank):
        return []
    d, st = ends(emissions(logp, size), labels, blank)
    return cluster(d, st, min_score)


def pack(found, max_hits):
    """[(start, end, score)] -> the rows the library writes: hits (max_hits,2) int32, hit_score (max_hits,) float64, count."""
    hits = np.full((max_hits, 2), -1, np.int32)
    score = np.full((max_hits,), NEG, np.float64)
    for i, (a, b, s) in enumerate(found[:max_hits]):
        hits[i] = (a, b)
        score[i] = s
    return hits, score, len(found)


def search_batch(logp, sizes, keywords, min_score, blank=0, max_hits=4, pairs=None):
    """The library's three outputs for logp (B,T,A), sizes (B,), ``keywords`` a list of label lists and min_score (K,).
    ``pairs``: compute only these (b, k); the others are left at -2 / NaN / -2 (for spot checks of a large batch)."""
    logp = np.asarray(logp, np.float32)
    n_b, n_k = logp.shape[0], len(keywords)
    hits = np.full((n_b, n_k, max_hits, 2), -2, np.int32)
    score = np.full((n_b, n_k, max_hits), np.nan, np.float64)
    count = np.full((n_b, n_k), -2, np.int32)
    todo = pairs if pairs is not None else [(b, k) for b in range(n_b) for k in range(n_k)]
    for b, k in todo:
        hits[b, k], score[b, k], count[b, k] = pack(
            search_pair(logp[b], sizes[b], keywords[k], min_score[k], blank), max_hits)
    return hits, score, count
