"""Pure-Python statement of ``ds2_edit_stats`` (include/ds2hip.h): TEST INFRASTRUCTURE ONLY.

Items, distance, the per-cell tie rule and the ten output values are implemented literally, one cell at a time;
``backtrace_counts`` walks the same table backwards under the same rule, which is what the forward-carried counts must equal.
"""

FIELDS = ('char_dist', 'char_sub', 'char_del', 'char_ins', 'ref_chars',
          'word_dist', 'word_sub', 'word_del', 'word_ins', 'ref_words')


def char_items(labels, space_id):
    """The sequence with every space label removed (Decoder.cer)."""
    return [int(c) for c in labels if int(c) != space_id]


def word_items(labels, space_id):
    """The maximal runs of non-space labels, as tuples (str.split(): leading, trailing, repeated spaces make no word)."""
    words, cur = [], []
    for c in labels:
        c = int(c)
        if c == space_id:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        words.append(tuple(cur))
    return words


def _move(hyp, ref, dist, i, j):
    """The one predecessor cell (i, j) takes, as (pi, pj, op), op in 'M', 'S', 'D', 'I'."""
    if i == 0:
        return 0, j - 1, 'D'
    if j == 0:
        return i - 1, 0, 'I'
    if hyp[i - 1] == ref[j - 1]:
        return i - 1, j - 1, 'M'
    best = None
    for pi, pj, op in ((i - 1, j - 1, 'S'), (i, j - 1, 'D'), (i - 1, j, 'I')):       # the tie order
        if best is None or dist[pi][pj] + 1 < dist[best[0]][best[1]] + 1:
            best = (pi, pj, op)
    return best


def table(hyp, ref):
    """dist[i][j] and counts[i][j] = (S, D, I, matches) of hypothesis prefix i against reference prefix j."""
    m, n = len(hyp), len(ref)
    dist = [[0] * (n + 1) for _ in range(m + 1)]
    counts = [[None] * (n + 1) for _ in range(m + 1)]
    counts[0][0] = (0, 0, 0, 0)
    for i in range(m + 1):
        for j in range(n + 1):
            if i == 0 and j == 0:
                continue
            pi, pj, op = _move(hyp, ref, dist, i, j)
            s, d, ins, mt = counts[pi][pj]
            dist[i][j] = dist[pi][pj] + (op != 'M')
            counts[i][j] = (s + (op == 'S'), d + (op == 'D'), ins + (op == 'I'), mt + (op == 'M'))
    return dist, counts


def align_counts(hyp, ref):
    """(dist, S, D, I, matches) of two item sequences, counts carried forward."""
    dist, counts = table(hyp, ref)
    return (dist[len(hyp)][len(ref)],) + counts[len(hyp)][len(ref)]


def backtrace_counts(hyp, ref):
    """The same five values from a back-trace of the distance table under the stated tie rule."""
    dist, _ = table(hyp, ref)
    i, j = len(hyp), len(ref)
    tally = {'S': 0, 'D': 0, 'I': 0, 'M': 0}
    while i or j:
        i, j, op = _move(hyp, ref, dist, i, j)
        tally[op] += 1
    return dist[len(hyp)][len(ref)], tally['S'], tally['D'], tally['I'], tally['M']


def align_counts_diag(hyp, ref):
    """``align_counts`` without the matches, swept by anti-diagonals in numpy: for the sequences of thousands of items
    the cell-by-cell table is too slow for.  tests/test_edit_stats_cpu.py holds it to ``align_counts``."""
    import numpy as np
    ids = {}
    h = np.asarray([ids.setdefault(x, len(ids)) for x in hyp], dtype=np.int64)
    r = np.asarray([ids.setdefault(x, len(ids)) for x in ref], dtype=np.int64)
    m, n = len(h), len(r)
    one = {'S': np.array([1, 1, 0, 0]), 'D': np.array([1, 0, 1, 0]), 'I': np.array([1, 0, 0, 1])}
    prev2 = np.zeros((m + 1, 4), dtype=np.int64)      # diagonal d - 2, row i = cell (i, d - 2 - i): dist, S, D, I
    prev1 = np.zeros((m + 1, 4), dtype=np.int64)
    cur = np.zeros((m + 1, 4), dtype=np.int64)        # d = 0: cell (0, 0)
    for d in range(1, m + n + 1):
        prev2, prev1, cur = prev1, cur, prev2
        lo, hi = max(0, d - n), min(d, m)
        if lo == 0:
            cur[0] = d * one['D']
        if hi == d:
            cur[d] = d * one['I']
        a, b = max(lo, 1), min(hi, d - 1)             # the inner cells i = a .. b, j = d - i >= 1
        if a > b:
            continue
        i = np.arange(a, b + 1)
        eq = (h[i - 1] == r[d - i - 1])[:, None]
        sub, dele, ins = prev2[i - 1] + one['S'], prev1[i] + one['D'], prev1[i - 1] + one['I']
        best = sub
        best = np.where((dele[:, :1] < best[:, :1]), dele, best)
        best = np.where((ins[:, :1] < best[:, :1]), ins, best)
        cur[i] = np.where(eq, prev2[i - 1], best)
    return tuple(int(v) for v in cur[m])


def edit_stats_row(hyp, ref, space_id, align=align_counts):
    """The ten stats of one hypothesis / reference pair of label sequences."""
    hc, rc = char_items(hyp, space_id), char_items(ref, space_id)
    hw, rw = word_items(hyp, space_id), word_items(ref, space_id)
    cd = align(hc, rc)
    wd = align(hw, rw)
    return [cd[0], cd[1], cd[2], cd[3], len(rc), wd[0], wd[1], wd[2], wd[3], len(rw)]


def edit_stats(hyp, hyp_len, ref, ref_offsets, ref_lens, max_ref_len, space_id=-1, ref_index=None, group=None,
               n_groups=0, align=align_counts):
    """``ds2_edit_stats`` on host sequences: returns (stats (R x 10 lists), totals (G x 10 lists of the ADDED sums))."""
    rows = len(hyp_len)
    stride = len(hyp[0]) if rows else 0
    stats, totals = [], [[0] * 10 for _ in range(n_groups)]
    for r in range(rows):
        ri = int(ref_index[r]) if ref_index is not None else r
        g = int(group[r]) if group is not None else 0
        ok = 0 <= int(hyp_len[r]) <= stride and 0 <= ri < len(ref_lens) and (group is None or 0 <= g < n_groups)
        ok = ok and 0 <= int(ref_lens[ri]) <= max_ref_len
        if not ok:
            stats.append([-1] * 10)
            continue
        off = int(ref_offsets[ri])
        row = edit_stats_row(list(hyp[r][:int(hyp_len[r])]), list(ref[off:off + int(ref_lens[ri])]), space_id, align)
        stats.append(row)
        if group is not None:
            totals[g] = [a + b for a, b in zip(totals[g], row)]
    return stats, totals
