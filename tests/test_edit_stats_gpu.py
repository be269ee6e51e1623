"""ds2_edit_stats (csrc/edit_stats.hip) against its Python statement tests/edit_ref.py: ``==`` throughout, the counts are
integers.  Sequences of more than a few thousand cells use the reference's anti-diagonal form, which
tests/test_edit_stats_cpu.py holds to the cell-by-cell one."""
import numpy as np
import pytest
import torch

from tests import edit_ref

pytestmark = pytest.mark.gpu
SPACE = 0
SENTINEL = 3            # a label of the alphabet, written past hyp_len: reading it would change the counts
GUARD = 0x5A5A5A5A


def _align(h, r):
    return edit_ref.align_counts(h, r) if len(h) * len(r) <= 4000 else edit_ref.align_counts_diag(h, r)


def _seq(rng, n, alphabet=4):
    return rng.integers(0, alphabet, size=n).tolist()


def _run(hyps, refs, space=SPACE, ref_index=None, group=None, n_groups=0, totals_start=None, stride=None, max_ref_len=None,
         hyp_len=None, ref_lens=None):
    """One launch through the C ABI with guarded buffers; returns (stats list, totals list or None) after checking the
    guards and that the caller's totals start was added to."""
    from ds2hip import lib
    rows = len(hyps)
    stride = max([len(h) for h in hyps] + [1]) + 3 if stride is None else stride
    hyp = np.full((rows, stride), SENTINEL, dtype=np.int32)
    for r, h in enumerate(hyps):
        hyp[r, :len(h)] = h
    hl = [len(h) for h in hyps] if hyp_len is None else hyp_len
    rl = [len(r) for r in refs] if ref_lens is None else ref_lens
    flat, offs = [], []
    for r in refs:
        offs.append(len(flat))
        flat.extend(r)
    flat = flat + [SENTINEL] * 4
    max_ref_len = max([len(r) for r in refs] + [0]) if max_ref_len is None else max_ref_len
    dev = lambda x, dt=torch.int32: torch.tensor(np.asarray(x), dtype=dt, device='cuda')      # noqa: E731
    guarded = torch.full((rows * 10 + 20,), GUARD, dtype=torch.int32, device='cuda')
    stats = guarded[10:10 + rows * 10]
    ws = torch.full((4096,), 0xA7, dtype=torch.uint8, device='cuda')                        # garbage, must not matter
    totals = None
    if group is not None:
        start = np.zeros((n_groups, 10), dtype=np.int64) if totals_start is None else np.asarray(totals_start)
        totals = dev(start, torch.int64)
    lib.call('ds2_edit_stats', dev(hyp), dev(hl), rows, stride, dev(flat), dev(offs), dev(rl), len(refs), max_ref_len,
             None if ref_index is None else dev(ref_index), None if group is None else dev(group), n_groups, space, ws,
             ws.numel(), stats, totals)
    host = guarded.cpu().numpy()
    assert (host[:10] == GUARD).all() and (host[10 + rows * 10:] == GUARD).all()
    got = host[10:10 + rows * 10].reshape(rows, 10).tolist()
    want, want_tot = edit_ref.edit_stats(hyp, hl, flat, offs, rl, max_ref_len, space, ref_index, group, n_groups, align=_align)
    assert got == want
    if group is not None:
        got_tot = totals.cpu().numpy()
        assert (got_tot == np.asarray(want_tot, dtype=np.int64).reshape(n_groups, 10) + start).all()
        return got, got_tot.tolist()
    return got, None


def test_constants_are_the_headers():
    import os
    import re
    from ds2hip import lib, ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ds2hip.h')).read()
    val = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, hdr).group(1))      # noqa: E731
    assert ops.EDIT_MAX_ITEMS == lib.EDIT_MAX_ITEMS == val('DS2_EDIT_MAX_ITEMS') >= 2048
    assert ops.EDIT_THREADS == val('DS2_EDIT_THREADS') and ops.EDIT_CHUNK * ops.EDIT_THREADS == ops.EDIT_MAX_ITEMS
    assert ops.EDIT_FIELDS == edit_ref.FIELDS


def test_lengths_around_every_width():
    from ds2hip import ops
    rng = np.random.default_rng(1)
    edges = sorted({0, 1, 63, 64, 65, ops.EDIT_CHUNK - 1, ops.EDIT_CHUNK, ops.EDIT_CHUNK + 1, ops.EDIT_THREADS - 1,
                    ops.EDIT_THREADS, ops.EDIT_THREADS + 1})
    pairs = [(n, n) for n in edges] + [(0, n) for n in edges[1:]] + [(n, 0) for n in edges[1:]]
    pairs += [(257, 63), (8, 256), (65, 255), (1, 257), (256, 1)]
    hyps, refs = [_seq(rng, m) for m, _ in pairs], [_seq(rng, n) for _, n in pairs]
    stats, _ = _run(hyps, refs)
    assert stats[0] == [0] * 10                                         # both sides empty
    # the same lengths without spaces: every label an item, so the ITEM counts sit on the edges too
    hyps, refs = [[c + 1 for c in h] for h in hyps], [[c + 1 for c in r] for r in refs]
    stats, _ = _run(hyps, refs)
    assert [s[4] for s in stats] == [n for _, n in pairs]


def test_the_limit_itself_and_one_past_it():
    from ds2hip import lib, ops
    lim = ops.EDIT_MAX_ITEMS
    rng = np.random.default_rng(2)
    # no space label: 2048 character items a side, and ONE word of 2048 labels a side that differs in its last label
    ref = (rng.integers(0, 3, size=lim) + 1).tolist()
    hyp = list(ref)
    for k in rng.integers(0, lim - 1, size=300):
        hyp[k] = 1 + (hyp[k] % 3)
    hyp = hyp[40:] + hyp[:40]
    stats, _ = _run([hyp], [ref], space=-1, stride=lim)
    assert stats[0][4] == lim and stats[0][5:] == [1, 1, 0, 0, 1]
    same = list(ref)
    same[-1] = 1 + (same[-1] % 3)
    stats, _ = _run([same], [ref], space=-1, stride=lim)
    assert stats[0] == [1, 1, 0, 0, lim, 1, 1, 0, 0, 1]
    # with spaces: 1024 one-label words a side, the most a side can hold
    alt = lambda seq: [c for pair in zip(seq, [SPACE] * len(seq)) for c in pair]         # noqa: E731
    stats, _ = _run([alt(_seq(rng, lim // 2, 3))], [alt([c + 1 for c in _seq(rng, lim // 2, 3)])], stride=lim)
    assert stats[0][9] == lim // 2
    one = torch.zeros((1,), dtype=torch.int32, device='cuda')
    out = torch.zeros((10,), dtype=torch.int32, device='cuda')
    for stride, max_ref in ((lim + 1, 4), (4, lim + 1)):
        with pytest.raises(lib.Ds2Error, match='DS2_EDIT_MAX_ITEMS') as err:
            lib.call('ds2_edit_stats', torch.zeros((stride,), dtype=torch.int32, device='cuda'), one, 1, stride, one, one, one, 1,
                     max_ref, None, None, 0, SPACE, None, 0, out, None)
        assert err.value.code == lib.ERR_ARG


def test_words():
    rng = np.random.default_rng(3)
    long_a = (rng.integers(0, 3, size=90) + 1).tolist()                  # a word longer than 64 labels
    long_b = long_a[:-1] + [1 + (long_a[-1] % 3)]                        # equal except in the last label
    short = [1, 2, 3, 1]
    hyps = [long_a + [SPACE] + short, long_a + [SPACE] + short, [SPACE, SPACE] + short + [SPACE] + long_b + [SPACE],
            short[:-1] + [2], long_a + long_a]
    refs = [long_a + [SPACE] + short, long_b + [SPACE, SPACE] + short, long_b + [SPACE] + short,
            short, long_a + [SPACE] + long_a]
    stats, _ = _run(hyps, refs)
    assert stats[0][5:] == [0, 0, 0, 0, 2] and stats[1][5:] == [1, 1, 0, 0, 2] and stats[3][5:] == [1, 1, 0, 0, 1]
    # no space in the alphabet: label 0 is an ordinary label and the reference is one word
    stats, _ = _run([[1, 0, 2, 2], [1, 0, 2]], [[1, 0, 2], [1, 0, 2]], space=-1)
    assert stats == [[1, 0, 0, 1, 3, 1, 1, 0, 0, 1], [0, 0, 0, 0, 3, 0, 0, 0, 0, 1]]


def _mixed(rng, rows, lo=0, hi=30):
    return [_seq(rng, rng.integers(lo, hi)) for _ in range(rows)]


def test_invalid_rows_totals_and_reference_index():
    rng = np.random.default_rng(4)
    rows = 12
    hyps, refs = _mixed(rng, rows), _mixed(rng, 5, 1)
    ref_index = [int(v) for v in rng.integers(0, 5, size=rows)]
    group = [int(v) for v in rng.integers(0, 3, size=rows)]
    stride = 33
    hyp_len = [len(h) for h in hyps]
    ref_lens = [len(r) for r in refs]
    hyp_len[2] = stride + 1                     # one bad hyp_len ...
    hyp_len[9] = -1
    ref_index[4] = 5                            # ... one bad ref_index (N = 5) ...
    ref_index[10] = -1
    group[6] = 3                                # ... one bad group (G = 3) ...
    group[11] = -2
    ref_lens[3] = 31                            # ... and one bad ref_lens (max_ref_len = 30): every row that uses it
    for r in (0, 1, 5):
        ref_index[r] = 0 if r else 3
    start = rng.integers(-5, 1000, size=(3, 10))
    stats, totals = _run(hyps, refs, ref_index=ref_index, group=group, n_groups=3, totals_start=start, stride=stride,
                         max_ref_len=30, hyp_len=hyp_len, ref_lens=ref_lens)
    bad = {2, 9, 4, 10, 6, 11} | {r for r in range(rows) if 0 <= ref_index[r] < 5 and ref_index[r] == 3}
    assert 0 in bad and 1 not in bad
    for r in range(rows):
        assert (stats[r] == [-1] * 10) == (r in bad), r
    want = np.asarray(start, dtype=np.int64).copy()
    for r in range(rows):
        if r not in bad:
            want[group[r]] += np.asarray(stats[r], dtype=np.int64)
    assert (np.asarray(totals) == want).all()
    # without a group nothing is totalled and a NULL ref_index pairs row r with reference r
    stats, _ = _run(hyps[:5], refs)
    assert all(s[0] >= 0 for s in stats)
    stats, _ = _run(hyps[:7], refs)             # rows 5 and 6 have no reference
    assert stats[5] == [-1] * 10 and stats[6] == [-1] * 10 and stats[4][0] >= 0


def test_position_independence():
    rng = np.random.default_rng(6)
    row_h, row_r = _seq(rng, 70), _seq(rng, 64)
    others_h, others_r = _mixed(rng, 299, 0, 40), _mixed(rng, 299, 0, 40)
    alone, _ = _run([row_h], [row_r])
    first, _ = _run([row_h] + others_h, [row_r] + others_r)
    last, _ = _run(others_h + [row_h], others_r + [row_r])
    assert alone[0] == first[0] == last[-1]
    assert first[1:] == last[:-1]


def test_ops_layer():
    from ds2hip import ops
    rng = np.random.default_rng(8)
    hyps, refs = _mixed(rng, 6), _mixed(rng, 6)
    hyp = np.full((6, 32), SENTINEL, dtype=np.int32)
    for r, h in enumerate(hyps):
        hyp[r, :len(h)] = h
    dev = lambda x, dt=torch.int32: torch.tensor(np.asarray(x), dtype=dt, device='cuda')      # noqa: E731
    offs = np.cumsum([0] + [len(r) for r in refs])[:-1]
    flat = [c for r in refs for c in r] or [0]
    group = [0, 1, 0, 1, 0, 1]
    totals = torch.zeros((2, 10), dtype=torch.int64, device='cuda')
    args = (dev(hyp), dev([len(h) for h in hyps]), dev(flat), dev(offs), dev([len(r) for r in refs]), 30, SPACE)
    stats = ops.edit_stats(*args, group=dev(group), totals=totals)
    want = [edit_ref.edit_stats_row(h, r, SPACE) for h, r in zip(hyps, refs)]
    assert stats.dtype == torch.int32 and stats.cpu().tolist() == want
    assert totals.cpu().tolist() == [[sum(w[k] for w in want[g::2]) for k in range(10)] for g in (0, 1)]
    assert ops.edit_stats(*args).cpu().tolist() == want                  # no group: no totals needed
    with pytest.raises(RuntimeError, match='group needs totals'):
        ops.edit_stats(*args, group=dev(group))
    with pytest.raises(RuntimeError, match='hyp must be torch.int32'):
        ops.edit_stats(args[0].long(), *args[1:])
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.edit_stats(args[0].cpu(), *args[1:])
    empty = ops.edit_stats(dev(np.zeros((0, 4))), dev([]), dev([0]), dev([]), dev([]), 0, SPACE)
    assert tuple(empty.shape) == (0, 10)
