"""N-best lists without a GPU: tests/nbest_ref.py against beam_ref and bias_ref (row 0), its ordering and distinctness,
the N best of ALL labellings by brute force (no LM, char LM, word LM), the decoder's posterior formula, the argument
refusals of ds2_ctc_beam_search_nbest, and the binding table / ABI revision."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import beam_ref, bias_ref, nbest_ref
from tests.test_beam_ref_cpu import _tiny_lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _check_order(rows, count, nbest):
    assert count == len(rows) <= nbest
    scores = [r[2] for r in rows]
    assert all(x >= y for x, y in zip(scores, scores[1:])), scores
    assert len({tuple(r[0]) for r in rows}) == len(rows)                        # the final beam holds each prefix once
    for lab, off, _, _, _ in rows:
        assert len(lab) == len(off) and all(x < y for x, y in zip(off, off[1:]))


@pytest.mark.parametrize('a, w', [(5, 1), (5, 4), (8, 16), (29, 8)])
def test_row_0_is_beam_ref(a, w):
    rng = np.random.default_rng(a * 100 + w)                                   # the cases of test_beam_ref_cpu
    for t in (0, 1, 7, 25):
        probs = _softmax(rng.standard_normal((t, a)) * 2.0) if t else np.zeros((0, a), np.float32)
        lp = beam_ref.frame_log_probs(probs, False)
        s0, s1 = {}, {}
        want = beam_ref.beam_search(lp, 0, w, stats=s0)
        for nbest in sorted({1, w}):
            rows, count = nbest_ref.beam_search_nbest(lp, 0, w, nbest, stats=s1)
            _check_order(rows, count, nbest)
            assert count >= 1 and rows[0][:4] == want and rows[0][4] == 0
            assert s1['cut'] == s0['cut'] and s1['rank'][0] == s0['pick'] and len(s1['rank']) == count


@pytest.mark.parametrize('w', [1, 3, 16])
def test_row_0_is_bias_ref(w):
    rng = np.random.RandomState(w)                                             # the case of test_bias_cpu
    lp = beam_ref.frame_log_probs(_softmax(rng.standard_normal((12, 6)) * 2.0), False)
    phrases = [[1, 2], [3]]
    _, nxt, gain, final = bias_ref.tables(phrases, 6, 0)
    trans = bias_ref.pack(nxt, gain)
    for weight in (0.0, 1.5):
        s0, s1 = {}, {}
        want = bias_ref.beam_search_bias(lp, 0, w, trans, final, weight, stats=s0)
        rows, count = nbest_ref.beam_search_nbest(lp, 0, w, w, trans, final, weight, stats=s1)
        _check_order(rows, count, w)
        assert rows[0] == want and s1['cut'] == s0['cut'] and s1['rank'][0] == s0['pick']
        assert all(r[4] == bias_ref.F(r[0], phrases) for r in rows)
        assert all(r[2] == r[3] + float(np.float32(weight)) * r[4] for r in rows)
    # no graph is the root-only graph
    root = np.zeros((1, 6), np.int32), np.zeros(1, np.int32)
    assert nbest_ref.beam_search_nbest(lp, 0, w, w) == nbest_ref.beam_search_nbest(lp, 0, w, w, root[0], root[1], 3.0)


def test_fewer_valid_entries_than_n():
    lp = beam_ref.frame_log_probs(_softmax(np.random.default_rng(1).standard_normal((1, 3))), False)
    rows, count = nbest_ref.beam_search_nbest(lp, 0, 16, 16)
    assert count == 3 and sorted(r[0] for r in rows) == [[], [1], [2]]
    assert nbest_ref.beam_search_nbest([], 0, 16, 16) == ([([], [], 0.0, 0.0, 0)], 1)       # no frames: nothing said
    stats = {}
    zero = beam_ref.frame_log_probs(np.zeros((1, 3), np.float32), False)
    assert nbest_ref.beam_search_nbest(lp + zero, 0, 16, 16, stats=stats) == ([], 0) and stats['rank'] == []


def _ctc_of_every_labelling(lp, blank):
    """{labelling: log p} over every path, fp64 (the pattern of tests/test_bias_gpu.py)."""
    import itertools
    t, a = len(lp), len(lp[0])
    tot = {}
    for path in itertools.product(range(a), repeat=t):
        y = tuple(c for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1]))
        tot[y] = beam_ref.log_add(tot.get(y, beam_ref.NEG_INF), sum(lp[k][c] for k, c in enumerate(path)))
    return tot


@pytest.mark.parametrize('unit', [None, 'char', 'word'])
@pytest.mark.parametrize('t, a', [(4, 3), (4, 4), (5, 3)])
def test_the_n_best_of_all_labellings(tmp_path, unit, t, a):
    labels = ['_', ' ', 'A', 'B'][:a]                                           # a = 3: no B; the LMs score it as they find it
    lm = _tiny_lm(tmp_path, labels, unit, 0) if unit else None
    alpha, beta = (0.9, 0.4) if unit else (0.0, 0.0)
    rng = np.random.default_rng(50 * t + a + len(unit or ''))
    compared = 0
    for _ in range(4):
        lp = beam_ref.frame_log_probs(_softmax(rng.standard_normal((t, a)) * 1.5), False)
        stats = {}
        rows, count = nbest_ref.beam_search_nbest(lp, 0, 128, 128, lm=lm, alpha=alpha, beta=beta, space_id=1, stats=stats)
        assert stats['cut'] == []                                               # nothing was pruned: the beam holds them all
        every = _ctc_of_every_labelling(lp, 0)
        fused = sorted(((v + (beam_ref.lm_score(lm, list(y), alpha, beta, 1) if lm else 0.0), y) for y, v in every.items()),
                       key=lambda x: -x[0])
        assert count == len(fused) == len(rows)
        _check_order(rows, count, 128)
        for n, (row, (v, y)) in enumerate(zip(rows, fused)):
            near = [abs(v - fused[m][0]) for m in (n - 1, n + 1) if 0 <= m < len(fused)]
            assert abs(row[2] - v) <= 1e-9 * max(1.0, abs(v)), (n, row, v)
            if min(near) > 1e-7 * max(1.0, abs(v)):                             # its place is decided beyond rounding
                assert tuple(row[0]) == y and abs(row[3] - every[y]) <= 1e-9 * max(1.0, abs(every[y])), (n, row, y)
                compared += 1
    assert compared >= 40


def test_posterior_formula():
    from codes.decoder import DeviceBeamCTCDecoder
    post = DeviceBeamCTCDecoder.nbest_posteriors
    scores = np.float32([-3.25, -4.5, -4.5, -90.0])
    got = post(scores)
    s = [float(x) for x in scores]
    lse = math.log(sum(math.exp(x) for x in s))
    assert len(got) == 4 and all(abs(g - math.exp(x - lse)) <= 1e-15 for g, x in zip(got, s))
    assert abs(sum(got) - 1.0) <= 1e-12 and got[1] == got[2] and got[0] > got[1] > got[3] > 0.0
    assert post(np.float32([-1234.5])) == [1.0]                                # far below exp's range: the max is taken out
    far = np.float32([-2000.0, -2001.0])                                       # float32 holds both exactly: 1 : 1/e
    big = post(far)
    assert abs(big[0] - 1.0 / (1.0 + math.exp(-1.0))) <= 1e-15 and abs(big[0] + big[1] - 1.0) <= 1e-15
    assert post([]) == [0.0] and post(np.zeros(0, np.float32)) == [0.0]         # count 0: nothing to weigh
    with pytest.raises(ValueError, match='nbest'):
        DeviceBeamCTCDecoder(['_', 'A', 'B'], beam_width=4, nbest=5)
    with pytest.raises(ValueError, match='nbest'):
        DeviceBeamCTCDecoder(['_', 'A', 'B'], beam_width=4, nbest=0)
    assert DeviceBeamCTCDecoder(['_', 'A', 'B'], beam_width=4, nbest=4).nbest == 4
    assert DeviceBeamCTCDecoder(['_', 'A', 'B'], beam_width=4).nbest == 1


def test_nbest_entry_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    fn = lib.load().ds2_ctc_beam_search_nbest
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    # 0 probs sizes B T A blank W log | 8 ngram cap word cap order unit bos eos unk space alpha beta oov |
    # 21 trans final S w | 25 nbest ws ws_bytes | 28 labels offsets len score ctc bias count stream
    ok = [one, one, 1, 4, 5, 0, 4, 0, None, 0, None, 0, 1, 0, -1, -1, -1, -1, 0.0, 0.0, 0.0, one, one, 3, 2.0,
          2, one, 1 << 20, one, one, one, one, one, one, one, None]

    def refused(changes):
        args = list(ok)
        for pos, val in changes:
            args[pos] = val
        rc = fn(*args)
        return rc, lib.load().ds2_last_error().decode()
    for bad in (0, -1, 5, 129):                                         # nbest outside 1..beam_width: both numbers are named
        rc, msg = refused([(25, bad)])
        assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_nbest' in msg and 'nbest %d' % bad in msg and '= 4' in msg, msg
    for pos in (28, 29, 30, 31, 32, 34):                                # a NULL output, a NULL out_count
        rc, msg = refused([(pos, None)])
        assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_nbest' in msg, (pos, msg)
    assert 'out_count' in refused([(34, None)])[1]
    # with a graph, the _bias entry's own refusals
    for pos, bad in ((23, 0), (23, -1), (23, 32769), (22, None), (33, None), (24, float('inf')), (24, float('-inf')),
                     (24, float('nan'))):
        rc, msg = refused([(pos, bad)])
        assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_nbest' in msg, (pos, bad, msg)
    assert 'states' in refused([(23, 32769)])[1] and 'finite' in refused([(24, float('nan'))])[1]
    assert 'NULL' in refused([(22, None)])[1]
    # what the batch entry refuses, under this function's name -- with and without a graph
    for graph in ([], [(21, None)]):
        for pos, bad in ((6, 0), (6, 129), (4, 129), (5, 5), (1, None), (27, 8), (13, 3)):
            rc, msg = refused(graph + [(pos, bad)] + ([(25, 1)] if pos == 6 else []))
            assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_nbest' in msg, (pos, bad, msg)
    # B = 0 is DS2_OK, S at its limit is taken, and without a graph the bias arguments are ignored
    assert refused([(2, 0), (23, 32768)])[0] == 0
    assert refused([(2, 0), (21, None), (22, None), (23, -7), (24, float('nan')), (33, None)])[0] == 0
    assert refused([(2, 0), (25, 4)])[0] == 0                           # nbest = beam_width


def test_the_symbol_is_bound_and_the_revision_stays_404():
    from ds2hip import lib
    assert 'ds2_ctc_beam_search_nbest' in lib.SIGNATURES
    res, args = lib.SIGNATURES['ds2_ctc_beam_search_nbest']
    assert len(args) == 36 and len(lib.SIGNATURES['ds2_ctc_beam_search_bias'][1]) == 34
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404 == lib.ABI_VERSION
    assert lib.load().ds2_version() == 404
    assert re.search(r'int\s+ds2_ctc_beam_search_nbest\(', hdr)
