"""Banded CTC alignment without a GPU: the two forms of the host reference (tests/align_banded_ref.py) against each other,
against the unbanded reference and against brute force; the band helpers of ``codes.align``; the C ABI's new entry points and
their host-side refusals."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import align_banded_ref as bref
from tests import align_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dyadic(rng, shape, holes=0.0):
    x = rng.integers(-2048, 2049, size=shape) / 64.0
    if holes:
        x[rng.random(shape) < holes] = -np.inf
    return x


def _labels(rng, n, a):
    return [int(v) for v in rng.integers(1, a, size=n)]


def _same(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert got[1].tolist() == want[1].tolist(), what


@pytest.mark.parametrize('t_n,n,w', [(40, 30, 8), (63, 50, 16), (100, 90, 32), (129, 100, 64), (50, 10, 64), (30, 60, 16)])
def test_windowed_equals_masked_full_on_diagonal_bands(t_n, n, w):
    rng = np.random.default_rng(t_n + n)
    feasible = 0
    for a, holes in ((3, 0.0), (29, 0.05), (5, 0.0)):
        labels = _labels(rng, n, a)
        x = _dyadic(rng, (t_n, a), holes)
        lo = bref.diagonal(t_n, 2 * n + 1, w)
        want = bref.masked_full(x, labels, lo, w)
        _same(bref.windowed(x, labels, lo, w), want, (t_n, n, w, a))
        if want[1] is not None:
            feasible += 1
            assert bref.in_band(want[1], lo, w) and align_ref.is_valid_path(want[1], n, labels)
            assert align_ref.path_score(x, want[1], labels)[0] == want[0]
    assert feasible or n > t_n


@pytest.mark.parametrize('steps', [(0,), (1,), (2,), (3,), (0, 1, 2, 3), (0, 0, 0, 0, 0, 0, 0, 40), (1, 2, 0, 40, 0, 0)])
def test_windowed_equals_masked_full_on_staircase_bands(steps):
    rng = np.random.default_rng(len(steps) + sum(steps))
    for t_n, n, w, a in ((60, 80, 16, 29), (33, 40, 64, 3), (90, 150, 41, 29)):
        labels = _labels(rng, n, a)
        x = _dyadic(rng, (t_n, a))
        x[:, 0][rng.random(t_n) < 0.5] = 0.0
        lo = bref.staircase(t_n, steps)
        _same(bref.windowed(x, labels, lo, w), bref.masked_full(x, labels, lo, w), (steps, t_n, n, w))


def test_a_band_that_jumps_by_its_width_and_a_bad_band_give_no_alignment():
    rng = np.random.default_rng(2)
    t_n, n, a, w = 100, 60, 29, 16
    labels, x = _labels(rng, n, a), _dyadic(rng, (t_n, a))
    good = bref.diagonal(t_n, 2 * n + 1, w)
    assert np.isfinite(bref.masked_full(x, labels, good, w)[0])
    for name, delta in (('jump of W', w), ('jump of W + 5', w + 5)):
        lo = good.copy()
        lo[50:] += delta - (lo[50] - lo[49])
        for f in (bref.masked_full, bref.windowed):
            assert f(x, labels, lo, w) == (-np.inf, None), name
    lo = good.copy()
    lo[50:] += w - 1 - (lo[50] - lo[49])                            # one state short of the width: state lo[49] + W - 1 carries on
    _same(bref.windowed(x, labels, lo, w), bref.masked_full(x, labels, lo, w), 'jump of W - 1')
    for name, lo in (('decreasing', np.r_[good[:10], good[9] - 1, good[11:]]), ('negative', np.r_[-1, good[1:]]),
                     ('decreasing at the end', np.r_[good[:-1], good[-2] - 1])):
        assert bref.band_is_bad(lo, w), name
        for f in (bref.masked_full, bref.windowed):
            assert f(x, labels, lo, w) == (-np.inf, None), name
    assert bref.brute_force(np.zeros((3, 3)), [], [2, 1, 1], 4) == (-np.inf, None)


@pytest.mark.parametrize('t_n', [0, 1, 2, 5, 33, 64])
def test_full_band_equals_the_unbanded_reference(t_n):
    rng = np.random.default_rng(t_n)
    a = 5
    for n in (0, 1, 2, t_n // 2, t_n, t_n + 1):
        labels = _labels(rng, n, a)
        x = _dyadic(rng, (t_n, a), 0.05)
        want = align_ref.viterbi(x, labels)
        for w in (2 * n + 1, 2 * n + 2, 64 + 2 * n):
            lo = np.zeros(t_n, dtype=np.int64)
            _same(bref.masked_full(x, labels, lo, w), want, ('full', t_n, n, w))
            _same(bref.windowed(x, labels, lo, w), want, ('windowed', t_n, n, w))
    for f in (bref.masked_full, bref.windowed):
        sc, st = f(np.zeros((0, a)), [], [], 64)
        assert sc == 0.0 and st.shape == (0,)
    assert bref.windowed(np.zeros((0, a)), [1], [], 64) == (-np.inf, None)


def _inputs(t_n, a_n):
    rng = np.random.default_rng(100 * t_n + a_n)
    x = rng.integers(-40, 1, size=(t_n, a_n)) / 8.0
    holes = x.copy()
    holes[rng.random((t_n, a_n)) < 0.25] = -np.inf
    levels = rng.integers(-2, 1, size=(t_n, a_n)).astype(np.float64)
    return [x, holes, levels, np.full((t_n, a_n), -1.0)]


TRANSCRIPTS = [list(p) for n in range(4) for p in itertools.product((1, 2), repeat=n)]


@pytest.mark.parametrize('t_n', range(1, 7))
def test_masked_full_equals_brute_force_inside_the_band(t_n):
    """T <= 6, A = 3, every transcript of up to 3 labels, bands of 2-4 states that stand still, climb by one or two states a
    frame, or jump: the same score and, through the tie rule, the same path as the enumeration of all labellings whose state
    path stays in the band."""
    bands = [(w, bref.staircase(t_n, steps)) for w in (2, 3, 4) for steps in ((0,), (1,), (2,), (0, 1), (1, 0, 2), (0, 3), (0, 4))]
    seen_inf = seen_path = seen_cut = 0
    for x in _inputs(t_n, 3):
        for labels in TRANSCRIPTS:
            free = align_ref.viterbi(x, labels)[0]
            for w, lo in bands:
                want = bref.brute_force(x, labels, lo, w)
                got = bref.masked_full(x, labels, lo, w)
                _same(got, want, (t_n, labels, w, lo.tolist()))
                _same(bref.windowed(x, labels, lo, w), want, ('windowed', t_n, labels, w, lo.tolist()))
                seen_inf += want[1] is None
                seen_path += want[1] is not None
                seen_cut += want[0] < free
    assert seen_inf > 0 and seen_path > 0 and (seen_cut > 0 or t_n < 3)


def test_diagonal_band():
    from codes.align import diagonal_band
    for t_n, s_n, w in itertools.product((1, 2, 3, 64, 1000), (1, 3, 63, 64, 65, 401, 100001), (64, 128, 4096)):
        lo = diagonal_band(t_n, s_n, w)
        assert lo.dtype == torch.int64 and lo.shape == (t_n,)
        assert lo.tolist() == bref.diagonal(t_n, s_n, w).tolist()
        assert int(lo[0]) == 0 and bool((lo[1:] >= lo[:-1]).all()) and int(lo.min()) >= 0
        if t_n > 1 or s_n <= w:                                     # (one frame is first and last: it starts at 0)
            assert int(lo[-1]) + w >= s_n
        assert int(lo.max()) <= max(s_n - w, 0)
    # an hour against 50 000 labels: the products pass 2^31
    lo = diagonal_band(180000, 100001, 4096)
    assert int(lo[-1]) == 100001 - 4096 and int(lo[90000]) == (90000 * 100000) // 179999 - 2048
    assert int((lo[1:] - lo[:-1]).max()) == 1
    assert diagonal_band(0, 5, 64).shape == (0,)


def test_band_margin_on_hand_made_paths():
    from codes.align import band_margin
    w, s_n = 4, 12
    lo = [0, 0, 2, 4, 8]
    # lower edge restricts frames 2-4 (lo > 0), upper edge frames 0-3 (lo + 4 < 12)
    assert band_margin([0, 1, 3, 5, 10], lo, w, s_n) == 1           # 3 - 2, 5 - 4; above: 3 - 0, 3 - 1, 5 - 3, 7 - 5
    assert band_margin([3, 3, 5, 7, 11], lo, w, s_n) == 0           # on the upper edge at frame 0
    assert band_margin([0, 1, 2, 5, 10], lo, w, s_n) == 0           # on the lower edge at frame 2
    assert band_margin([2, 2, 4, 6, 8], lo, w, s_n) == 0            # the lower edge at the last frame, where only it counts
    assert band_margin([1, 1, 4, 6, 11], lo, w, s_n) == 1
    assert band_margin([0, 1, 2], [0, 0, 0], 64, 12) is None        # the band holds every state: nothing restricts
    assert band_margin([], [], 64, 100) is None
    assert band_margin(torch.tensor([5, 6], dtype=torch.int32), np.array([5, 5]), 8, 13) == 0
    assert band_margin([60, 62], [0, 0], 64, 65) == 1               # the upper edge alone


def test_banded_entry_points_are_declared_bound_and_exported():
    from ds2hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    assert 'banded CTC alignment' in hdr
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, res, nargs in (('ds2_ctc_align_banded_ws_bytes', 'size_t', 3), ('ds2_ctc_align_banded', 'int', 20)):
        m = re.search(r'\n\s*%s\s+%s\s*\(([^;]*?)\)\s*;' % (res, name), code)
        assert m, name + ' is not declared in include/ds2hip.h'
        assert len(m.group(1).split(',')) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(handle, name), name + ' is not exported'
    assert 'double* score' in re.search(r'int\s+ds2_ctc_align_banded\s*\(([^;]*?)\)\s*;', code).group(1)
    band_min = int(re.search(r'#define\s+DS2_ALIGN_BAND_MIN\s+(\d+)', hdr).group(1))
    band_max = int(re.search(r'#define\s+DS2_ALIGN_BAND_MAX\s+(\d+)', hdr).group(1))
    assert (band_min, band_max) == (lib.ALIGN_BAND_MIN, lib.ALIGN_BAND_MAX) and band_min == 64 and band_max in (4096, 8192)
    assert lib.query('ds2_ctc_align_banded_ws_bytes', 2, 10, 64) >= 2 * 10 * 64
    assert lib.query('ds2_ctc_align_banded_ws_bytes', 1, 180000, 4096) >= 180000 * 4096      # past 2^29: counted in size_t


@pytest.mark.parametrize('band', [0, 63, 96, 'twice the maximum'])
def test_bad_band_widths_are_refused_before_any_launch(band):
    from ds2hip import lib
    band = 2 * lib.ALIGN_BAND_MAX if isinstance(band, str) else band
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    rc = lib.load().ds2_ctc_align_banded(one, one, one, one, one, one, 1, 4, 3, 5, band, 0, 1, one, 1 << 30, one, one, one,
                                         one, None)
    assert rc == lib.ERR_ARG
    msg = lib.load().ds2_last_error()
    assert b'band %d' % band in msg and b'power of two' in msg


def test_small_workspace_and_other_arguments_are_refused_before_any_launch():
    from ds2hip import lib
    one = ctypes.c_void_p(16)
    fn = lib.load().ds2_ctc_align_banded
    rc = fn(one, one, one, one, one, one, 1, 4, 3, 5, 64, 0, 1, one, 8, one, one, one, one, None)
    assert rc == lib.ERR_ARG
    msg = lib.load().ds2_last_error()
    assert b'workspace' in msg and str(lib.query('ds2_ctc_align_banded_ws_bytes', 1, 4, 64)).encode() in msg
    big = 1 << 30
    for args in ((one, one, one, one, one, one, 1, 4, 257, 5, 64, 0, 1, one, big, one, one, one, one, None),     # A
                 (one, one, one, one, one, one, 1, 4, 3, 5, 64, 3, 1, one, big, one, one, one, one, None),       # blank
                 (one, one, one, one, one, one, -1, 4, 3, 5, 64, 0, 1, one, big, one, one, one, one, None),      # B
                 (one, one, one, one, one, one, 1, -4, 3, 5, 64, 0, 1, one, big, one, one, one, one, None),      # T
                 (one, one, one, one, one, one, 1, 4, 3, 1 << 30, 64, 0, 1, one, big, one, one, one, one, None),  # 2 L + 1
                 (one, one, one, one, one, None, 1, 4, 3, 5, 64, 0, 1, one, big, one, one, one, one, None),      # lo
                 (None, one, one, one, one, one, 1, 4, 3, 5, 64, 0, 1, one, big, one, one, one, one, None),      # probs
                 (one, one, one, one, one, one, 1, 4, 3, 5, 64, 0, 1, one, big, one, one, one, None, None),      # score
                 (one, one, one, one, one, one, 1, 4, 3, 5, 64, 0, 1, None, big, one, one, one, one, None)):     # ws
        assert fn(*args) == lib.ERR_ARG, args


def test_ctc_align_banded_refuses_cpu_tensors():
    from codes.align import LongAligner
    from ds2hip import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)                 # noqa: E731
    with pytest.raises(RuntimeError):
        ops.ctc_align_banded(torch.full((1, 4, 3), 1 / 3.), i32(4), i32(1, 2), i32(0), i32(2), 2,
                             torch.zeros((1, 4), dtype=torch.int32), 64)
    with pytest.raises(RuntimeError):
        LongAligner(['_', 'A', 'B']).align(torch.full((4, 3), 1 / 3.), [1, 2])
