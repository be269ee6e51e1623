"""The host reference for alignment with gaps (tests/align_gap_ref.py) against brute force, against the plain banded reference
at g = inf and on a constructed recording whose optimum can be proved by hand; ``codes.align.path_band``.  No GPU."""
import numpy as np
import pytest
import torch

from tests import align_banded_ref as bref
from tests import align_gap_ref as gref
from tests import align_ref

INF = float('inf')
SPACE = 1


def _quarters(rng, shape, lo=-12, hi=1, holes=0.0):
    x = (rng.integers(lo, hi, size=shape) / 4.0).astype(np.float32)
    if holes:
        x[rng.random(shape) < holes] = -np.inf
    return x


@pytest.mark.parametrize('w', [2, 3, 4])
def test_reference_is_the_joint_maximum(w):
    """Brute force over every (state path, per-frame gap choice) pair, T <= 7 and L <= 3: the reference, which decides the
    gap at each (t, s) on its own, finds the same score, path and gap frames -- the pointwise maximum is the joint one."""
    rng = np.random.default_rng(w)
    seen_gap = seen_none = 0
    for trial in range(60):
        t_n, n, a = int(rng.integers(1, 8)), int(rng.integers(0, 4)), 4
        labels = [int(v) for v in rng.integers(1, a, size=n)]
        space = SPACE if trial % 3 else -1
        g = [0.0, 0.25, 1.0, 3.0, INF][trial % 5]
        x = _quarters(rng, (t_n, a), holes=0.1 if trial % 2 else 0.0)
        lo = np.minimum(bref.staircase(t_n, (0, 1, 1, 2)), max(2 * n + 1 - w, 0)) if trial % 4 else np.zeros(t_n, dtype=np.int64)
        want = gref.brute_force(x, labels, lo, w, 0, space, g)
        for impl in (bref.masked_full, bref.windowed):
            got = gref.align_gap(x, labels, lo, w, 0, space, g, impl=impl)
            assert got[0] == want[0], (trial, impl.__name__, got, want)
            if want[1] is None:
                assert got[1] is None and got[2] is None
                continue
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (trial, impl.__name__, got, want)
        if want[1] is None:
            seen_none += 1
        else:
            seen_gap += int(want[2].any())
            el = gref.eligible(labels, space)
            assert el[want[1]][want[2] == 1].all()
    assert seen_gap >= 10 and seen_none >= 3


def test_infinite_penalty_is_the_plain_reference():
    rng = np.random.default_rng(5)
    for trial in range(30):
        t_n, n, a, w = int(rng.integers(0, 40)), int(rng.integers(0, 12)), 5, int(rng.integers(3, 30))
        labels = [int(v) for v in rng.integers(1, a, size=n)]
        x = _quarters(rng, (t_n, a), holes=0.05)
        lo = bref.diagonal(t_n, 2 * n + 1, w)
        for impl in (bref.masked_full, bref.windowed):
            sc, st = impl(align_ref.frame_terms(x, True), labels, lo, w, 0)
            got = gref.align_gap(x, labels, lo, w, 0, SPACE, INF, impl=impl)
            assert got[0] == sc
            if st is None:
                assert got[1] is None
            else:
                assert np.array_equal(got[1], st) and not got[2].any()


def test_eligibility():
    assert gref.eligible([], SPACE).tolist() == [True]
    assert gref.eligible([2, 3], SPACE).tolist() == [True, False, False, False, True]
    assert gref.eligible([2, 1, 3], SPACE).tolist() == [True, False, True, False, True, False, True]
    assert gref.eligible([2, 1, 3], -1).tolist() == [True, False, False, False, False, False, True]
    assert gref.eligible([1, 1], SPACE).tolist() == [True, False, True, False, True]


def constructed(n_ins=4):
    """'ab cb' (labels 2 3 1 4 3; 0 blank, 1 space, 5 a symbol the transcript lacks) spoken as blank / symbol frames in
    turn, every frame's own symbol at 0 and the rest at -8.  ``n_ins`` foreign frames (symbol 5 at 0, the NEXT label -- at
    the end the last -- at -2, the rest at -8) stand before the first frame, after the blank that follows the space, and
    after the last frame.  -> (clean (T0,6), dirty (T0 + 3 n_ins, 6), labels, is-inserted (T,) bool)."""
    labels = [2, 3, 1, 4, 3]
    seq = [0, 2, 0, 3, 0, 1, 0, 4, 0, 3, 0]
    clean = np.full((len(seq), 6), -8.0, dtype=np.float32)
    clean[np.arange(len(seq)), seq] = 0.0

    def block(near):
        b = np.full((n_ins, 6), -8.0, dtype=np.float32)
        b[:, 5], b[:, near] = 0.0, -2.0
        return b
    dirty = np.concatenate([block(2), clean[:7], block(4), clean[7:], block(3)])
    ins = np.zeros(len(dirty), dtype=bool)
    ins[:n_ins] = ins[n_ins + 7:2 * n_ins + 7] = ins[-n_ins:] = True
    return clean, dirty, labels, ins


def test_constructed_recording():
    """With g = 1 every path pays at most 0 on a clean frame (its row's maximum; f = -1 is below it) and at most -1 on an
    inserted one (the transcript's symbols are at -2 or -8 there, a gap at -1), so no path beats -3 n_ins; the bound is met
    only by taking each clean frame's own symbol -- which fixes the states 0..10 on the clean frames, each symbol having one
    state that fits between its neighbours -- and a gap on every inserted frame, which must then sit in an eligible blank:
    state 0, state 6 (between 6 and the label state 7) and state 10.  So the gap frames are exactly the inserted ones and
    every label's span is the clean case's, shifted.  Without gaps the clean spans would put all inserted frames into blank
    states at -8 each, -24 n_ins in all, while spending each block in the neighbouring label's state costs at most
    -2 n_ins - 8 per block: the spans move."""
    n_ins = 4
    clean, dirty, labels, ins = constructed(n_ins)
    w, s_n = 16, 11
    sc0, st0 = bref.masked_full(align_ref.frame_terms(clean, True), labels, np.zeros(len(clean), dtype=np.int64), w, 0)
    assert sc0 == 0.0 and st0.tolist() == list(range(11))
    starts0, ends0 = align_ref.spans(st0, len(labels))
    shift = np.array([n_ins] * 3 + [2 * n_ins] * 2)
    lo = np.zeros(len(dirty), dtype=np.int64)
    for impl in (bref.masked_full, bref.windowed):
        sc, st, gap = gref.align_gap(dirty, labels, lo, w, 0, SPACE, 1.0, impl=impl)
        assert sc == -3.0 * n_ins
        assert np.array_equal(gap.astype(bool), ins)
        starts, ends = align_ref.spans(st, len(labels))
        assert np.array_equal(starts, starts0 + shift) and np.array_equal(ends, ends0 + shift)
        assert set(st[ins].tolist()) == {0, 6, 10}
        # without gaps: a better path than the clean spans allow, and other spans
        sc_p, st_p, gap_p = gref.align_gap(dirty, labels, lo, w, 0, SPACE, INF, impl=impl)
        assert not gap_p.any() and -24.0 * n_ins < -3 * (2.0 * n_ins + 8) <= sc_p < sc
        starts_p, ends_p = align_ref.spans(st_p, len(labels))
        assert not (np.array_equal(starts_p, starts0 + shift) and np.array_equal(ends_p, ends0 + shift))
        assert starts_p[0] < n_ins and ends_p[-1] > len(dirty) - 1 - n_ins
    # end blanks only: the middle block cannot be absorbed, the other two still are
    sc, st, gap = gref.align_gap(dirty, labels, lo, w, 0, -1, 1.0)
    assert gap[:n_ins].all() and gap[-n_ins:].all() and not gap[n_ins:-n_ins].any()
    assert s_n == 2 * len(labels) + 1


def _path(rng, t_n, s_n):
    """A random monotone path from 0 to s_n - 1 with steps of 0, 1 or 2."""
    st = [0]
    for t in range(1, t_n):
        left = t_n - 1 - t
        lo_step = max(0, (s_n - 1 - st[-1]) - 2 * left)
        st.append(min(st[-1] + max(int(rng.integers(0, 3)), lo_step), s_n - 1))
    return np.array(st, dtype=np.int64)


def test_path_band_is_legal_and_a_fixed_point():
    from codes.align import path_band
    rng = np.random.default_rng(11)
    for trial in range(40):
        w = int(rng.choice([4, 8, 64]))
        s_n = int(rng.integers(1, 5 * w)) | 1
        t_n = int(rng.integers((s_n + 1) // 2 + 1, 3 * s_n + 4))
        st = _path(rng, t_n, s_n)
        if trial % 2:                                               # a long opening in state 0, then the rest
            opening = t_n - (s_n + 1) // 2 - 1
            st = np.concatenate([np.zeros(opening, dtype=np.int64), _path(rng, t_n - opening, s_n)])
        assert (np.diff(st) >= 0).all() and (np.diff(st) <= 2).all()
        lo = path_band(torch.from_numpy(st), w, s_n)
        assert lo.dtype == torch.int64
        lo = lo.numpy()
        want = np.maximum.accumulate(np.clip(st - w // 2, 0, max(s_n - w, 0)))
        assert np.array_equal(lo, want)
        assert not bref.band_is_bad(lo, w) and bref.in_band(st, lo, w)      # legal, and it holds the path
        assert (np.diff(lo) <= 2).all() and lo.max(initial=0) <= max(s_n - w, 0)
        # centred: away from the row's ends the path is w // 2 above lo
        mid = (st - w // 2 >= 0) & (st - w // 2 <= max(s_n - w, 0))
        assert (st[mid] - lo[mid] == w // 2).all()
        assert np.array_equal(path_band(torch.from_numpy(st), w, s_n).numpy(), lo)
    assert path_band(torch.zeros(0, dtype=torch.int32), 64, 9).numel() == 0


def test_path_band_fixed_point_of_realignment():
    """Aligning inside ``path_band(path)`` of the banded optimum's own path returns a path whose band is again legal; once
    two successive paths agree, so do their bands (the loop in LongAligner stops moving)."""
    from codes.align import path_band
    rng = np.random.default_rng(3)
    n, t_n, a, w = 20, 70, 6, 8
    labels = [int(v) for v in rng.integers(2, a, size=n)]
    x = _quarters(rng, (t_n, a), lo=-20, hi=1)
    x[:25, 0] = 0.5                                                   # a long opening that belongs to state 0
    s_n = 2 * n + 1
    lo = bref.diagonal(t_n, s_n, w)
    sc, st = bref.windowed(align_ref.frame_terms(x, True), labels, lo, w, 0)
    assert st is not None
    scores = [sc]
    for _ in range(12):
        lo = path_band(torch.from_numpy(st), w, s_n).numpy()
        assert not bref.band_is_bad(lo, w) and bref.in_band(st, lo, w)
        sc2, st2 = bref.windowed(align_ref.frame_terms(x, True), labels, lo, w, 0)
        assert sc2 >= scores[-1]                                      # the old path is still admissible
        scores.append(sc2)
        if np.array_equal(st2, st):
            assert np.array_equal(path_band(torch.from_numpy(st2), w, s_n).numpy(), lo)
            break
        st = st2
    else:
        raise AssertionError('no fixed point in 12 rounds: %r' % scores)
    assert scores[-1] > scores[0]                                     # re-centring found a better path than the diagonal band
