"""The GEMM edge suite's cases are what they claim to be (tests/gemm_cases.py); no GPU.

The exactness arguments of the integer and selection references, the embedded layout's power to expose a read outside an
operand or a write outside C, the coverage of the launcher's forms by the case table, and the fp64 bound's room for a plain
fp32 accumulator are all checked here, so that a red GPU test speaks about the kernels and a green one about all of them."""
import collections

import numpy as np
import pytest

from tests import gemm_cases as gc
from tests.test_split_cpu import split3

SINGLE = gc.single_cases()
GROUPS = gc.group_cases()


def test_case_names_are_unique():
    names = [c.name for c in SINGLE + GROUPS]
    assert len(names) == len(set(names))


def test_integer_cases_stay_below_2_pow_24():
    ks = sorted({c.dims(512)[2] for c in SINGLE if c.ref == 'int'} | {c.k for c in GROUPS if c.ref == 'int'})
    for k in ks:
        amax, bmax = gc.int_ranges(k)
        assert 2 * amax * bmax * k < 2 ** 24, k
        # the prefilled C of beta = 1 / accumulate (|c0| <= 1000) fits beside the largest true sum
        assert amax * bmax * k + 1000 < 2 ** 24
        rng = np.random.default_rng(k)
        a, b = gc.int_matrix(rng, (64, k), amax), gc.int_matrix(rng, (k, 64), bmax)
        assert np.abs(a).max() <= amax and np.abs(b).max() <= bmax
        assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))
        # values that need a second bf16 term: odd and above 256
        assert np.any((np.abs(a) > 256) & (a.astype(np.int64) % 2 != 0))
        a1, a2, a3 = split3(a)
        assert np.any(a2 != 0)
        # every split term of an integer below 2^10 is an integer, and bf16(a) is at most twice |a|
        assert np.array_equal(a1, np.round(a1)) and np.array_equal(a2, np.round(a2)) and not a3.any()
        assert np.abs(a1).max() <= 2 * amax
        ref = gc.reference('int', a, b)
        assert np.array_equal(ref, (a.astype(np.int64) @ b.astype(np.int64)).astype(np.float64))


def _selection_cases():
    out = []
    for c in SINGLE:
        if c.ref in ('selA', 'selB'):
            m, n, k = c.dims(512)
            out.append((c.name, c.ref, m, n, k, gc.kper_of(k, c.split_k), c.seed()))
    for c in GROUPS:
        if c.ref in ('selA', 'selB'):
            for p, m in enumerate(c.ms):
                out.append(('%s[%d]' % (c.name, p), c.ref, m, c.n, c.k, gc.BK, c.seed() + p))
    return out


@pytest.mark.parametrize('name,ref,m,n,k,kper,seed', _selection_cases(), ids=[s[0] for s in _selection_cases()])
def test_selection_cases_select(name, ref, m, n, k, kper, seed):
    opa, opb, (pi, sg) = gc.make_ops(ref, m, n, k, seed, kper)
    sel, arb = (opb, opa) if ref == 'selA' else (opa.T, opb)                # sel: K x columns
    assert sel.shape[0] == k
    assert np.all((sel != 0).sum(axis=0) == 1) and set(np.unique(sel)) == {-1.0, 0.0, 1.0}
    assert np.array_equal(np.abs(sel).argmax(axis=0), pi) and np.array_equal(sel[pi, np.arange(sel.shape[1])], sg)
    hit = set(pi.tolist())
    if sel.shape[1] >= k:
        assert hit == set(range(k))
    for kk in gc.boundaries(k, kper):                                         # both sides of every slab and split boundary
        assert kk in hit, kk
    for b in range(kper, k, kper):
        assert b - 1 in hit and b in hit
    # the arbitrary operand: finite, no zero of either sign, all 24 bits in use, split terms normal, split error-free
    assert np.all(np.isfinite(arb)) and np.all(arb != 0)
    assert np.all(arb.view(np.uint32) & 1 == 1)
    e = np.frexp(arb)[1]
    assert e.min() < -60 and e.max() > 60
    a1, a2, a3 = split3(arb)
    tiny = 2.0 ** -126
    assert np.all(np.abs(a1) >= tiny) and np.all((a2 == 0) | (np.abs(a2) >= tiny)) and np.all((a3 == 0) | (np.abs(a3) >= 2.0 ** -124))
    assert np.count_nonzero(a3) > 0.9 * a3.size
    assert np.array_equal(a1.astype(np.float64) + a2.astype(np.float64) + a3.astype(np.float64), arb.astype(np.float64))
    assert np.array_equal((a3 + a2) + a1, arb)                                # the accumulators' order: a1 + (a3 + a2), in fp32
    # the reference is the fp64 product, exactly
    ref_c = gc.reference(ref, opa, opb, (pi, sg))
    assert ref_c.dtype == np.float32
    assert np.array_equal(ref_c.astype(np.float64), opa.astype(np.float64) @ opb.astype(np.float64))


# --------------------------------------------------------------------------------------------- the embedded layout
@pytest.mark.parametrize('rows,cols,ld,offset', [(5, 7, 7, 0), (5, 7, 12, 0), (5, 7, 8, 1), (1, 1, 4, 0), (33, 16, 17, 1)])
def test_embedded_layout(rows, cols, ld, offset):
    rng = np.random.default_rng(rows * 100 + ld)
    mat = rng.standard_normal((rows, cols)).astype(np.float32)
    e = gc.Embedded(rows, cols, ld, offset, 'nan').put(mat)
    assert np.array_equal(e.view(), mat)                                      # the view round-trips
    assert e.start == gc.FRONT + offset and e.start >= 64
    assert e.size - (e.start + (rows - 1) * ld + cols) >= 48 * ld + 64        # tail guard
    inside = e.inside()
    assert inside.sum() == rows * cols and np.all(np.isnan(e.buf[~inside])) and np.all(np.isfinite(e.buf[inside]))
    for r in range(rows):
        assert np.array_equal(e.buf[e.start + r * ld: e.start + r * ld + cols], mat[r])
    # a read of ANY guard or pad float turns a product into NaN: walk every outside position a widened or shifted view reaches
    other = np.ones((cols, 3), np.float32)
    assert np.all(np.isfinite(e.view() @ other))
    wide = np.lib.stride_tricks.as_strided(e.buf[e.start:], (rows, ld), (4 * ld, 4))
    if ld > cols:
        for c in range(cols, ld):
            assert np.all(np.isnan(wide[:, c:c + 1] @ np.ones((1, 2), np.float32)))       # every pad column
    before = np.lib.stride_tricks.as_strided(e.buf[e.start - 1:], (rows, cols), (4 * ld, 4))
    assert np.isnan(before @ other).any()                                     # one float early: the front guard
    below = np.lib.stride_tricks.as_strided(e.buf[e.start:], (rows + 48, cols), (4 * ld, 4))
    assert np.all(np.isnan((below @ other)[rows:]))                           # rows behind the operand: the tail guard
    for pos in np.flatnonzero(~inside):
        assert np.isnan(e.buf[pos])

    # C: a write outside the view is detected, one inside is not
    c = gc.Embedded(rows, cols, ld, 0, 'sentinel').put(mat)
    assert np.all(np.isfinite(c.buf))
    assert c.outside_intact(c.buf)
    out = c.buf.copy()
    c.view(out)[...] = 0
    assert c.outside_intact(out)
    for pos in (0, c.start - 1, c.start + cols if ld > cols else c.start + c.span, c.start + c.span, c.size - 1):
        bad = c.buf.copy()
        bad[pos] = 0.0
        assert not c.outside_intact(bad), pos
    # what a linear fill in place of the 2-D one would do: rows * cols contiguous zeros from the view's start
    if ld > cols and rows > 1:
        bad = c.buf.copy()
        bad[c.start: c.start + rows * cols] = 0.0
        assert not c.outside_intact(bad)


def test_ld_modes():
    assert gc.ld_of(161, 'tight') == 161 and gc.ld_of(161, 'pad4') == 168 and gc.ld_of(160, 'pad4') == 164
    assert gc.ld_of(48, 'odd') == 49 and gc.ld_of(130, 'odd') == 133 and gc.ld_of(161, 'pad1') == 162
    for w in range(1, 40):
        assert gc.ld_of(w, 'pad4') % 4 == 0 and gc.ld_of(w, 'pad4') > w and gc.ld_of(w, 'odd') % 4 == 1 and gc.ld_of(w, 'odd') > w


# --------------------------------------------------------------------------------------------- coverage of the forms
def _forms():
    table = collections.Counter()
    zero = collections.Counter()
    bodies = collections.Counter()
    for c in SINGLE:
        for f in c.families:
            form = gc.expected_form(c, f, slots=512)
            table[form.kernel + ('+atomic' if form.atomic else '')] += 1
            zero[form.zero] += 1
            for b in form.bodies:
                bodies[(form.family(), b)] += 1
    for c in GROUPS:
        for f in c.families:
            for acc in (False, True):
                form = gc._expected_group(c, f, acc)
                table[form.kernel] += 1
                zero[form.zero] += 1
                for b in form.bodies:
                    bodies[(form.family(), b)] += 1
    return table, zero, bodies


def test_every_form_has_cases():
    table, zero, bodies = _forms()
    print()
    for name in sorted(table):
        print('%-28s %4d' % (name, table[name]))
    for name in sorted(zero):
        print('zero_rows: %-17s %4d' % (name, zero[name]))
    for fam, b in sorted(bodies):
        print('edge-tile body %d in %-8s %4d' % (b, fam, bodies[(fam, b)]))
    want = []
    for tr in ('NN', 'NT', 'TN', 'TT'):
        for fam in (6, 9):
            want += ['bf16x%d-%s' % (fam, tr), 'bf16x%d-%s+atomic' % (fam, tr)]
        want += ['f32-vec-' + tr, 'f32-novec-' + tr]
    # (a v2 launch always has stream-K pieces and data-parallel workgroups: see expected_form)
    want += ['v2-vec-TN+atomic', 'v2-novec-TN+atomic', 'v2-vec-NT+atomic', 'v2-novec-NT+atomic']
    want += ['group-bf16x6', 'group-bf16x9', 'group-f32-vec', 'group-f32-novec']
    for w in want:
        assert table[w] > 0, w
    assert zero['linear'] > 0 and zero['2d'] > 0 and zero['none'] > 0
    for fam in ('bf16x6', 'bf16x9', 'f32', 'group'):
        for b in (0, 1, 2):
            assert bodies[(fam, b)] > 0, (fam, b)


def test_mirror_on_known_dispatches():
    """spot values worked out by hand from launch()"""
    f = gc.expected_form(gc.Case('x', 1, 0, 130, 161, 1000, split_k=3), 6)
    assert (f.kernel, f.atomic, f.nsplit, f.zero) == ('bf16x6-TN', True, 3, 'linear')            # kper 336
    f = gc.expected_form(gc.Case('x', 1, 0, 130, 161, 1000, split_k=4, ldc='pad1'), 0)
    assert (f.kernel, f.atomic, f.nsplit, f.zero) == ('f32-vec-TN', True, 4, '2d')               # kper 256
    f = gc.expected_form(gc.Case('x', 0, 1, 130, 161, 40, split_k=4), 9)
    assert (f.kernel, f.nsplit) == ('f32-vec-NT', 3)                                             # K % 16: out of the split family
    f = gc.expected_form(gc.Case('x', 1, 0, 128, 128, 10247, split_k=0), 6)
    assert (f.kernel, f.nsplit) == ('bf16x6-TN', 31)                                             # cap 32, kper 336
    f = gc.expected_form(gc.Case('x', 1, 0, 128, 128, 10247, split_k=0), 0)
    assert (f.kernel, f.nsplit) == ('f32-vec-TN', 31)
    f = gc.expected_form(gc.Case('x', 1, 0, 128 * 23, 128 * 23, 512, split_k=0), 0)
    assert f.stream_k                                              # no split; 529 tiles on 512 slots, 32 slabs: the stream-K form
    assert not gc.expected_form(gc.Case('x', 1, 0, 128 * 23, 128 * 23, 512, split_k=0, beta=1), 0).atomic
    f = gc.expected_form(gc.Case('x', 1, 0, 128 * 23, 128 * 23, 2048, split_k=0), 0)
    assert f.atomic and f.nsplit == 6                                                            # 8192 / 529 = 15, K / 320 = 6
    f = gc.expected_form(gc.Case('x', 1, 0, 128 * 23, 128 * 23, 2048, split_k=0), 6)
    assert not f.atomic                                                                          # 1024 / 529 = 1
    sk = gc.Case('x', 0, 1, 0, 256, 384, sk='half+1')
    assert sk.dims(512)[0] == 128 * 257 and gc.expected_form(sk, 0).stream_k and not gc.expected_form(sk, 6).stream_k
    assert not gc.expected_form(gc.Case('x', 0, 1, 0, 256, 240, sk='half+1'), 0).stream_k        # 15 slabs
    assert not gc.expected_form(gc.Case('x', 0, 1, 0, 256, 384, sk='half+1', beta=1), 0).stream_k
    sk = gc.Case('x', 0, 1, 0, 256, 384, sk='half+1', odd_lda_family=6)
    assert gc.expected_form(sk, 6).kernel == 'v2-novec-NT'
    sk = gc.Case('x', 1, 0, 0, 384, 256, sk='2s-1')
    assert cdiv_tiles(sk) == 2 * 512 - 1 and gc.expected_form(sk, 0).stream_k


def cdiv_tiles(case):
    m, n, _ = case.dims(512)
    return gc.cdiv(m, 128) * gc.cdiv(n, 128)


# --------------------------------------------------------------------------------------------- the fp64 bound
def _fma_chain(opa, opb, k0, k1):
    """one fp32 accumulator, k order, one rounding per term (fmaf)"""
    acc = np.zeros((opa.shape[0], opb.shape[1]), np.float32)
    a64, b64 = opa.astype(np.float64), opb.astype(np.float64)
    for kk in range(k0, k1):
        acc = (acc.astype(np.float64) + a64[:, kk, None] * b64[None, kk, :]).astype(np.float32)
    return acc


def _pairwise(opa, opb, k0, k1):
    """fp32 products, then a pairwise fp32 tree"""
    terms = [(opa[:, kk, None] * opb[None, kk, :]).astype(np.float32) for kk in range(k0, k1)]
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


@pytest.mark.parametrize('case', [c for c in gc.fp64_cases() if (c.ta, c.tb) == (0, 1)], ids=lambda c: c.name)
def test_fp64_bound_holds_for_a_plain_fp32_accumulator(case):
    m, n, k = case.dims()
    opa, opb, _ = gc.make_ops('fp64', m, n, k, case.seed())
    ref = gc.reference('fp64', opa, opb)
    kper = gc.kper_of(k, case.split_k)
    nsplit = gc.cdiv(k, kper)
    pieces = nsplit if nsplit > 1 else 0
    bound = gc.fp64_bound(opa, opb, k, pieces)
    assert np.all(bound > 0)
    for chain in (_fma_chain, _pairwise):
        c = np.zeros((m, n), np.float32)
        for s in range(nsplit):
            part = chain(opa, opb, s * kper, min(k, (s + 1) * kper))
            c = part if nsplit == 1 else c + part
        ratio = float((np.abs(c.astype(np.float64) - ref) / bound).max())
        print('%s %s: max |c - ref| / bound = %.3f' % (case.name, chain.__name__, ratio))
        assert ratio <= 1.0
