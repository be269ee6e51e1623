"""Every form of ds2_gemm_f32 and ds2_gemm_f32_tn_group at its dispatch edges, against references that need no tolerance.

The cases, the operand builders and the references are tests/gemm_cases.py (checked on the CPU by test_gemm_cases_cpu.py).
Every operand of every case sits inside a buffer of its own whose other floats are NaN (A, B) or a sentinel bit pattern (C):
nothing outside op(A), op(B) may reach C, nothing outside C may change.  The tests assert results only, never which kernel
ran.  One pytest case is one set of operands, launched once per kernel family.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
HOST_REF_LIMIT = 2e8            # m n k above which the fp64 reference product runs on the device


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def family(ops):
    """use(f) selects the kernel family of ds2_gemm_f32 (0: f32-input MFMA, 6 / 9: bf16 split-operand kernels); the family in
    effect before the test is restored whatever happens."""
    before = ops.gemm_split_mode()

    def use(f):
        assert ops.gemm_split_mode(f) == f
        return f
    try:
        yield use
    finally:
        ops.gemm_split_mode(before)


class Dev:
    """an Embedded view on the device"""

    def __init__(self, emb):
        self.emb = emb
        self.host = torch.from_numpy(emb.buf)
        self.t = self.host.to(DEV, copy=True)
        self.ptr = self.t.data_ptr() + 4 * emb.start
        assert self.t.data_ptr() % 16 == 0

    def view(self, t=None):
        e = self.emb
        return torch.as_strided(self.t if t is None else t, (e.rows, e.cols), (e.ld, 1), e.start)

    def rows2d(self):
        """contiguous (rows, ld) tensor that starts at the view (for ops.gemm); its last row reaches into the tail guard"""
        e = self.emb
        return self.t[e.start: e.start + e.rows * e.ld].view(e.rows, e.ld)

    def reset(self):
        self.t.copy_(self.host)

    def check_outside(self, what):
        """every byte outside the view is what it was: the buffer equals (original with the view's floats replaced)"""
        want = self.host.to(DEV, copy=True)
        self.view(want).copy_(self.view())
        assert torch.equal(want.view(torch.int32), self.t.view(torch.int32)), '%s: C changed outside its view' % what


def _operands(case, family_, slots, cache):
    m, n, k = case.dims(slots)
    lda, ldb, ldc = case.lds(slots, family_)
    key = (lda, ldb, ldc)
    if key in cache:
        return cache[key]
    if 'ops' not in cache:
        opa, opb, extra = gc.make_ops(case.ref, m, n, k, case.seed(), gc.kper_of(k, case.split_k))
        clean_a, clean_b = opa, opb
        spot = None
        if case.poison:
            m0, n0, k0 = 77, 150, k - 3
            val = np.float32(np.nan if case.poison.startswith('nan') else np.inf)
            if case.poison.endswith('A'):
                clean_a, opa = opa.copy(), opa.copy()
                opa[m0, k0], clean_a[m0, k0], spot = val, 0.0, ('row', m0)
            else:
                clean_b, opb = opb.copy(), opb.copy()
                opb[k0, n0], clean_b[k0, n0], spot = val, 0.0, ('col', n0)
        c0 = gc.c_prefill(np.random.default_rng(case.seed() + 1), m, n)
        if m * n * k <= HOST_REF_LIMIT:
            ref = gc.reference(case.ref, clean_a, clean_b, extra)
            bound = gc.fp64_bound(opa, opb, k, 0) / (k + 2) if case.ref == 'fp64' else None      # (|a| @ |b|) 2^-24
            ref = torch.from_numpy(np.asarray(ref, np.float64))
            bound = None if bound is None else torch.from_numpy(bound).to(DEV)
            ref = ref.to(DEV)
        else:
            assert case.ref in ('int', 'fp64') and not case.poison
            da, db = torch.from_numpy(opa).to(DEV).double(), torch.from_numpy(opb).to(DEV).double()
            ref = da @ db
            bound = (da.abs() @ db.abs()) * 2.0 ** -24 if case.ref == 'fp64' else None
            del da, db
        if case.beta:
            ref = ref + torch.from_numpy(c0).to(DEV).double()
        cache['ops'] = (opa, opb, c0, ref, bound, spot)
    opa, opb, c0, ref, bound, spot = cache['ops']
    sa, sb = gc.stored(opa, case.ta), gc.stored(opb, case.tb)
    a = Dev(gc.Embedded(sa.shape[0], sa.shape[1], lda, case.a_off, 'nan').put(sa))
    b = Dev(gc.Embedded(sb.shape[0], sb.shape[1], ldb, case.b_off, 'nan').put(sb))
    c = Dev(gc.Embedded(m, n, ldc, 0, 'sentinel').put(c0))
    cache[key] = (a, b, c, ref, bound, spot)
    return cache[key]


def _launch(ops, case, a, b, c, m, n, k):
    if case.section in ('edgeM', 'edgeN', 'slabs', 'auto', 'fp64', 'stat', 'select'):
        ops.gemm(a.rows2d(), b.rows2d(), trans_a=bool(case.ta), trans_b=bool(case.tb), out=c.rows2d(), beta=float(case.beta),
                 m=m, n=n, k=k, lda=a.emb.ld, ldb=b.emb.ld, ldc=c.emb.ld, split_k=case.split_k)
    else:
        ops.gemm_raw(case.ta, case.tb, m, n, k, a.ptr, a.emb.ld, b.ptr, b.emb.ld, c.ptr, c.emb.ld, beta=float(case.beta),
                     split_k=case.split_k)


def _mismatch(got, ref):
    bad = (got.double() != ref).nonzero()
    return '%d wrong of %d, first at %s: got %r, want %r' % (
        len(bad), ref.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())


EXACT = [c for c in gc.single_cases() if c.ref in ('int', 'selA', 'selB') and not c.poison]


@pytest.mark.parametrize('case', EXACT, ids=lambda c: c.name)
def test_gemm_exact(ops, family, slots, case):
    """integer and selection references: C equals the reference exactly in every family, whichever kernel the launcher picks,
    with or without atomics; NaN around A and B stays out of C; the sentinel around C stays"""
    m, n, k = case.dims(slots)
    cache = {}
    for f in case.families:
        a, b, c, ref, _, _ = _operands(case, f, slots, cache)
        c.reset()
        family(f)
        _launch(ops, case, a, b, c, m, n, k)
        got = c.view()
        assert torch.equal(got.double(), ref), 'family %d (%s): %s' % (f, gc.expected_form(case, f, slots).kernel, _mismatch(got, ref))
        c.check_outside('family %d' % f)


def _pieces(case, f, slots):
    return gc.pieces_per_output(gc.expected_form(case, f, slots))


@pytest.mark.parametrize('case', gc.fp64_cases(), ids=lambda c: c.name)
def test_gemm_fp64_bound(ops, family, slots, case):
    """general N(0, 1) operands: |c - ref| <= (K + S + 2) 2^-24 (|a| @ |b|) elementwise (gemm_cases.fp64_bound: rigorous and
    order-free for an fp32 accumulator; S = atomically added pieces).  Measured on an MI355X, max over the elements of
    |c - ref| / bound (printed with -s): family 0 0.22 / 0.14 / 0.08 at K = 16 / 32 / 48, families 6 and 9 0.10 / 0.05 / 0.04
    (their 16-term instruction rounds less often than the f32 one's chain), all three 0.002 at K = 1000 in three pieces.  The
    constant is the derived one for every family: nothing was doubled."""
    m, n, k = case.dims(slots)
    cache = {}
    for f in case.families:
        a, b, c, ref, unit, _ = _operands(case, f, slots, cache)
        c.reset()
        family(f)
        _launch(ops, case, a, b, c, m, n, k)
        bound = (k + _pieces(case, f, slots) + 2) * unit
        ratio = float(((c.view().double() - ref).abs() / bound).max())
        print('%s family %d: max |c - ref| / bound = %.4f' % (case.name, f, ratio))
        assert ratio <= 1.0, (f, ratio)
        c.check_outside('family %d' % f)


@pytest.mark.parametrize('case', gc.STAT_CASES, ids=lambda c: c.name)
def test_gemm_split_families_no_worse_than_f32(ops, family, slots, case):
    """the project's statistical rule (test_gemm_split_operand_kernels_are_as_accurate_as_the_f32_kernels): max and rms error
    relative to |a| @ |b| of families 6 and 9 are at most 1.25 x family 0's on the same operands"""
    m, n, k = case.dims(slots)
    cache = {}
    err = {}
    for f in (0, 6, 9):
        a, b, c, ref, unit, _ = _operands(case, f, slots, cache)
        c.reset()
        family(f)
        _launch(ops, case, a, b, c, m, n, k)
        e = (c.view().double() - ref).abs() / (unit * 2.0 ** 24)
        err[f] = (float(e.max()), float(e.pow(2).mean().sqrt()))
    print(case.name, err)
    for f in (6, 9):
        assert err[f][0] <= 1.25 * err[0][0] + 1e-8, err
        assert err[f][1] <= 1.25 * err[0][1] + 1e-9, err


@pytest.mark.parametrize('case', gc.nonfinite_cases(), ids=lambda c: c.name)
def test_gemm_nonfinite_stays_in_its_row_or_column(ops, family, slots, case):
    """one NaN or +Inf in op(A)[m0, k0] makes row m0 of C non-finite in every column and leaves every other element exact; the
    same for a column through op(B)[k0, n0] (family 0 gives Inf or NaN, the split families NaN: Inf - Inf enters the second
    term)"""
    m, n, k = case.dims(slots)
    cache = {}
    for f in case.families:
        a, b, c, ref, _, (axis, idx) = _operands(case, f, slots, cache)
        c.reset()
        family(f)
        _launch(ops, case, a, b, c, m, n, k)
        got = c.view().double()
        keep = torch.ones(m if axis == 'row' else n, dtype=torch.bool, device=DEV)
        keep[idx] = False
        if axis == 'row':
            assert not torch.isfinite(got[idx, :]).any(), 'family %d' % f
            assert torch.equal(got[keep, :], ref[keep, :]), 'family %d' % f
        else:
            assert not torch.isfinite(got[:, idx]).any(), 'family %d' % f
            assert torch.equal(got[:, keep], ref[:, keep]), 'family %d' % f
        c.check_outside('family %d' % f)


# --------------------------------------------------------------------------------------------- the grouped launch
@pytest.mark.parametrize('case', gc.group_cases(), ids=lambda c: c.name)
def test_gemm_tn_group_exact(ops, family, case):
    """C_p = A_p^T B_p for up to four problems in one launch, exact in every family; accumulate = False overwrites the
    prefilled C, accumulate = True adds to it"""
    lds = case.lds()
    probs = []
    for p, m in enumerate(case.ms):
        opa, opb, extra = gc.make_ops(case.ref, m, case.n, case.k, case.seed() + p)
        if case.share_b and p > 0:
            opb = probs[0]['opb']
        ref = torch.from_numpy(np.asarray(gc.reference(case.ref, opa, opb, extra), np.float64)).to(DEV)
        c0 = gc.c_prefill(np.random.default_rng(case.seed() + 100 + p), m, case.n)
        lda, ldb, ldc = lds[p]
        a = Dev(gc.Embedded(case.k, m, lda, 0, 'nan').put(gc.stored(opa, 1)))
        b = probs[0]['b'] if (case.share_b and p > 0) else Dev(gc.Embedded(case.k, case.n, ldb, 0, 'nan').put(opb))
        c = Dev(gc.Embedded(m, case.n, ldc, 0, 'sentinel').put(c0))
        probs.append(dict(opb=opb, a=a, b=b, c=c, ref=ref, c0=torch.from_numpy(c0).to(DEV).double()))
    args = [(q['a'].ptr, q['a'].emb.ld, m, q['b'].ptr, q['b'].emb.ld, q['c'].ptr, q['c'].emb.ld) for q, m in zip(probs, case.ms)]
    for f in case.families:
        family(f)
        for accumulate in (False, True):
            exact_sum = case.ref == 'int'                  # (a selection's values added to integers would round: add to zeros)
            for q in probs:
                q['c'].reset()
                if accumulate and not exact_sum:
                    q['c'].view().zero_()
            ops.gemm_tn_group(args, case.n, case.k, accumulate=accumulate)
            for p, q in enumerate(probs):
                want = q['ref'] + q['c0'] if accumulate and exact_sum else q['ref']
                got = q['c'].view()
                what = 'family %d, accumulate %s, problem %d' % (f, accumulate, p)
                assert torch.equal(got.double(), want), '%s: %s' % (what, _mismatch(got, want))
                q['c'].check_outside(what)


# --------------------------------------------------------------------------------------------- refusals
def _group_raw(count, a, lda, m, b, ldb, c, ldc, n, k, accumulate=0):
    """ds2_gemm_f32_tn_group without the Python wrapper's own argument check (the count itself is under test)"""
    from ds2hip import lib
    cnt = len(a)
    vp, ip = ctypes.c_void_p * cnt, ctypes.c_int * cnt
    args = (vp(*a), ip(*lda), ip(*m), vp(*b), ip(*ldb), vp(*c), ip(*ldc))
    rc = lib.load().ds2_gemm_f32_tn_group(count, *[ctypes.cast(x, ctypes.c_void_p) for x in args], n, k, accumulate,
                                          lib.stream_ptr())
    if rc != 0:
        raise lib.Ds2Error(rc, lib.load().ds2_last_error().decode())


@pytest.mark.parametrize('fam', [0, 6, 9])
def test_gemm_refusals_launch_nothing(ops, family, fam):
    """bad arguments come back as lib.Ds2Error and C keeps every bit"""
    from ds2hip import lib
    family(fam)
    m, n, k = 32, 48, 16
    rng = np.random.default_rng(5)
    a = Dev(gc.Embedded(m, k, k, 0, 'nan').put(gc.int_matrix(rng, (m, k), 7)))
    b = Dev(gc.Embedded(n, k, k, 0, 'nan').put(gc.int_matrix(rng, (n, k), 7)))
    c = Dev(gc.Embedded(m, n, n, 0, 'sentinel').put(gc.c_prefill(rng, m, n)))

    def refused(code, fn, *args, **kw):
        with pytest.raises(lib.Ds2Error) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, ei.value
        torch.cuda.synchronize()
        assert torch.equal(c.t.view(torch.int32), c.host.to(DEV).view(torch.int32))

    raw = ops.gemm_raw
    refused(lib.ERR_ARG, raw, 0, 1, m, n, k, a.ptr, k, b.ptr, k, c.ptr, n, beta=0.5)
    refused(lib.ERR_ARG, raw, 0, 1, m, n, k, a.ptr, k - 1, b.ptr, k, c.ptr, n)
    refused(lib.ERR_ARG, raw, 0, 1, m, n, k, a.ptr, k, b.ptr, k, c.ptr, n - 1)
    refused(lib.ERR_ARG, raw, 0, 1, 0, n, k, a.ptr, k, b.ptr, k, c.ptr, n)
    refused(lib.ERR_ARG, raw, 0, 1, m, n, k, a.ptr, k, b.ptr, k, c.ptr, n, split_k=-1)
    # the 2 GB guard, reached with dimensions only: checked before any memory is touched
    refused(lib.ERR_UNSUPPORTED, raw, 0, 1, 2, 16, 16, a.ptr, 2 ** 29, b.ptr, 16, c.ptr, 16)
    # the grouped launch: A_p is k x m_p, B_p k x n -- here (16 x 32) and (16 x 48) read out of the same buffers
    one = dict(a=[a.ptr], lda=[m], m=[m], b=[b.ptr], ldb=[n], c=[c.ptr], ldc=[n])
    refused(lib.ERR_ARG, _group_raw, 0, n=n, k=k, **one)
    five = {key: val * 5 for key, val in one.items()}
    refused(lib.ERR_ARG, _group_raw, 5, n=n, k=k, **five)
    two = {key: val * 2 for key, val in one.items()}
    two['m'] = [m, 0]
    refused(lib.ERR_ARG, _group_raw, 2, n=n, k=k, **two)
