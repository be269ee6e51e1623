"""The kernels around the big ones -- the tail of a training step (csrc/optim.hip), the decode head and the layout helpers
(csrc/misc.hip), the frontend (csrc/spectrogram.hip) -- against the plain references of tests/small_refs.py: exact where the
arithmetic allows it, within a derived float32 bound elsewhere, at the sizes where their grids, loops and branches change.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import small_refs as refs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24                    # unit roundoff of float32: one rounding to nearest loses at most U of the result


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from ds2hip import lib as _lib
    _lib.load()
    return _lib


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# =========================================================================================== 1. sumsq
SS_STRIDE4 = 1024 * 256           # float4s one pass of sumsq's capped grid covers (SS_BLOCKS x 256 threads, csrc/optim.hip)
SS_CAPPED = 4 * SS_STRIDE4 + 4 * 77 + 3          # past the cap: a partial second stride of 77 float4s and a 3-float tail
SS_FLUSH = 4 * (SS_STRIDE4 * 65) + 7             # 65 float4s per thread: one `cnt == 64` flush and one more trip (273 MB)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 100003, SS_CAPPED, SS_FLUSH])
def test_sumsq_is_exact_on_small_integers(ops, n):
    """Integers in [-3, 3]: a thread adds at most 64 * 4 products of at most 9 between two flushes (2304 < 2^24) and the whole
    sum is below 9 * 6.9e7 < 2^53, so every fp32 partial and the fp64 combine are exact and the result must EQUAL the integer
    sum: a dropped tail, a block or a stride counted twice or not at all changes it.

    The last size is the only one that reaches the `cnt == 64` flush (n / 4 > 1024 * 256 * 64, n > 67.1 M floats).  The model's
    flat gradient (codes/engine.py ``gflat``) has 38.07 M elements -- 37 float4s per thread -- and a multi-task model adds
    800 x A per head: training never reaches the flush, that branch is library-only."""
    torch.manual_seed(n % 1000)
    xi = torch.randint(-3, 4, (n,), dtype=torch.int8, device=DEV)
    x = xi.float()
    want = int((xi.to(torch.int32) * xi.to(torch.int32)).sum(dtype=torch.int64).item())
    got = float(ops.sumsq(x).item())
    assert got == float(want), (n, got, want)


def test_sumsq_counts_every_element_once_at_the_edges_of_its_strides(ops):
    """One 3 in an all-zero buffer of the capped size is worth exactly 9 wherever it sits: the first element, either side of
    the first stride's end, the last float4, the first tail element, the last element."""
    n, n4 = SS_CAPPED, SS_CAPPED // 4
    x = torch.zeros(n, device=DEV)
    for i in (0, 4 * SS_STRIDE4 - 1, 4 * SS_STRIDE4, 4 * n4 - 1, 4 * n4, n - 1):
        x[i] = 3.0
        got = float(ops.sumsq(x).item())
        x[i] = 0.0
        assert got == 9.0, (i, got)
    assert float(ops.sumsq(x).item()) == 0.0


@pytest.mark.parametrize('n', [100003, SS_CAPPED])
def test_sumsq_of_normals_within_the_fp32_run_bound(ops, n):
    """rtol = 260 U.  A thread's fp32 accumulator takes at most 64 trips between two flushes, each trip 4 products (one
    rounding each) and 4 additions (three inside the trip, one into the accumulator), and block 0's threads at most one tail
    element more: <= 257 non-negative terms, each rounded once as a product and passing through <= 256 roundings as part of a
    sum.  For non-negative terms the error of such a run is at most gamma_257 = 257 U / (1 - 257 U) < 260 U of the sum,
    whatever the order (and less where the compiler fuses a product into the addition).  The partials are then combined in
    fp64: ~20 roundings of 2^-53, nothing at this level.  The reference is the fp64 sum of the fp64 squares."""
    torch.manual_seed(n % 1000)
    x = torch.randn(n, device=DEV)
    want = float((x.double() * x.double()).sum().item())
    got = float(ops.sumsq(x).item())
    print('sumsq n=%d: relative error %.3g U (bound 260 U)' % (n, abs(got - want) / want / U))
    assert abs(got - want) <= 260 * U * want, (n, got, want)


# =========================================================================================== 2. clip_sgd_nesterov
CS_STRIDE4 = 2048 * 256           # float4s one pass of clip_sgd_kernel's capped grid covers


@pytest.mark.parametrize('n', [4, 7, 100003, 2 * (CS_STRIDE4 * 4) + 4 * 77 + 3])
def test_clip_sgd_is_exact_on_small_integers(ops, n):
    """No clip (sumsq = None), integer p, g, buf in [-8, 8], grad_scale = -2, lr = 2^-3, momentum = 1/2: g*gs is an even
    integer of at most 16, buf*momentum + g*gs a multiple of 1/2 of at most 24, (g*gs + momentum*buf') a multiple of 1/4 of at
    most 28, its product with lr a multiple of 1/32 below 4 and p after two steps a multiple of 1/32 below 16 -- every product
    and sum fits 24 bits, fused or not, so p and buf must equal the float64 reference BIT FOR BIT after the first step (which
    must ignore what buf holds) and after the second.  The largest size takes the capped grid through two full strides, a
    partial third and a 3-element tail.  The 64 floats behind element n of every buffer must stay as they were."""
    rng = np.random.default_rng(n % 1000)
    gs, lr, mom, pad = -2.0, 2.0 ** -3, 0.5, 64

    def ints():
        return rng.integers(-8, 9, size=n + pad).astype(np.float32)
    p0, b0, g1, g2 = ints(), ints(), ints(), ints()
    p, buf = _t(p0), _t(b0)
    ref_p, ref_b = p0[:n].astype(np.float64), b0[:n].astype(np.float64)
    for step, g in enumerate((g1, g2)):
        gd = _t(g)
        ops.clip_sgd_nesterov(p[:n], gd[:n], buf[:n], None, gs, 400.0, lr, mom, step == 0)
        ref_p, ref_b, _ = refs.nesterov_clip_step(ref_p, g[:n], ref_b, gs, 400.0, lr, mom, step == 0, clip=False)
        got_p, got_b = p.cpu().numpy(), buf.cpu().numpy()
        assert np.array_equal(got_p[:n].astype(np.float64), ref_p), (n, step)
        assert np.array_equal(got_b[:n].astype(np.float64), ref_b), (n, step)
        assert np.array_equal(_bits(got_p[n:]), _bits(p0[n:])) and np.array_equal(_bits(got_b[n:]), _bits(b0[n:]))
        assert np.array_equal(_bits(gd.cpu().numpy()), _bits(g))


@pytest.mark.parametrize('grad_scale', [1.0, 0.125, -0.125])
def test_clip_sgd_clip_numerics(ops, grad_scale):
    """n = 100003 standard-normal parameters, gradients of scale 10, 0.01 and 50: norms of about 3162, 3.2 and 15811 times
    |grad_scale| against max_norm = 400 |grad_scale|, so the first and third step clip and the second does not.  Every step is
    compared with the float64 reference applied to what the device held before it (p, buf as float32) and given the sum of
    squares the device computed: what is measured is this kernel's own rounding.

    The bounds, to first order in U, with G = |g * grad_scale| (the clip coefficient is <= 1), m = momentum, and lr, momentum
    handed to both sides as the float32 values the kernel receives:
      coefficient: the norm rounded to fp32, + 1e-6f, the division: 3 roundings; grad_scale * coef: a 4th; g * that: a 5th, so
                    |d gv| <= 5 U G
      buf' = fl(fl(buf m) + gv):  |d buf'| <= 5 U G + U m |buf| + U (m |buf| + G) = U (6 G + 2 m |buf|)      <- buf's bound
      t = fl(buf' m):             |d t|    <= m |d buf'| + U m (m |buf| + G)      = U (7 m G + 3 m^2 |buf|)
      d = fl(gv + t):             |d d|    <= |d gv| + |d t| + U (G + m (m |buf| + G)) = U ((6 + 8 m) G + 4 m^2 |buf|)
      e = fl(d lr):               |d e|    <= lr |d d| + U lr ((1 + m) G + m^2 |buf|)  = U lr ((7 + 9 m) G + 5 m^2 |buf|)
      p' = fl(p - e):             |d p'|   <= |d e| + U (|p| + |e|)               = U |p| + U lr ((8 + 10 m) G + 6 m^2 |buf|)
    and (8 + 10 m) / (1 + m) <= 9, 6 m^2 / (1 + m) <= 3 for m <= 1:   |d p'| <= U (|p| + 9 lr (1 + m) (G + |buf|)).
    The estimate 8 U (|p| + lr (1 + m) (G + |buf|)) this test was specified with counts one rounding too few on the lr term
    (9, not 8: the five roundings behind gv reach p twice, directly and through buf') and seven too many on p itself, which is
    rounded once; and it cannot hold for buf, whose error is of the order U G, not U lr G -- buf has its own line above.
    A fused multiply-add only removes roundings."""
    torch.manual_seed(0)
    n, pad = 100003, 64
    lr, mom = float(np.float32(3e-4)), float(np.float32(0.9))
    max_norm = float(np.float32(400.0 * abs(grad_scale)))
    p, buf = torch.zeros(n + pad, device=DEV), torch.zeros(n + pad, device=DEV)
    p[:n] = torch.randn(n, device=DEV)
    coefs, worst_p, worst_b = [], 0.0, 0.0
    for step, scale in enumerate((10.0, 0.01, 50.0)):
        g = torch.zeros(n + pad, device=DEV)
        g[:n] = torch.randn(n, device=DEV) * scale
        p_prev, b_prev, g_h = p[:n].cpu().numpy(), buf[:n].cpu().numpy(), g[:n].cpu().numpy()
        ss = ops.sumsq(g[:n])
        ss_h = float(ss.item())
        exact = float((g_h.astype(np.float64) ** 2).sum())
        assert abs(ss_h - exact) <= 260 * U * exact                          # (test_sumsq_of_normals_within_the_fp32_run_bound)
        ops.clip_sgd_nesterov(p[:n], g[:n], buf[:n], ss, grad_scale, max_norm, lr, mom, step == 0)
        ref_p, ref_b, coef = refs.nesterov_clip_step(p_prev, g_h, b_prev, grad_scale, max_norm, lr, mom, step == 0, sumsq=ss_h)
        coefs.append(coef)
        big_g = np.abs(g_h.astype(np.float64) * grad_scale)
        old_b = np.zeros(n) if step == 0 else np.abs(b_prev.astype(np.float64))
        tol_p = U * (np.abs(p_prev.astype(np.float64)) + 9.0 * lr * (1.0 + mom) * (big_g + old_b))
        tol_b = U * (6.0 * big_g + 2.0 * mom * old_b)
        err_p = np.abs(p[:n].cpu().numpy().astype(np.float64) - ref_p)
        err_b = np.abs(buf[:n].cpu().numpy().astype(np.float64) - ref_b)
        worst_p, worst_b = max(worst_p, float((err_p / tol_p).max())), max(worst_b, float((err_b / tol_b).max()))
        print('clip_sgd gs=%g step %d: coef %.6g, worst error / bound: p %.3f, buf %.3f'
              % (grad_scale, step, coef, float((err_p / tol_p).max()), float((err_b / tol_b).max())))
        assert np.all(err_p <= tol_p), (step, float((err_p / tol_p).max()))
        assert np.all(err_b <= tol_b), (step, float((err_b / tol_b).max()))
        assert bool((p[n:] == 0).all()) and bool((buf[n:] == 0).all())
    assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, coefs


# =========================================================================================== 3. step_stats
def _step_stats_raw(lib, costs, sumsq, words, n_err):
    """ds2_step_stats on a PRIVATE table of flag words (plain device memory of the test's own; the library's are not touched)."""
    table = torch.tensor([words.data_ptr() + 4 * i for i in range(max(n_err, 1))], dtype=torch.int64).to(DEV)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    lib.call('ds2_step_stats', costs, costs.numel(), sumsq, table, n_err, out)
    return out.cpu().numpy()


def _same_float64(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize('bsz', [1, 63, 64, 65, 200])
def test_step_stats_sums_counts_and_copies(ops, lib, bsz):
    """Costs are multiples of 1/8 below 500: their fp64 sum is exact in any order.  With infinities and NaN the sum is inf or NaN
    exactly as numpy's float64 sum (an order-independent outcome); out[3] counts +inf and -inf, not NaN; out[1] is the given
    sum of squares bit for bit, or 0 without one."""
    rng = np.random.default_rng(bsz)
    base = (rng.integers(0, 4000, size=bsz) / 8.0).astype(np.float32)
    ss = torch.tensor([1234.5678901234567], dtype=torch.float64, device=DEV)
    words = torch.zeros(1, dtype=torch.int32, device=DEV)
    clean = ops.step_stats(_t(base), ss).cpu().numpy()                       # through the wrapper: the library's own words
    assert clean[0] == base.astype(np.float64).sum() and clean[2] == 0.0 and clean[3] == 0.0
    assert clean[1:2].view(np.int64)[0] == ss.cpu().numpy().view(np.int64)[0]
    assert ops.step_stats(_t(base), None).cpu().numpy()[1] == 0.0
    cases = {'no inf': base}
    c = base.copy(); c[0] = np.inf; c[bsz - 1] = np.inf
    cases['+inf at both ends'] = c
    if bsz >= 3:
        c = c.copy(); c[bsz // 2] = -np.inf
        cases['+inf at both ends and a -inf'] = c
    c = base.copy(); c[bsz - 1] = -np.inf
    cases['-inf alone'] = c
    c = base.copy(); c[bsz - 1] = np.nan
    cases['NaN'] = c
    if bsz >= 3:
        c = c.copy(); c[0] = np.inf; c[1] = -np.inf
        cases['NaN beside +inf and -inf'] = c
    for name, c in cases.items():
        with np.errstate(invalid='ignore'):
            want_sum = c.astype(np.float64).sum()
        for given in (ss, None):
            out = _step_stats_raw(lib, _t(c), given, words, 0)
            assert _same_float64(out[0], want_sum), (name, out[0], want_sum)
            assert out[3] == float(np.isinf(c).sum()), (name, out[3])
            assert out[2] == 0.0
            if given is None:
                assert out[1] == 0.0
            else:
                assert out[1:2].view(np.int64)[0] == ss.cpu().numpy().view(np.int64)[0]
    assert np.isnan(_step_stats_raw(lib, _t(cases['NaN']), ss, words, 0)[0])


@pytest.mark.parametrize('n_err', [0, 1, 65, 130])
def test_step_stats_flag_words(lib, n_err):
    """out[2] is 1 iff one of the n_err words is non-zero: none, the first, the last (beyond lane 63 for 65 and 130 words), and
    a word whose only set bit is the top one (the words are unsigned)."""
    costs = _t(np.asarray([1.5, 2.25, 3.0], np.float32))
    words = torch.zeros(max(n_err, 1), dtype=torch.int32, device=DEV)
    assert _step_stats_raw(lib, costs, None, words, n_err)[2] == 0.0
    if n_err == 0:
        words[0] = 1                                                         # not one of the zero words it was told about
        out = _step_stats_raw(lib, costs, None, words, 0)
        assert out[2] == 0.0 and out[0] == 6.75
        return
    for pos, val in ((0, 1), (n_err - 1, 1), (n_err - 1, -2 ** 31), (n_err // 2, 7)):
        words[pos] = val
        out = _step_stats_raw(lib, costs, None, words, n_err)
        words[pos] = 0
        assert out[2] == 1.0 and out[0] == 6.75 and out[3] == 0.0, (pos, val, out)
    assert _step_stats_raw(lib, costs, None, words, n_err)[2] == 0.0


# =========================================================================================== 4. add2
def _add2_into(lib, a, b, out):
    lib.call('ds2_add2', a, b, a.numel(), out)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 2048 * 256 * 4 + 4 * 33 + 2])
def test_add2_is_ieee_addition_at_every_alignment(lib, n):
    """IEEE addition has one answer: the output must equal numpy's float32 a + b bit for bit -- on the 16-byte path (all three
    pointers aligned; the largest size passes the 2048-block cap and has a 2-float tail) and on the scalar path that a, b or out
    starting one element into a longer tensor selects.  The 8 floats either side of the output must stay as they were."""
    rng = np.random.default_rng(n % 1000)
    a_h = (rng.standard_normal(n + 1) * np.exp(4 * rng.standard_normal(n + 1))).astype(np.float32)
    b_h = (rng.standard_normal(n + 1) * np.exp(4 * rng.standard_normal(n + 1))).astype(np.float32)
    a_d, b_d = _t(a_h), _t(b_h)
    shifts = [(0, 0, 0)] if n > 1 << 20 else [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for sa, sb, so in shifts:
        out = torch.full((n + 17,), -77.0, device=DEV)
        assert (a_d.data_ptr() | b_d.data_ptr() | out.data_ptr()) % 16 == 0
        _add2_into(lib, a_d[sa:sa + n], b_d[sb:sb + n], out[8 + so:8 + so + n])
        got = out.cpu().numpy()
        want = a_h[sa:sa + n] + b_h[sb:sb + n]
        assert np.array_equal(_bits(got[8 + so:8 + so + n]), _bits(want)), (n, sa, sb, so)
        assert np.all(got[:8 + so] == -77.0) and np.all(got[8 + so + n:] == -77.0), (n, sa, sb, so)


def test_add2_wrapper(ops):
    a, b = torch.randn(1027, device=DEV), torch.randn(1027, device=DEV)
    assert np.array_equal(_bits(ops.add2(a, b).cpu().numpy()), _bits(a.cpu().numpy() + b.cpu().numpy()))


# =========================================================================================== 5. softmax_rows
@pytest.mark.parametrize('a', [1, 2, 29, 43, 63, 64, 65, 128, 129, 255, 256])
def test_softmax_rows_against_float64(ops, a):
    """Every element within rtol (16 + |x - rowmax|) U of the float64 softmax, every row sum within 4 U of 1.

    Where the roundings are (lane l holds columns l, l + 64, l + 128, l + 192; the denominator is accumulated in fp64):
      x - max is rounded to |x - max| U, which the exponential turns into a RELATIVE error of |x - max| U         (the gap term)
      expf: 1 ulp (the documented bound of the device library) <= 2 U, on the numerator                            2
      and on every term of the denominator, so on their sum                                                        2
      the denominator also carries the gap term of ITS terms: sum_j p_j |x_j - max| U = (H(p) - ln Z) U <= ln(A) U  5.5
      1 / sum rounded to float32, and the product with it                                                          2
    which is 11.5: 16 holds with room for second-order terms.  (With the fp32 tree of 9 additions the kernel had before, the
    worst case was 20.5.)
    Row sums (of the float32 outputs, taken in float64): the expf errors are common to numerator and denominator and cancel,
    what is left is the rounding of 1 / sum (U) and the weighted mean of the products' roundings (U): <= 2 U, asserted at the
    4 U specified.  The fp32 tree missed that: 5.80 U at A = 129 (3.3 - 3.9 U at most other widths), 1.22 U at most now.
    Columns holding -inf come out exactly 0."""
    rng = np.random.default_rng(a)
    worst, worst_sum, failures = 0.0, 0.0, []
    for rows in (1, 5, 301):
        base = (4 * rng.standard_normal((rows, a))).astype(np.float32)
        # max - min = 80 exactly: the smallest probability, e^-80 / sum >= 1.8e-35 / 256, is still a NORMAL float32
        spread = rng.uniform(-40.0, 40.0, size=(rows, a)).astype(np.float32)
        holes = base.copy()
        if a > 1:
            cmax = rng.integers(0, a, size=rows)
            spread[np.arange(rows), cmax] = 40.0
            spread[np.arange(rows), (cmax + 1 + rng.integers(0, a - 1, size=rows)) % a] = -40.0
            holes[rng.random((rows, a)) < 0.3] = -np.inf
            holes[np.arange(rows), rng.integers(0, a, size=rows)] = 1.0     # (never a whole row)
        for name, x in (('normal', base), ('shifted', base + np.float32(1e4)), ('spread', spread), ('-inf', holes)):
            want = refs.softmax64(x)
            got = ops.softmax_rows(_t(x), rows, a).cpu().numpy().astype(np.float64)
            gap = np.abs(x.astype(np.float64) - x.astype(np.float64).max(axis=1, keepdims=True))
            finite = np.isfinite(x)
            assert np.all(got[~finite] == 0.0), (name, rows)
            if name == 'spread' and a > 1:
                assert float(gap.max()) == 80.0
            ratio = float((np.abs(got - want)[finite] / (((16.0 + gap[finite]) * U) * want[finite])).max())
            sums = float(np.abs(got.sum(axis=1) - 1.0).max())
            worst, worst_sum = max(worst, ratio), max(worst_sum, sums)
            if ratio > 1.0 or sums > 4 * U:
                failures.append((name, rows, ratio, sums / U))
    print('softmax A=%d: worst error / bound %.3f, worst |row sum - 1| %.2f U' % (a, worst, worst_sum / U))
    assert not failures, failures


@pytest.mark.parametrize('a', [0, 257])
def test_softmax_rows_rejects_what_a_wave_cannot_hold(ops, lib, a):
    x = torch.zeros(4 * 257, device=DEV)
    y = torch.full((4 * 257,), 5.0, device=DEV)
    with pytest.raises(lib.Ds2Error) as ei:
        lib.call('ds2_softmax_rows', x, 4, a, y)
    assert ei.value.code == lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())                                            # nothing was launched


# =========================================================================================== 6. argmax_rows
@pytest.mark.parametrize('a', [1, 29, 64, 65, 127, 128, 200])
def test_argmax_rows_has_torch_max_order(ops, a):
    """Lane l scans columns l, l + 64, ...; the lanes' candidates are then merged.  torch.max's order in both: the largest value,
    NaN larger than anything, the lowest index among equals."""
    rng = np.random.default_rng(a)
    rows = [rng.standard_normal(a) for _ in range(40)]

    def row(**cols):
        r = rng.standard_normal(a)
        for k, v in cols.items():
            if int(k[1:]) >= a:
                return
            r[int(k[1:])] = v
        rows.append(r)
    row(c3=10.0, c67=10.0)                       # a tie inside lane 3's own columns
    row(c70=10.0, c134=10.0, c198=10.0)
    row(c3=10.0, c9=10.0)                        # between lanes
    row(c5=10.0, c67=10.0)                       # the LOWER lane holds the higher index
    row(c63=10.0, c64=10.0)
    row(c0=10.0, c17=10.0, c28=10.0)             # three ways, with column 0
    row(c0=10.0, c64=10.0, c126=10.0)
    row(c0=10.0)
    row(**{'c%d' % (a - 1): 10.0})
    rows.append(np.full(a, -np.inf))             # -> 0
    rows.append(np.full(a, np.inf))
    row(c7=np.inf)
    row(c7=np.inf, c5=np.inf)
    row(c66=np.inf, c2=np.inf)
    row(c0=-np.inf, c1=-np.inf)
    rows.append(np.full(a, np.nan))              # -> 0
    row(c12=np.nan, c3=50.0)                     # NaN beside larger finite values
    row(c76=np.nan, c12=50.0)                    # in a lane's second column
    row(c12=np.nan, c3=np.inf)
    row(c20=np.nan, c4=np.nan)                   # two NaN in different lanes: the first
    row(c4=np.nan, c68=np.nan)                   # ... in one lane
    row(c70=np.nan, c9=np.nan)                   # ... the lower lane holds the later one
    row(**{'c%d' % (a - 1): np.nan})
    r = np.full(a, np.nan); r[0] = 1.0           # all NaN but column 0
    rows.append(r)
    x = np.stack(rows).astype(np.float32)
    want = refs.argmax_nan_first(x)
    got = ops.argmax_rows(_t(x), x.shape[0], a).cpu().numpy()
    assert got.dtype == np.int32 and np.all((got >= 0) & (got < a)), got
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]]


# =========================================================================================== 7. greedy_collapse
@pytest.mark.parametrize('blank', [0, 28, 5])
@pytest.mark.parametrize('t', [1, 63, 64, 65, 128, 150])
def test_greedy_collapse_against_the_plain_loop(ops, t, blank):
    """One wave walks a row in chunks of 64 frames.  Rows: a repeat run over frames 60-70 (across the chunk edge), a label change
    exactly at frame 64, two labels alternating without a blank (every frame kept: lens == size), an all-blank row, a row whose
    frame 0 is a label; sizes T, T + 7 (clamped to T), 1, 0 and -3 (nothing)."""
    rng = np.random.default_rng(100 * t + blank)
    labels = [c for c in range(29) if c != blank]
    la, lb = labels[3], labels[11]

    def noisy():
        r = rng.choice(labels, size=t)
        r[rng.random(t) < 0.5] = blank
        return r
    run = noisy(); run[0] = la; run[60:71] = lb
    change = noisy(); change[56:64] = la; change[64:72] = lb
    alt = np.where(np.arange(t) % 2 == 0, la, lb)
    rows = [(run, t), (run, t + 7), (change, t), (change, t + 7), (alt, t), (alt, t + 7), (alt, max(t - 1, 1)),
            (np.full(t, blank), t), (run, 1), (noisy(), 0), (noisy(), t // 2 + 1), (noisy(), -3)]
    best = np.stack([r for r, _ in rows]).astype(np.int32)
    sizes = np.asarray([s for _, s in rows], np.int32)
    ids, offs, lens = [v.cpu().numpy() for v in ops.greedy_collapse(_t(best), _t(sizes), blank)]
    for b, (r, s) in enumerate(rows):
        want_ids, want_offs = refs.collapse(r, s, blank)
        k = len(want_ids)
        assert lens[b] == k, (b, int(lens[b]), k)
        assert list(ids[b, :k]) == want_ids and list(offs[b, :k]) == want_offs, b
        assert np.all(ids[b, k:] == 0) and np.all(offs[b, k:] == 0), b
    assert lens[4] == t and lens[5] == t and lens[7] == 0 and lens[8] == 1 and lens[9] == 0 and lens[11] == 0


# =========================================================================================== 8. transposes
def _group_raw(lib, tensors, count, batch, rows, cols, out):
    """ds2_transpose2d_group without the wrapper's own assertions."""
    ptrs = (ctypes.c_void_p * len(tensors))(*[x.data_ptr() for x in tensors])
    rc = lib.load().ds2_transpose2d_group(count, ctypes.cast(ptrs, ctypes.c_void_p), batch, rows, cols, out.data_ptr(),
                                          lib.stream_ptr())
    if rc != 0:
        raise lib.Ds2Error(rc, lib.load().ds2_last_error().decode())


def test_transposes_at_tile_edges(ops, lib):
    """32 x 32 tiles: a single element, one row, one column, exactly one tile, below / above a tile in both directions, whole
    tiles only.  A transpose moves bits: exact."""
    rng = np.random.default_rng(8)
    for rows, cols in ((1, 1), (1, 33), (33, 1), (32, 32), (31, 65), (64, 96)):
        x = rng.standard_normal((rows, cols)).astype(np.float32)
        out = torch.full((rows * cols + 16,), -77.0, device=DEV)
        ops.transpose2d(_t(x), rows, cols, out=out[:rows * cols])
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got[:rows * cols].reshape(cols, rows)), _bits(x.T)), (rows, cols)
        assert np.all(got[rows * cols:] == -77.0)
    for t, f in ((1, 161), (31, 161), (32, 160)):
        x = rng.standard_normal((3, t, f)).astype(np.float32)
        assert np.array_equal(_bits(ops.transpose_btf(_t(x)).cpu().numpy()), _bits(x.transpose(0, 2, 1))), (t, f)
    batch, rows, cols = 2, 33, 31
    for cnt in (1, 8):
        xs = [_t(rng.standard_normal((batch, rows, cols)).astype(np.float32)) for _ in range(cnt)]
        out = torch.full((cnt * batch * rows * cols + 16,), -77.0, device=DEV)
        ops.transpose2d_group(xs, batch, rows, cols, out[:cnt * batch * rows * cols])
        got = out[:cnt * batch * rows * cols].view(cnt, batch, cols, rows)
        for i, x in enumerate(xs):
            for b in range(batch):
                assert torch.equal(got[i, b], ops.transpose2d(x[b].contiguous(), rows, cols))
                assert np.array_equal(_bits(got[i, b].cpu().numpy()), _bits(x[b].cpu().numpy().T))
        assert bool((out[cnt * batch * rows * cols:] == -77.0).all())


def test_transpose_group_rejects_nine_inputs_and_a_grid_of_65536(lib):
    xs = [torch.zeros(4, device=DEV) for _ in range(9)]
    out = torch.full((64,), 5.0, device=DEV)
    for count, batch in ((9, 1), (8, 8192), (0, 1)):
        with pytest.raises(lib.Ds2Error) as ei:
            _group_raw(lib, xs, count, batch, 2, 2, out)
        assert ei.value.code == lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    _group_raw(lib, xs, 8, 1, 2, 2, out)                                     # (the same call within the limits runs)
    torch.cuda.synchronize()
    assert bool((out[:32] == 0.0).all()) and bool((out[32:] == 5.0).all())


# =========================================================================================== 9. spectrogram
def _noise(n, seed, scale=0.1):
    return np.clip(scale * np.random.default_rng(seed).standard_normal(n), -1, 1).astype(np.float32)


def _spect(ops, wavs, t_max, normalize=True, host_offsets=False):
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(w) for w in wavs])]).astype(np.int64))
    return ops.spectrogram(_t(np.concatenate(wavs)), offs if host_offsets else offs.to(DEV), t_max, normalize=normalize)


EDGE_LENS = (161, 2399, 2400, 2401, 40960, 41119, 128320, 240000)           # 2, 15, 16, 16, 257, 257, 803, 1501 frames


@pytest.fixture(scope='module')
def edge_clips():
    return [_noise(n, 50 + i) for i, n in enumerate(EDGE_LENS)]


@pytest.mark.parametrize('t_max', [1501, 17])
def test_spectrogram_frame_and_grid_edges(ops, edge_clips, t_max):
    """0.1 x white noise, atol 2e-4 (the bound of tests/test_kernels_gpu.py::test_spectrogram_matches_oracle for this input).
    Clips of 2 frames up to 1501: the normalise kernel's loop over the per-frame partials takes 1, 2, 4 and 6 trips (256 frames
    per trip), its grid reaches the 64-block cap (t_max >= 802), the shortest clip reflects at both ends of every frame.
    t_max = 17 cuts the longer clips: their statistics are those of their first 17 frames."""
    want = refs.batch_log_spectrogram64(edge_clips, t_max)
    got = _spect(ops, edge_clips, t_max).cpu().numpy()
    assert got.shape == want.shape == (len(EDGE_LENS), t_max, 161)
    for b, n in enumerate(EDGE_LENS):
        nfr = min(1 + n // 160, t_max)
        err = float(np.abs(got[b, :nfr] - want[b, :nfr]).max())
        print('spectrogram t_max=%d clip of %d samples: max error %.3g' % (t_max, n, err))
        assert err <= 2e-4, (n, err)
        assert np.all(got[b, nfr:] == 0.0), n
    raw = _spect(ops, edge_clips, t_max, normalize=False).cpu().numpy()
    want_raw = refs.batch_log_spectrogram64(edge_clips, t_max, normalize=False)
    np.testing.assert_allclose(raw, want_raw, rtol=0, atol=2e-5)             # (that test's bound for the raw log-magnitudes)
    assert torch.equal(_spect(ops, edge_clips, t_max, host_offsets=True), _t(got))


@pytest.mark.parametrize('frames,t_max', [(16, 16), (16, 17), (17, 16), (17, 17)])
def test_spectrogram_single_clip_at_the_block_edge(ops, frames, t_max):
    """A block of the transform kernel covers 16 frames: t_max = 16 is one block, 17 two; a clip of 16 / 17 frames fills it, is
    padded by one zero frame, or is cut by one."""
    clip = _noise(160 * (frames - 1) + 7, frames)
    want = refs.batch_log_spectrogram64([clip], t_max)
    got = _spect(ops, [clip], t_max).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-4)
    assert torch.equal(_spect(ops, [clip], t_max, host_offsets=True), _t(got))


def _content_clip(name):
    n = 37923
    t = np.arange(n) / 16000.0
    noise = _noise(n, 5)
    return {'int16 scale': (noise * 32768).astype(np.float32),
            'near silence': (noise * np.float32(1e-4)).astype(np.float32),
            'dc': (noise + np.float32(0.5)).astype(np.float32),
            'sine 1000 Hz': (0.3 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32),      # bin 20 exactly
            'sine 1012.5 Hz': (0.3 * np.sin(2 * np.pi * 1012.5 * t)).astype(np.float32),    # between bins 20 and 21
            }[name]


# The float32 CPU run of the oracle's formula (small_refs.log_spectrogram32) against the float64 oracle, measured where this
# test was written -- max |error| raw / normalised:
#   int16 scale     4.9e-05 / 7.7e-05   (bins of magnitude ~100 beside a frame norm of ~3e4: the FFT's error is relative to the norm)
#   near silence    7.9e-11 / 1.8e-06   (log1p(m) ~ m ~ 1e-4; the normalisation divides by a std of 5e-5)
#   dc              5.0e-06 / 1.1e-05
#   sine 1000 Hz    9.0e-07 / 2.4e-06
#   sine 1012.5 Hz  1.1e-06 / 2.9e-06
# (the figure depends a little on the FFT library behind torch.stft: 5.0e-05 / 7.8e-05 and 7.4e-06 / 1.6e-05 for the first and the
# third on another machine, where the kernel itself measured 4.0e-05 / 6.0e-05 and 6.0e-06 / 1.3e-05 -- in every case at or
# below the float32 CPU run.)
# The kernel is a different, equally sound float32 factorisation (5 x 64, sincospi twiddles): it gets 4x the figure of the
# input at hand, computed again by the test, and never less than the 2e-5 raw / 2e-4 normalised of the white-noise test.
@pytest.mark.parametrize('name', ['int16 scale', 'near silence', 'dc', 'sine 1000 Hz', 'sine 1012.5 Hz'])
def test_spectrogram_amplitude_and_content(ops, name):
    clip = _content_clip(name)
    for normalize, floor in ((False, 2e-5), (True, 2e-4)):
        cpu32 = refs.fp32_frontend_error(clip, normalize)
        tol = max(4.0 * cpu32, floor)
        want = refs.log_spectrogram64(clip, normalize)
        got = _spect(ops, [clip], want.shape[0], normalize=normalize).cpu().numpy()[0].astype(np.float64)
        err = float(np.abs(got - want).max())
        print('spectrogram %s normalize=%d: kernel %.3g, float32 CPU run %.3g, bound %.3g' % (name, normalize, err, cpu32, tol))
        assert err <= tol, (name, normalize, err, cpu32)


def test_spectrogram_silent_clip_beside_a_normal_one(ops):
    """An all-zero clip: log1p(0) = 0 in every bin, mean 0, std 0, and (0 - 0) / (0 + eps) is exactly 0, as in the oracle."""
    clips = [np.zeros(20000, np.float32), _noise(16000, 6)]
    want = refs.batch_log_spectrogram64(clips, 126)
    assert np.all(want[0] == 0.0)
    got = _spect(ops, clips, 126).cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(got[0] == 0.0)
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=2e-4)
    raw = _spect(ops, clips, 126, normalize=False).cpu().numpy()
    assert np.all(raw[0] == 0.0)
