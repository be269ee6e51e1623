"""Every kernel form of the six BatchNorm entry points at its dispatch edges, against float64 under derived bounds.

The cases, the references and the bounds are tests/bn_cases.py (checked on the CPU by test_bn_cases_cpu.py).  Every operand of
every case sits in a flat buffer of its own, at a chosen offset off 16-byte alignment, surrounded by NaN (inputs, the
workspace) or a sentinel bit pattern (outputs): nothing outside an operand may reach a result, nothing outside an output may
change, and a partial sum that no block wrote shows as NaN.  apply and backward run under a GIVEN mean_invstd, so each entry
point is held to its own bound.  The tests assert results only, never which kernel ran.  `-s` prints, per case and result,
how far into its bound the error reaches (error / bound; for invstd the position inside its interval).  Needs an MI355X.

Measured on an MI355X, the largest error / bound over the whole table (112 tests, 4 s):
  ds2_bn2d_stats        mean 0.11, invstd 0.12, running_mean 0.34, running_var 0.22, eval invstd 0.85 (one rounding: <= 1 by IEEE)
  ds2_bn2d_apply_htanh  y 0.11, (T, B, C D) layout 0.21
  ds2_bn2d_htanh_bwd    dx 0.31, dgamma 0.23, dbeta 0.12
  ds2_bn1d_stats        mean 0.44, invstd 0.70, running_mean 0.54, running_var 0.49, eval invstd 0.87
  ds2_bn1d_apply        y 0.59
  ds2_bn1d_bwd          dx 0.34, dgamma 0.92, dbeta 0.32
The figures near 1 belong to channels of one to three rows, where a thread adds a single term and the bound is three roundings
wide (dgamma at rows = 1: 0.92); at 257 rows and more no sum passes 0.35."""
import numpy as np
import pytest
import torch

from tests import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    from ds2hip import lib as _lib
    return _lib


class Dev:
    """a Flat view on the device"""

    def __init__(self, flat):
        self.flat = flat
        self.host = torch.from_numpy(flat.buf)
        self.t = self.host.to(DEV, copy=True)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * flat.start

    def reset(self):
        self.t.copy_(self.host)

    def unchanged(self):
        return torch.equal(self.t.view(torch.int32), self.host.to(DEV).view(torch.int32))

    def result(self, what):
        """the view's floats after a launch: finite, and every float around them what it was"""
        buf = self.t.cpu().numpy()
        assert self.flat.outside_intact(buf), '%s: written outside its view' % what
        out = self.flat.view(buf).copy()
        assert np.isfinite(out).all(), '%s: %d non-finite values' % (what, (~np.isfinite(out)).sum())
        return out


class Operands:
    """the device buffers of one case"""

    def __init__(self, case, lib):
        self.case, self.lib, self.off = case, lib, case.offs()
        self.inputs = []
        c = case.channels
        assert lib.query('ds2_bn_ws_bytes', c) == 4 * bc.ws_floats(c)
        ws = bc.Flat(bc.ws_floats(c), 0, 'sentinel')
        ws.view().view(np.uint32)[:] = bc.NAN_BITS
        self.ws = Dev(ws)

    def inp(self, name, arr):
        d = Dev(bc.Flat(arr.size, self.off.get(name, 0), 'nan').put(arr))
        self.inputs.append((name, d))
        return d

    def out(self, name, n, init=None):
        f = bc.Flat(n, self.off.get(name, 0), 'sentinel')
        if init is not None:
            f.put(init)
        return Dev(f)

    def call(self, name, *args):
        self.ws.reset()
        self.lib.call(name, *args)
        torch.cuda.synchronize()
        buf = self.ws.t.cpu().numpy()
        assert self.ws.flat.outside_intact(buf), '%s wrote behind its workspace' % name
        return self.ws.flat.view(buf)

    def inputs_unchanged(self):
        for name, d in self.inputs:
            assert d.unchanged(), 'input %s changed' % name


def _report(case, entry, ratios):
    for key, r in ratios.items():
        print('RATIO %s %s %s %.4f' % (entry, case.name, key, r))
        assert np.isfinite(r) and r <= 1.0, (case.name, entry, key, r)


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _check_stats(ops_, case, p, name, head, ex):
    """training statistics (with or without running buffers), then eval from the buffers the training step left"""
    c = case.channels
    mi = ops_.out('mi', 2 * c)
    rm = ops_.out('rm', c, p.rm0) if case.running else None
    rv = ops_.out('rv', c, p.rv0) if case.running else None
    ws = ops_.call(name, *head, bc.EPS, bc.MOMENTUM, 0, rm and rm.ptr, rv and rv.ptr, mi.ptr, ops_.ws.ptr)
    part = ws[:c * bc.NPART * 4].view(np.float64)
    assert np.isfinite(part).all(), 'a partial sum that no block wrote'
    got = mi.result('mean_invstd')
    _report(case, name, bc.stats_ratios(p, got))
    if case.kind == 'count':
        assert np.array_equal(got[:c], ex.mean), 'mean is not float32(S / count)'
        assert _ulps(got[c:], ex.invstd) <= 1
    if not case.running:
        return
    rm1, rv1 = rm.result('running_mean'), rv.result('running_var')
    _report(case, name, bc.running_ratios(p, rm1, rv1))
    # eval: mean_invstd from the buffers, which keep every bit; the workspace is not touched
    mi_e = ops_.out('mi', 2 * c)
    before = (rm.t.clone(), rv.t.clone())
    ws = ops_.call(name, *head, bc.EPS, bc.MOMENTUM, 1, rm.ptr, rv.ptr, mi_e.ptr, ops_.ws.ptr)
    assert (ws.view(np.uint32) == bc.NAN_BITS).all()
    assert torch.equal(before[0].view(torch.int32), rm.t.view(torch.int32))
    assert torch.equal(before[1].view(torch.int32), rv.t.view(torch.int32))
    got = mi_e.result('eval mean_invstd')
    mean_e, inv_e, b_inv = bc.eval_ref(rm1, rv1)
    assert np.array_equal(got[:c].view(np.uint32), mean_e.view(np.uint32))
    _report(case, name + '(eval)', {'invstd': float((np.abs(got[c:].astype(np.float64) - inv_e) / b_inv).max())})


def _check_bwd(ops_, case, p, name, args_of, ex):
    c, n = case.channels, case.count * case.channels
    dx, dgamma, dbeta = ops_.out('dx', n), ops_.out('dgamma', c), ops_.out('dbeta', c)
    ws = ops_.call(name, *args_of(dx, dgamma, dbeta), ops_.ws.ptr)
    assert np.isfinite(ws[:c * bc.NPART * 4].view(np.float64)).all(), 'a partial sum that no block wrote'
    assert np.isfinite(ws[c * bc.NPART * 4:]).all()
    got = (dx.result('dx').reshape(p.shape), dgamma.result('dgamma'), dbeta.result('dbeta'))
    _report(case, name, bc.bwd_ratios(p, *got))
    if case.kind == 'count':
        assert np.array_equal(got[1], ex.dgamma) and np.array_equal(got[2], ex.dbeta)
    if case.kind == 'edge':
        assert p.bw.keep.all()                  # no exclusions: y = x exactly, the mask is decided by x alone


@pytest.mark.parametrize('case', bc.conv_cases(), ids=lambda c: c.name)
def test_bn2d_case(lib, case):
    """ds2_bn2d_stats (training, eval), ds2_bn2d_apply_htanh (both layouts), ds2_bn2d_htanh_bwd on one set of operands"""
    p = bc.make(case)
    ex = bc.exact_expectations(p)
    o = Operands(case, lib)
    b, c, d, t = case.B, case.C, case.D, case.T
    x, dy = o.inp('x', p.x), o.inp('dy', p.dy)
    gamma, beta, mi = o.inp('gamma', p.gamma), o.inp('beta', p.beta), o.inp('mi', p.mi)
    _check_stats(o, case, p, 'ds2_bn2d_stats', (x.ptr, b, c, case.inner), ex)

    y = o.out('y', p.x.size)
    o.call('ds2_bn2d_apply_htanh', x.ptr, mi.ptr, gamma.ptr, beta.ptr, b, c, d, t, 0, y.ptr)
    got = y.result('y').reshape(p.shape)
    _report(case, 'ds2_bn2d_apply_htanh', bc.apply_ratios(p, got))
    if case.kind in ('count', 'edge'):
        assert np.array_equal(got.view(np.uint32), ex.y.view(np.uint32)), 'y is not bit-exact'
    if case.tbf:
        yt = o.out('y', p.x.size)
        o.call('ds2_bn2d_apply_htanh', x.ptr, mi.ptr, gamma.ptr, beta.ptr, b, c, d, t, 1, yt.ptr)
        got_t = yt.result('y (T, B, C D)').reshape(t, b, c * d)
        back = np.ascontiguousarray(got_t.transpose(1, 2, 0)).reshape(p.shape)
        _report(case, 'ds2_bn2d_apply_htanh(tbf)', bc.apply_ratios(p, back))
        if case.kind in ('count', 'edge'):
            assert np.array_equal(got_t.view(np.uint32), case.tbf_of(ex.y).view(np.uint32))

    _check_bwd(o, case, p, 'ds2_bn2d_htanh_bwd',
               lambda dx, dg, db: (x.ptr, dy.ptr, mi.ptr, gamma.ptr, beta.ptr, b, c, d, t, dx.ptr, dg.ptr, db.ptr), ex)
    o.inputs_unchanged()


def _seq_run(lib, case, p, ex=None):
    """the three sequence entry points on one set of operands"""
    o = Operands(case, lib)
    rows, f = case.rows, case.F
    xa, dy = o.inp('xa', p.x), o.inp('dy', p.dy)
    xb = o.inp('xb', p.xb) if p.xb is not None else None
    gamma, beta, mi = o.inp('gamma', p.gamma), o.inp('beta', p.beta), o.inp('mi', p.mi)
    xbp = xb and xb.ptr
    _check_stats(o, case, p, 'ds2_bn1d_stats', (xa.ptr, xbp, rows, f), ex)
    y = o.out('y', p.x.size)
    o.call('ds2_bn1d_apply', xa.ptr, xbp, mi.ptr, gamma.ptr, beta.ptr, rows, f, y.ptr)
    got = y.result('y').reshape(p.shape)
    _report(case, 'ds2_bn1d_apply', bc.apply_ratios(p, got))
    if case.kind == 'count':
        assert np.array_equal(got, ex.y), 'y is not exact'
    _check_bwd(o, case, p, 'ds2_bn1d_bwd',
               lambda dx, dg, db: (xa.ptr, xbp, dy.ptr, mi.ptr, gamma.ptr, rows, f, dx.ptr, dg.ptr, db.ptr), ex)
    o.inputs_unchanged()


@pytest.mark.parametrize('case', bc.seq_cases(), ids=lambda c: c.name)
def test_bn1d_case(lib, case):
    """ds2_bn1d_stats (training, eval), ds2_bn1d_apply, ds2_bn1d_bwd on one set of operands"""
    p = bc.make(case)
    _seq_run(lib, case, p, bc.exact_expectations(p))


# --------------------------------------------------------------------------------------------- 16-byte against scalar
def _seq_raw(lib, case, p):
    """mean_invstd, y, dx, dgamma, dbeta of the sequence entry points as device tensors, no checks"""
    o = Operands(case, lib)
    rows, f = case.rows, case.F
    xa, xb, dy = o.inp('xa', p.x), o.inp('xb', p.xb), o.inp('dy', p.dy)
    gamma, beta, mi = o.inp('gamma', p.gamma), o.inp('beta', p.beta), o.inp('mi', p.mi)
    outs = {'mean_invstd': o.out('mi', 2 * f), 'y': o.out('y', p.x.size), 'dx': o.out('dx', p.x.size),
            'dgamma': o.out('dgamma', f), 'dbeta': o.out('dbeta', f)}
    o.call('ds2_bn1d_stats', xa.ptr, xb.ptr, rows, f, bc.EPS, bc.MOMENTUM, 0, None, None, outs['mean_invstd'].ptr, o.ws.ptr)
    o.call('ds2_bn1d_apply', xa.ptr, xb.ptr, mi.ptr, gamma.ptr, beta.ptr, rows, f, outs['y'].ptr)
    o.call('ds2_bn1d_bwd', xa.ptr, xb.ptr, dy.ptr, mi.ptr, gamma.ptr, rows, f, outs['dx'].ptr, outs['dgamma'].ptr,
           outs['dbeta'].ptr, o.ws.ptr)
    return {k: d.result(k) for k, d in outs.items()}


@pytest.mark.parametrize('rows,f', bc.VEC_SCALAR_SHAPES)
def test_bn1d_16_byte_and_scalar_kernels_on_the_same_data(lib, rows, f):
    """The same data once aligned (16-byte kernels) and once with every big tensor one float off (scalar kernels).
    csrc/bn.hip used to say that the two give identical bits because they sum each column's rows in the same order.  They do
    not on an MI355X: the compiler fuses the last product of a term into the accumulation in the 16-byte forms (v_pk_fma_f32)
    and not in the scalar ones (v_mul_f32, then one v_pk_add_f32 over both accumulators).  Measured (the counts are printed):
    y and dbeta agree in every bit; up to 3 % of mean_invstd (none while a thread adds one term), 5 to 36 % of dx and up to
    64 % of dgamma differ in their last bits.  The comment was corrected; the assertion is the float64 bound, the same one for
    both forms."""
    aligned = bc.Seq('pair', rows, f)
    shifted = bc.Seq('pair', rows, f, off=tuple((nm, 1) for nm in ('xa', 'xb', 'dy', 'y', 'dx')))
    assert set(aligned.forms().values()) == {'vec'} and set(shifted.forms().values()) == {'scalar'}
    p = bc.make(aligned)
    res = {}
    for case in (aligned, shifted):
        r = res[case] = _seq_raw(lib, case, p)
        _report(case, 'ds2_bn1d_stats', bc.stats_ratios(p, r['mean_invstd']))
        _report(case, 'ds2_bn1d_apply', bc.apply_ratios(p, r['y'].reshape(p.shape)))
        _report(case, 'ds2_bn1d_bwd', bc.bwd_ratios(p, r['dx'].reshape(p.shape), r['dgamma'], r['dbeta']))
    for key in res[aligned]:
        differ = res[aligned][key].view(np.uint32) != res[shifted][key].view(np.uint32)
        print('BITS %dx%d %s: %d of %d differ between the two forms' % (rows, f, key, differ.sum(), differ.size))


# --------------------------------------------------------------------------------------------- through ds2hip.ops, chained
def test_bn2d_chain_through_ops(lib):
    """statistics -> apply (both layouts) -> backward the way codes/model.py calls them: apply and backward read the
    statistics kernel's own mean_invstd, and are held to float64 under exactly those numbers"""
    from ds2hip import ops
    case = bc.Conv('ops', 3, 32, 21, 33, tbf=True)
    p0 = bc.make(case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    x, dy = dev(p0.x.reshape(3, 32, 21, 33)), dev(p0.dy.reshape(3, 32, 21, 33))
    gamma, beta, rm, rv = dev(p0.gamma), dev(p0.beta), dev(p0.rm0), dev(p0.rv0)
    mi = ops.bn2d_stats(x, rm, rv, training=True)
    _report(case, 'ops.bn2d_stats', bc.stats_ratios(p0, mi.cpu().numpy()))
    _report(case, 'ops.bn2d_stats', bc.running_ratios(p0, rm.cpu().numpy(), rv.cpu().numpy()))
    p = bc.make(case, mi=mi.cpu().numpy())
    y = ops.bn2d_apply_htanh(x, mi, gamma, beta, layout_tbf=False)
    _report(case, 'ops.bn2d_apply_htanh', bc.apply_ratios(p, y.cpu().numpy().reshape(p.shape)))
    yt = ops.bn2d_apply_htanh(x, mi, gamma, beta, layout_tbf=True)
    assert yt.shape == (33, 3, 32 * 21)
    back = yt.permute(1, 2, 0).contiguous().cpu().numpy().reshape(p.shape)
    _report(case, 'ops.bn2d_apply_htanh(tbf)', bc.apply_ratios(p, back))
    dg, db = torch.empty(32, device=DEV), torch.empty(32, device=DEV)
    dx = ops.bn2d_htanh_bwd(x, dy, mi, gamma, beta, dg, db)
    _report(case, 'ops.bn2d_htanh_bwd', bc.bwd_ratios(p, dx.cpu().numpy().reshape(p.shape), dg.cpu().numpy(), db.cpu().numpy()))
    mi_e = ops.bn2d_stats(x, rm, rv, training=False)
    assert torch.equal(mi_e[:32], rm)


def test_bn1d_chain_through_ops(lib):
    from ds2hip import ops
    case = bc.Seq('ops', 530, 800)
    p0 = bc.make(case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    xa, xb, dy = dev(p0.x), dev(p0.xb), dev(p0.dy)
    gamma, beta, rm, rv = dev(p0.gamma), dev(p0.beta), dev(p0.rm0), dev(p0.rv0)
    mi = ops.bn1d_stats(xa, xb, 530, 800, rm, rv, training=True)
    _report(case, 'ops.bn1d_stats', bc.stats_ratios(p0, mi.cpu().numpy()))
    _report(case, 'ops.bn1d_stats', bc.running_ratios(p0, rm.cpu().numpy(), rv.cpu().numpy()))
    p = bc.make(case, mi=mi.cpu().numpy())
    y = ops.bn1d_apply(xa, xb, mi, gamma, beta, 530, 800)
    _report(case, 'ops.bn1d_apply', bc.apply_ratios(p, y.cpu().numpy()))
    dg, db = torch.empty(800, device=DEV), torch.empty(800, device=DEV)
    dx = ops.bn1d_bwd(xa, xb, dy, mi, gamma, 530, 800, dg, db)
    _report(case, 'ops.bn1d_bwd', bc.bwd_ratios(p, dx.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()))
    mi_e = ops.bn1d_stats(xa, xb, 530, 800, rm, rv, training=False)
    assert torch.equal(mi_e[:800], rm)
