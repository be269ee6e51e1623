"""Every kernel form of the three segmented BatchNorm entry points at its dispatch edges, against float64 under derived bounds.

The cases, the layouts, the per-task references and the bounds are tests/bn_seg_cases.py (checked on the CPU by
test_bn_seg_cases_cpu.py); the bounds are those of tests/bn_cases.py on each task's own rows.  Every operand of every case,
each task's gamma, beta, running buffers, dgamma and dbeta among them, sits in a flat buffer of its own at a chosen offset off
16-byte alignment, surrounded by NaN (inputs, the workspace) or a sentinel bit pattern (outputs); the workspace is exactly
G * ds2_bn_ws_bytes(F) long.  Nothing outside an operand may reach a result, nothing outside an output may change, and a
partial sum that no block wrote shows as NaN.  apply and backward run under a GIVEN mean_invstd, so each entry point is held
to its own bound.  The tests assert results only, never which kernel ran.  `-s` prints, per case and result, how far into
its bound the error reaches (error / bound over all tasks; for invstd the position inside its interval).  Needs an MI355X.

Measured on an MI355X, the largest error / bound over the whole table (81 tests, 3.4 s):
  ds2_bn1d_seg_stats   mean 0.42, invstd 0.70, running_mean 0.90, running_var 0.66, eval invstd 0.99 (one rounding: <= 1 by IEEE)
  ds2_bn1d_seg_apply   y 0.50
  ds2_bn1d_seg_bwd     dx 0.37, dgamma 0.98, dbeta 0.32
  through ds2hip.ops   mean 0.32, invstd 0.17, running_mean 0.88, running_var 0.17, y 0.34, dx 0.32, dgamma 0.49, dbeta 0.22
The figures near 1 belong to tasks of one to three rows, where a thread adds a single term and the bound is three roundings
wide (dgamma 0.98 and invstd 0.70 at T = 1 with one, two and three columns; running_mean 0.90 at three to twelve rows).  Every
integer case is exact, and every task equals its G = 1 launch bit for bit.  The two forms on the same data: y, dbeta and the
running mean agree in every bit; mean_invstd and the running variance differ by at most 1 ulp in about 1 % of the channels,
dgamma in a quarter of them and dx in 6 % of its elements at (257, [0, 1, 3], 260); at (51, [0, 5, 6], 36), where a thread
adds a single term, only dx differs.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bn_cases as bc
from tests import bn_seg_cases as sc
from tests.test_bn_edges_gpu import DEV, Dev, Operands, _ulps

pytestmark = pytest.mark.gpu

CASES = sc.seg_cases()
BY = {c.name: c for c in CASES}


@pytest.fixture(scope='module')
def lib():
    from ds2hip import lib as _lib
    return _lib


class SegOperands(Operands):
    """the device buffers of one case: Operands with a workspace for G tasks"""

    def __init__(self, case, lib):
        self.case, self.lib, self.off = case, lib, case.offs()
        self.inputs = []
        n = sc.ws_floats(case.F, case.G)
        assert case.G * lib.query('ds2_bn_ws_bytes', case.F) == 4 * n
        ws = bc.Flat(n, 0, 'sentinel')
        ws.view().view(np.uint32)[:] = bc.NAN_BITS
        self.ws = Dev(ws)


def _host_ints(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), ctypes.c_void_p)


def _host_ptrs(devs):
    """a host array of device pointers; None passes NULL at its index"""
    return ctypes.cast((ctypes.c_void_p * len(devs))(*[d and d.ptr for d in devs]), ctypes.c_void_p)


def _report(case, entry, ratios):
    for key, r in ratios.items():
        print('RATIO %s %s %s %.4f' % (entry, case.name, key, r))
        assert np.isfinite(r) and r <= 1.0, (case.name, entry, key, r)


def _run(lib, case, p):
    """The three entry points on one set of operands (p: xa, xb, dxf, mi, gamma, beta, rm0, rv0), with the checks every call
    answers to: finite results, nothing written outside an output or behind the workspace, no partial sum left unwritten,
    every input unchanged; eval leaves the running buffers and the workspace as they are.  Returns the results."""
    o = SegOperands(case, lib)
    T, B, F, G = case.T, case.B, case.F, case.G
    tasks = range(G)
    npart = sc.part_floats(F, G)
    xa, dxf, mi_in = o.inp('xa', p.xa), o.inp('dxf', p.dxf), o.inp('mi', p.mi)
    xb = o.inp('xb', p.xb) if p.xb is not None else None
    xbp = xb and xb.ptr
    gamma = [o.inp('gamma%d' % g, p.gamma[g]) for g in tasks]
    beta = [o.inp('beta%d' % g, p.beta[g]) for g in tasks]
    gh, bh, bounds = _host_ptrs(gamma), _host_ptrs(beta), _host_ints(case.bounds)
    res = SimpleNamespace()

    # statistics, training: tasks without running buffers pass NULL at their index, or both host arrays are NULL
    mi = o.out('mi', G * 2 * F)
    rm = [o.out('rm%d' % g, F, p.rm0[g]) if case.has_running(g) else None for g in tasks]
    rv = [o.out('rv%d' % g, F, p.rv0[g]) if case.has_running(g) else None for g in tasks]
    none = case.running is False
    head = (xa.ptr, xbp, T, B, F, G, bounds, bc.EPS, bc.MOMENTUM)
    ws = o.call('ds2_bn1d_seg_stats', *head, 0, None if none else _host_ptrs(rm), None if none else _host_ptrs(rv), mi.ptr,
                o.ws.ptr)
    assert np.isfinite(ws[:npart].view(np.float64)).all(), 'a partial sum that no block wrote'
    assert (ws[npart:].view(np.uint32) == bc.NAN_BITS).all(), 'the statistics do not use coef'
    res.mi = mi.result('mean_invstd').reshape(G, 2 * F)
    res.rm = [d and d.result('running_mean') for d in rm]
    res.rv = [d and d.result('running_var') for d in rv]
    res.mi_eval = None
    if all(case.has_running(g) for g in tasks):
        # eval from the buffers the training call left: they keep every bit, the workspace is not touched
        mi_e = o.out('mi', G * 2 * F)
        before = [d.t.clone() for d in rm + rv]
        ws = o.call('ds2_bn1d_seg_stats', *head, 1, _host_ptrs(rm), _host_ptrs(rv), mi_e.ptr, o.ws.ptr)
        assert (ws.view(np.uint32) == bc.NAN_BITS).all(), 'eval touched the workspace'
        for b, d in zip(before, rm + rv):
            assert torch.equal(b.view(torch.int32), d.t.view(torch.int32)), 'eval changed a running buffer'
        res.mi_eval = mi_e.result('eval mean_invstd').reshape(G, 2 * F)

    y = o.out('y', T * B * F)
    o.call('ds2_bn1d_seg_apply', xa.ptr, xbp, mi_in.ptr, T, B, F, G, bounds, gh, bh, y.ptr)
    res.y = y.result('y').reshape(T * B, F)

    dx = o.out('dy', T * B * F)
    dgamma = [o.out('dgamma%d' % g, F) for g in tasks]
    dbeta = [o.out('dbeta%d' % g, F) for g in tasks]
    ws = o.call('ds2_bn1d_seg_bwd', xa.ptr, xbp, dxf.ptr, mi_in.ptr, T, B, F, G, bounds, gh, dx.ptr, _host_ptrs(dgamma),
                _host_ptrs(dbeta), o.ws.ptr)
    assert np.isfinite(ws[:npart].view(np.float64)).all(), 'a partial sum that no block wrote'
    assert np.isfinite(ws[npart:]).all(), 'a coefficient that no block wrote'
    res.dx = dx.result('dx').reshape(T, B, F)
    res.dgamma = [d.result('dgamma') for d in dgamma]
    res.dbeta = [d.result('dbeta') for d in dbeta]
    o.inputs_unchanged()
    return res


def _check(case, p, res):
    """the results against the per-task float64 references, and against the exact expectations of a 'count' case"""
    F, G = case.F, case.G
    _report(case, 'ds2_bn1d_seg_stats', sc.stats_ratios(p, res.mi))
    if any(case.has_running(g) for g in range(G)):
        _report(case, 'ds2_bn1d_seg_stats', sc.running_ratios(p, res.rm, res.rv))
    for g in range(G):
        assert (res.rm[g] is None) == (not case.has_running(g))
    if res.mi_eval is not None:
        worst = 0.0
        for g in range(G):
            mean_e, inv_e, b_inv = bc.eval_ref(res.rm[g], res.rv[g])
            assert np.array_equal(res.mi_eval[g, :F].view(np.uint32), mean_e.view(np.uint32)), 'eval mean is not the buffer'
            worst = max(worst, float((np.abs(res.mi_eval[g, F:].astype(np.float64) - inv_e) / b_inv).max()))
        _report(case, 'ds2_bn1d_seg_stats(eval)', {'invstd': worst})
    _report(case, 'ds2_bn1d_seg_apply', sc.apply_ratios(p, res.y))
    _report(case, 'ds2_bn1d_seg_bwd', sc.bwd_ratios(p, res.dx, res.dgamma, res.dbeta))
    if case.kind == 'count':
        ex = sc.exact_expectations(p)
        assert np.array_equal(res.y.view(np.uint32), ex.y.view(np.uint32)), 'y is not bit-exact'
        for g in range(G):
            assert np.array_equal(res.mi[g, :F], ex.mean[g]), 'task %d: mean is not float32(S / count)' % g
            assert _ulps(res.mi[g, F:], ex.invstd[g]) <= 1, 'task %d: invstd' % g
            assert np.array_equal(res.dgamma[g], ex.dgamma[g]), 'task %d: dgamma is not exact' % g
            assert np.array_equal(res.dbeta[g], ex.dbeta[g]), 'task %d: dbeta is not exact' % g


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_bn1d_seg_case(lib, case):
    """ds2_bn1d_seg_stats (training, eval), ds2_bn1d_seg_apply, ds2_bn1d_seg_bwd on one set of operands"""
    p = sc.make(case)
    _check(case, p, _run(lib, case, p))


# --------------------------------------------------------------------------------------------- a task alone
@pytest.mark.parametrize('name', sc.ISOLATION)
def test_a_task_does_not_depend_on_its_neighbours(lib, name):
    """Each task's columns copied out to a contiguous (T, B_g, F) tensor and run as a G = 1 launch with the same alignment:
    the same thread adds the same terms in the same order, so every output of the task in the G-task launch equals the
    G = 1 result bit for bit -- mean_invstd, the running buffers, eval, its packed y block, its dx columns, dgamma, dbeta."""
    case = BY[name]
    p = sc.make(case)
    full = _run(lib, case, p)
    T, F = case.T, case.F
    for g in range(case.G):
        b0, b1 = case.bounds[g], case.bounds[g + 1]
        off = tuple((nm, o) for nm, o in case.off if nm in ('xa', 'xb', 'y', 'mi', 'dxf', 'dy'))
        off += tuple((s + '0', dict(case.off)[s + str(g)]) for s in sc.PER_TASK if s + str(g) in dict(case.off))
        one = sc.Seg('alone', T, (0, b1 - b0), F, off=off, xb=case.xb, running=case.has_running(g))
        assert one.forms() == case.forms()
        q = SimpleNamespace(xa=np.ascontiguousarray(p.xa[:, b0:b1]), xb=None, mi=p.mi[g:g + 1].copy(),
                            dxf=np.ascontiguousarray(sc.packed_block(case, p.dxf, g)), gamma=[p.gamma[g]], beta=[p.beta[g]],
                            rm0=[p.rm0[g]], rv0=[p.rv0[g]])
        if p.xb is not None:
            q.xb = np.ascontiguousarray(p.xb[:, b0:b1])
        alone = _run(lib, one, q)
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))   # noqa: E731
        assert same(full.mi[g], alone.mi[0]), 'task %d: mean_invstd' % g
        assert same(sc.packed_block(case, full.y, g), alone.y), 'task %d: y' % g
        assert same(full.dx[:, b0:b1], alone.dx), 'task %d: dx' % g
        assert same(full.dgamma[g], alone.dgamma[0]) and same(full.dbeta[g], alone.dbeta[0]), 'task %d: dgamma, dbeta' % g
        if case.has_running(g):
            assert same(full.rm[g], alone.rm[0]) and same(full.rv[g], alone.rv[0]), 'task %d: running buffers' % g
            assert same(full.mi_eval[g], alone.mi_eval[0]), 'task %d: eval' % g


# --------------------------------------------------------------------------------------------- 16-byte against scalar
@pytest.mark.parametrize('T,bounds,F', sc.BOTH_FORMS_SHAPES)
def test_bn1d_seg_both_forms_on_the_same_data(lib, T, bounds, F):
    """The same data once aligned and once with xa one float off 16-byte alignment (all three entries then take their scalar
    kernels).  Both runs are held to the float64 bounds.  As csrc/bn.hip records for the single-task kernels, the compiler
    may fuse a product into the following sum in one form and not in the other, so equality of the two is not asserted;
    the largest distance in ulps is printed."""
    aligned = sc.Seg('pair', T, bounds, F)
    shifted = sc.Seg('pair', T, bounds, F, off=(('xa', 1),))
    assert set(aligned.forms().values()) == {'vec'} and set(shifted.forms().values()) == {'scalar'}
    p = sc.make(aligned)
    res = {}
    for case in (aligned, shifted):
        res[case] = _run(lib, case, p)
        _check(case, p, res[case])
    a, b = res[aligned], res[shifted]
    pairs = {'mean_invstd': (a.mi, b.mi), 'y': (a.y, b.y), 'dx': (a.dx, b.dx), 'dgamma': (np.stack(a.dgamma), np.stack(b.dgamma)),
             'dbeta': (np.stack(a.dbeta), np.stack(b.dbeta)), 'running_mean': (np.stack(a.rm), np.stack(b.rm)),
             'running_var': (np.stack(a.rv), np.stack(b.rv))}
    for key, (u, v) in pairs.items():
        differ = u.view(np.uint32) != v.view(np.uint32)
        print('ULPS T%d-b%s-F%d %s: %d of %d differ between the two forms, by at most %d ulp'
              % (T, '.'.join(map(str, bounds)), F, key, differ.sum(), differ.size, _ulps(u.reshape(-1), v.reshape(-1))))


# --------------------------------------------------------------------------------------------- through ds2hip.ops, chained
@pytest.mark.parametrize('T,bounds,F', sc.CHAIN)
def test_bn1d_seg_chain_through_ops(lib, T, bounds, F):
    """statistics -> apply -> backward the way codes/model.py calls them, through the wrappers' workspace sizing and pointer
    marshalling: apply and backward read the statistics kernel's own mean_invstd, and are held to float64 under exactly
    those numbers"""
    from ds2hip import ops
    case = sc.Seg('ops', T, bounds, F)
    p0 = sc.make(case)
    G, B = case.G, case.B
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    host = lambda ts: [t.cpu().numpy() for t in ts]                            # noqa: E731
    xa, xb, dxf = dev(p0.xa), dev(p0.xb), dev(p0.dxf)
    gamma, beta = [dev(a) for a in p0.gamma], [dev(a) for a in p0.beta]
    rm, rv = [dev(a) for a in p0.rm0], [dev(a) for a in p0.rv0]
    mi = ops.bn1d_seg_stats(xa, xb, T, B, F, list(bounds), rm, rv, training=True)
    assert mi.shape == (G, 2 * F)
    _report(case, 'ops.bn1d_seg_stats', sc.stats_ratios(p0, mi.cpu().numpy()))
    _report(case, 'ops.bn1d_seg_stats', sc.running_ratios(p0, host(rm), host(rv)))
    p = sc.make(case, mi=mi.cpu().numpy())
    y = ops.bn1d_seg_apply(xa, xb, mi, T, B, F, list(bounds), gamma, beta)
    assert y.shape == (T * B, F)
    _report(case, 'ops.bn1d_seg_apply', sc.apply_ratios(p, y.cpu().numpy()))
    dg = [torch.full((F,), float('nan'), device=DEV) for _ in range(G)]
    db = [torch.full((F,), float('nan'), device=DEV) for _ in range(G)]
    dx = ops.bn1d_seg_bwd(xa, xb, dxf, mi, T, B, F, list(bounds), gamma, dg, db)
    _report(case, 'ops.bn1d_seg_bwd', sc.bwd_ratios(p, dx.cpu().numpy().reshape(T, B, F), host(dg), host(db)))
    mi_e = ops.bn1d_seg_stats(xa, xb, T, B, F, list(bounds), rm, rv, training=False)
    for g in range(G):
        assert torch.equal(mi_e[g, :F], rm[g])
