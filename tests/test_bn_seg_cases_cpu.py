"""The segmented BatchNorm edge suite's cases are what they claim to be (tests/bn_seg_cases.py); no GPU.

The case table's coverage of both kernel forms of the three entry points and of every geometry edge, the exactness of the
integer cases, the distance between the tasks' distributions, the per-task float64 references' agreement with torch in
float64 on x[:, b0:b1], the room the derived bounds leave a plain fp32 emulation of the kernels' arithmetic and index
arithmetic, and the mistakes the suite exists for (each applied to that emulation must leave a bound or break an exact
expectation) are all checked here, so that a red GPU test speaks about the kernels.  The argument contract of the three entry
points is checked here too: a refused call returns before any HIP call, so it needs no device."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bn_cases as bc
from tests import bn_seg_cases as sc

CASES = sc.seg_cases()
IDS = [c.name for c in CASES]
BY = {c.name: c for c in CASES}
_made = {}


def made(case):
    """the case's operands and references, computed once for the module; the big ones are not kept"""
    if case.name in _made:
        return _made[case.name]
    p = sc.make(case)
    if case.T * case.B * case.F <= 300000:
        _made[case.name] = p
    return p


# --------------------------------------------------------------------------------------------- the table
def test_case_names_are_unique_and_the_named_cases_exist():
    assert len(IDS) == len(set(IDS))
    assert set(sc.ISOLATION) <= set(IDS)
    iso = [BY[n] for n in sc.ISOLATION]
    assert any(c.G == 8 for c in iso) and any('scalar' in c.forms().values() for c in iso)
    assert all(f % 4 == 0 for _, _, f in sc.BOTH_FORMS_SHAPES)


def test_table_covers_both_forms_of_every_entry_point():
    for kind in ('fp64', 'count'):
        for e in sc.ENTRIES:
            forms = {c.forms()[e] for c in CASES if c.kind == kind}
            assert forms == {'vec', 'scalar'}, (kind, e, forms)
    # ... and at the real width in each form-deciding group: by F alone, by an offset
    assert any(c.F == 800 and set(c.forms().values()) == {'vec'} for c in CASES)
    assert any(c.F == 800 and c.off and 'scalar' in c.forms().values() for c in CASES)
    assert any(c.F == 801 for c in CASES)


def test_form_mirror_on_the_cases_the_table_names():
    f = lambda name: BY[name].forms()         # noqa: E731
    V, S = 'vec', 'scalar'
    forms = lambda a, b, c: {'seg_stats': a, 'seg_apply': b, 'seg_bwd': c}      # noqa: E731
    assert f('F4-T37-b0.3.7-F260-fp64') == forms(V, V, V)
    assert f('offset-T37-b0.3.7-F260-fp64-xa1') == forms(S, S, S)
    assert f('offset-T37-b0.3.7-F260-fp64-xb2') == forms(S, S, S)
    assert f('offset-T37-b0.3.7-F260-fp64-y3') == forms(V, S, V)
    assert f('offset-T37-b0.3.7-F260-fp64-mi1') == forms(V, S, S)
    assert f('offset-T37-b0.3.7-F260-fp64-dxf2') == forms(V, V, S)
    assert f('offset-T37-b0.3.7-F260-fp64-dy3') == forms(V, V, S)
    assert f('offset-T37-b0.3.7-F260-fp64-gamma11') == forms(V, S, S)          # the last task's gamma alone
    assert f('offset-T37-b0.3.7-F260-fp64-beta02') == forms(V, S, V)           # the first task's beta alone
    assert f('offset-T17-b0.4.10-F800-fp64-gamma11') == forms(V, S, S)
    nondec = [c for c in CASES if c.section == 'offset' and dict(c.off).get('rm0')]
    assert nondec and all(set(dict(c.off)) == {s + g for s in ('rm', 'rv', 'dgamma', 'dbeta') for g in '01'} and
                          c.forms() == forms(V, V, V) for c in nondec)
    # a NULL xb counts as aligned, whatever the table says about it
    assert f('noxb-T37-b0.3.7-F260-fp64-noxb') == forms(V, V, V)
    assert f('noxb-T37-b0.3.7-F260-fp64-xa1-noxb') == forms(S, S, S)
    assert sc.Seg('x', 2, (0, 1), 8, off=(('xb', 1),), xb=False).forms() == forms(V, V, V)
    assert all(set(c.forms().values()) == {S} for c in CASES if c.F % 4)
    # every task's gamma and beta is looked at
    for g in range(8):
        assert sc.form('seg_apply', {'gamma%d' % g: 1}, 8, 8) == S and sc.form('seg_apply', {'beta%d' % g: 3}, 8, 8) == S
        assert sc.form('seg_bwd', {'gamma%d' % g: 2}, 8, 8) == S and sc.form('seg_bwd', {'beta%d' % g: 1}, 8, 8) == V
        assert sc.form('seg_stats', {'gamma%d' % g: 1, 'beta%d' % g: 1, 'y': 1, 'mi': 1, 'dxf': 1, 'dy': 1}, 8, 8) == V


def test_table_reaches_every_geometry_edge():
    cd = bc.cdiv
    rows = lambda c: {c.rows(g) for g in range(c.G)}            # noqa: E731
    for e in sc.ENTRIES:
        for form in ('vec', 'scalar'):
            cs = [c for c in CASES if c.forms()[e] == form]
            # rows per task around the reduction's stride of 256, in launches that mix them
            assert {1, 2, 3, 255, 256, 257, 513} <= set().union(*[rows(c) for c in cs]), (e, form)
            assert any(len(rows(c)) > 1 and rows(c) & {255, 256, 257, 513} for c in cs)
            assert {1, 8} <= {c.G for c in cs}
            assert any(c.G == 8 and all(c.bg(g) == 1 for g in range(8)) for c in cs)
            assert any(c.G == 8 and len({c.bg(g) for g in range(8)}) > 2 for c in cs)
            assert any(c.G == 3 and c.bg(1) == 1 and c.bg(0) > 1 and c.bg(2) > 1 for c in cs)
            assert any(c.G == 3 and c.bg(0) == 1 and c.bg(2) == 1 and c.bg(1) > 1 for c in cs)
            assert any(not c.xb for c in cs) and any(c.kind == 'count' for c in cs)
            assert any(c.running is False for c in cs) and any(c.running is True for c in cs)
            assert any(isinstance(c.running, tuple) and True in c.running and False in c.running for c in cs)
    assert {36, 252, 256, 260, 800} <= {c.F for c in CASES if set(c.forms().values()) == {'vec'}}
    assert {9, 63, 64, 65, 200} <= {c.F // 4 for c in CASES if set(c.forms().values()) == {'vec'}}
    assert {1, 30, 63, 64, 65, 801} <= {c.F for c in CASES if set(c.forms().values()) == {'scalar'}}
    assert any(not c.xb and dict(c.off).get('xa') for c in CASES)
    # past the 4096-block cap of the elementwise kernels in each form, fp64 and exact
    for kind in ('fp64', 'count'):
        assert any(cd(c.T * c.B * c.F, 256) > 4096 and c.forms()['seg_bwd'] == 'scalar' and c.kind == kind for c in CASES)
        assert any(cd(c.T * c.B * c.F // 4, 256) > 4096 and c.forms()['seg_bwd'] == 'vec' and c.kind == kind for c in CASES)
    assert any((c.T, c.bounds, c.F) == (749, (0, 3, 7), 800) for c in CASES) and 749 * 7 * 200 > 1048576
    assert any((c.T, c.bounds, c.F) == (437, (0, 1, 3), 801) for c in CASES) and 437 * 3 * 801 > 1048576
    # a scalar launch with blockIdx.y > 0
    assert any(c.F >= 65 and c.F % 4 for c in CASES)
    # every section is repeated with integers
    by_section = {c.section for c in CASES if c.kind == 'fp64'}
    assert by_section == {'F4', 'F', 'offset', 'rows', 'geom', 'noxb', 'running', 'cap'}
    # only the cap cases are above a few hundred kilobytes
    assert all(c.T * c.B * c.F * 4 <= 600000 for c in CASES if c.T not in (749, 437))


def test_workspace_holds_part_and_coef_exactly():
    for F, G in ((1, 1), (30, 3), (800, 8)):
        assert sc.ws_floats(F, G) * 4 == G * (F * 64 * 2 * 8 + F * 2 * 4)
        assert sc.part_floats(F, G) * 4 == G * F * 64 * 2 * 8
        assert sc.ws_floats(F, G) - sc.part_floats(F, G) == G * 2 * F


def test_layout_helpers():
    case = sc.Seg('x', 3, (0, 2, 3, 6), 2)
    T, B, F = 3, 6, 2
    a = np.arange(T * B * F, dtype=np.float32).reshape(T, B, F)
    packed = sc.pack(case, a)
    # written out: packed row T b0 + t B_g + (b - b0) is interleaved row t B + b
    for g in range(3):
        b0, bg = case.bounds[g], case.bg(g)
        for t in range(T):
            for b in range(b0, b0 + bg):
                assert np.array_equal(packed[T * b0 + t * bg + (b - b0)], a[t, b])
                assert np.array_equal(sc.task_rows(case, a, g)[t * bg + (b - b0)], a[t, b])
                assert np.array_equal(sc.task_cm(case, a, g)[:, t * bg + (b - b0)], a[t, b])
    assert np.array_equal(sc.unpack(case, packed), a)
    out = np.zeros_like(a)
    for g in range(3):
        sc.put_task_cm(case, out, g, sc.task_cm(case, a, g))
    assert np.array_equal(out, a)
    assert np.array_equal(sc.packed_block(case, packed, 1), sc.task_rows(case, a, 1))


# --------------------------------------------------------------------------------------------- the values
@pytest.mark.parametrize('case', [c for c in CASES if c.kind == 'fp64'], ids=lambda c: c.name)
def test_tasks_draw_from_distributions_a_factor_of_two_apart(case):
    p = made(case)
    for t in p.tasks:
        n = case.rows(t.g)
        st = t.st
        if n > 1:
            assert ((st.hi - st.lo) / st.invstd).max() < 1e-3           # the interval pins invstd
            assert (np.abs(st.mean) / np.sqrt(st.var)).max() <= 3
        assert t.bw.borderline == 0
    for a, b in zip(p.tasks[:-1], p.tasks[1:]):
        if case.rows(a.g) >= 30 and case.rows(b.g) >= 30:
            assert 1.5 < np.sqrt(b.st.var).mean() / np.sqrt(a.st.var).mean() < 2.7
            assert 1.5 < b.st.mean.mean() / a.st.mean.mean() < 2.7
        assert b.gamma.min() / a.gamma.min() == pytest.approx(2, rel=0.5) and b.gamma.max() > a.gamma.max()
        assert b.beta.min() > a.beta.max() and b.rm0.min() > a.rm0.max() and b.rv0.min() >= a.rv0.max()
    if case.G == 1:                                                     # the single-task distribution of bn_cases
        assert sc.scale(case, 0) == 1


@pytest.mark.parametrize('case', [c for c in CASES if c.kind == 'count'], ids=lambda c: c.name)
def test_integer_cases_are_exact_and_a_misplaced_row_shows(case):
    p = made(case)
    ex = sc.exact_expectations(p)
    for t in p.tasks:
        g, n = t.g, case.rows(t.g)
        x, d = t.xc, t.dyc
        assert np.array_equal(x, np.round(x)) and np.abs(x).min() >= 4 * g + 1 and np.abs(x).max() <= 4 * g + 4
        assert np.array_equal(d, np.round(d)) and np.abs(d).min() >= 3 * g + 1 and np.abs(d).max() <= 3 * g + 3
        # every sum of every subset is an integer below 2^24: exact in fp32 in any order
        assert (x * x).sum(1).max() < 2 ** 24 and np.abs(d * x).sum(1).max() < 2 ** 24
        # one element dropped or counted twice, or a neighbour's row in its place, moves every sum by at least 1 ...
        s = x.sum(1)
        for delta in (-1.0, 1.0):
            assert np.all(((s + delta) / n).astype(np.float32) != (s / n).astype(np.float32))
        # xhat = x under mean_invstd = (0, 1), y an integer
        assert np.array_equal(t.bw.xh, x) and np.array_equal(t.mi, np.r_[np.zeros(case.F), np.ones(case.F)].astype(np.float32))
        assert np.array_equal(t.ap.y, x + 10 + g) and np.array_equal(sc.packed_block(case, ex.y, g), t.ap.y.T)
    # ... and the tasks' ranges are disjoint: a neighbour's row is no member of this task's
    for a, b in zip(p.tasks[:-1], p.tasks[1:]):
        assert np.abs(a.xc).max() < np.abs(b.xc).min() and np.abs(a.dyc).max() < np.abs(b.dyc).min()
        assert a.beta[0] + 1 == b.beta[0]


# --------------------------------------------------------------------------------------------- references against torch
TORCH_CASES = ['F4-T37-b0.3.7-F36-fp64', 'rows-T1-b0.1.3.6-F30-fp64', 'rows-T51-b0.5.6-F36-fp64',
               'geom-T3-b0.1.3.4.8.9.12.14.17-F30-fp64', 'geom-T9-b0.6.7.13-F36-fp64', 'noxb-T37-b0.3.7-F65-fp64-noxb',
               'geom-T37-b0.7-F36-fp64']


@pytest.mark.parametrize('name', TORCH_CASES)
def test_references_agree_with_torch_in_float64(name):
    """per task on x[:, b0:b1], as the reference model's per-head BatchNorm1d sees it: training, the running-buffer update,
    autograd, and the eval path"""
    import torch
    case = BY[name]
    p = made(case)
    T, B, F = case.T, case.B, case.F
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-12, atol=1e-13)      # noqa: E731
    x64 = p.xa.astype(np.float64) + (p.xb.astype(np.float64) if case.xb else 0.0)
    x = torch.from_numpy(x64).requires_grad_(True)
    dxf = torch.from_numpy(p.dxf.astype(np.float64))
    dx_ref = np.empty((T, B, F))
    y_ref = np.empty((T * B, F))
    y_eval_ref = np.empty((T * B, F))
    for t in p.tasks:
        g = t.g
        b0, b1 = case.bounds[g], case.bounds[g + 1]
        if case.rows(g) == 1:
            continue                                                    # torch refuses to train on one value per channel
        bn = torch.nn.BatchNorm1d(F, eps=1e-5, momentum=0.1).double()
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(t.gamma.astype(np.float64)))
            bn.bias.copy_(torch.from_numpy(t.beta.astype(np.float64)))
            bn.running_mean.copy_(torch.from_numpy(t.rm0.astype(np.float64)))
            bn.running_var.copy_(torch.from_numpy(t.rv0.astype(np.float64)))
        y = bn(x[:, b0:b1].reshape(-1, F))                              # (T B_g, F), row t B_g + (b - b0)
        y.backward(dxf[T * b0:T * b1])
        st = bc.stats_ref(t.xc, case.n_run(g), eps=1e-5)
        run = bc.running_ref(st, t.rm0, t.rv0, momentum=0.1)
        close(run.rm, bn.running_mean)
        close(run.rv, bn.running_var)
        mi = np.concatenate([st.mean, st.invstd])
        xabs = np.abs(t.xc)
        ap = bc.apply_ref(t.xc, xabs, mi, t.gamma, t.beta, False)
        bw = bc.bwd_ref(t.xc, xabs, t.dyc, mi, t.gamma, t.beta, False, case.n_run(g), False)
        close(ap.y.T, y)
        close(bw.dgamma, bn.weight.grad)
        close(bw.dbeta, bn.bias.grad)
        sc.put_task_cm(case, dx_ref, g, bw.dx)
        sc.packed_block(case, y_ref, g)[...] = ap.y.T
        close(sc.task_rows(case, dx_ref, g), x.grad[:, b0:b1].reshape(-1, F))
        # eval: the running buffers (as they were before the step above) give mean_invstd, and stay what they are
        bn.eval()
        with torch.no_grad():
            bn.running_mean.copy_(torch.from_numpy(t.rm0.astype(np.float64)))
            bn.running_var.copy_(torch.from_numpy(t.rv0.astype(np.float64)))
            y_eval = bn(x.detach()[:, b0:b1].reshape(-1, F))
        mean_e, inv_e, _ = bc.eval_ref(t.rm0, t.rv0, eps=1e-5)
        ap_e = bc.apply_ref(t.xc, xabs, np.concatenate([mean_e.astype(np.float64), inv_e]), t.gamma, t.beta, False)
        close(ap_e.y.T, y_eval)
        # the layouts, once more through the helpers: packed y, interleaved dx
        close(sc.packed_block(case, y_ref, g), y)
        close(sc.task_rows(case, sc.unpack(case, y_ref), g), y)


# --------------------------------------------------------------------------------------------- the emulation
F32 = np.float32
MUTATIONS = ('dxf_interleaved', 'y_interleaved', 'packed_lt', 'column_lt', 'count_TB', 'neighbour_gamma', 'neighbour_mi',
             'drop', 'swap')


def _seg_of_packed_row(case, R, lt=False):
    g = np.zeros(R.shape, np.int64)
    for k in range(1, case.G):
        first = case.T * case.bounds[k]
        g = np.where(first < R if lt else first <= R, k, g)
    return g


def _seg_of_column(case, b, lt=False):
    g = np.zeros(b.shape, np.int64)
    for k in range(1, case.G):
        g = np.where(case.bounds[k] < b if lt else case.bounds[k] <= b, k, g)
    return g


def _rows_of(a, idx):
    """rows idx of the 2-D array a; a row outside it reads NaN, as the guards around the device operands"""
    ok = (idx >= 0) & (idx < a.shape[0])
    out = a[np.where(ok, idx, 0)]
    out[~ok] = np.nan
    return out


def _sum32(v):
    """column sums of a task's (rows, F) fp32 terms the way bn1d_seg_reduce_kernel forms them: thread (p, ry) takes the task
    rows 4 p + ry + 256 j in turn, one fp32 partial each; the partials are combined in float64"""
    rows, F = v.shape
    k = bc.cdiv(rows, 256)
    pad = np.zeros((k * 256, F), F32)
    pad[:rows] = v
    part = np.zeros((256, F), F32)
    for j in range(k):
        part = part + pad[256 * j:256 * (j + 1)]
    assert part.dtype == F32
    return part.astype(np.float64).sum(0)


def _emulate(p, mut=None):
    """The three entries in plain fp32 numpy (no contraction), with the interleaved and packed index arithmetic of
    csrc/bn_seg.hip written out.  mut: one of MUTATIONS, a mistake the suite must see.  Returns what the entries return:
    mi (G, 2F) from the statistics, the running buffers (None for a task without), y packed, dx interleaved, dgamma and
    dbeta per task -- apply and backward under the GIVEN p.mi."""
    case = p.case
    T, B, F, G = case.T, case.B, case.F, case.G
    b0s = np.asarray(case.bounds[:-1], np.int64)
    bgs = np.asarray([case.bg(g) for g in range(G)], np.int64)
    v = (p.xa if p.xb is None else p.xa + p.xb).reshape(T * B, F)
    assert v.dtype == F32
    dxf = p.dxf
    nb = lambda g: (g + 1) % G          # noqa: E731   the neighbouring task
    mi_stats = np.empty((G, 2 * F), F32)
    rms, rvs, dgs, dbs = [], [], [], []
    coef = np.empty((G, 2 * F), F32)
    for g in range(G):
        b0, bg = int(b0s[g]), int(bgs[g])
        rows = T * bg
        r = np.arange(rows)
        t = r // bg
        src = t * B + b0 + (r - t * bg)                                 # the interleaved row of task row r
        vg = v[src]
        # statistics
        count = float(T * B if mut == 'count_TB' else rows)
        s0, s1 = _sum32(vg), _sum32(vg * vg)
        if mut == 'drop' and g == G - 1:
            s0 = s0 - vg[rows // 2].astype(np.float64)
        mean = s0 / count
        var = np.maximum(s1 / count - mean * mean, 0)
        mi_stats[g] = np.concatenate([mean, 1 / np.sqrt(var + sc.EPS)]).astype(F32)
        if case.has_running(g):
            unb = var * count / (count - 1) if count > 1 else var
            rms.append(((1 - sc.MOMENTUM) * p.rm0[g].astype(np.float64) + sc.MOMENTUM * mean).astype(F32))
            rvs.append(((1 - sc.MOMENTUM) * p.rv0[g].astype(np.float64) + sc.MOMENTUM * unb).astype(F32))
        else:
            rms.append(None)
            rvs.append(None)
        # backward reduction: the gradient from the task's packed block, row T b0 + r
        mu, inv = p.mi[g, :F][None], p.mi[g, F:][None]
        gr = _rows_of(dxf, src if mut == 'dxf_interleaved' else T * b0 + r)
        d0, d1 = _sum32(gr), _sum32(gr * (vg - mu) * inv)
        if mut == 'drop' and g == G - 1:
            d0 = d0 - gr[rows // 2].astype(np.float64)
        dgs.append(d1.astype(F32))
        dbs.append(d0.astype(F32))
        coef[g] = np.concatenate([d0 / count, d1 / count]).astype(F32)
    if mut == 'swap':
        dgs, dbs = dbs, dgs
    gam, bet = np.stack(p.gamma), np.stack(p.beta)
    # apply: packed row R -> task, task row, interleaved row
    R = np.arange(T * B)
    g = _seg_of_packed_row(case, R, lt=mut == 'packed_lt')
    r = R - T * b0s[g]
    t = r // bgs[g]
    o = t * B + b0s[g] + (r - t * bgs[g])
    gm = nb(g) if mut == 'neighbour_mi' else g
    gg = nb(g) if mut == 'neighbour_gamma' else g
    scl = gam[gg] * p.mi[gm, F:]
    yv = (_rows_of(v, o) - p.mi[gm, :F]) * scl + bet[g]
    assert yv.dtype == F32
    y = np.full((T * B, F), np.nan, F32)
    if mut == 'y_interleaved':
        ok = o < T * B
        y[o[ok]] = yv[ok]
    else:
        y[R] = yv
    # backward, elementwise: interleaved row S = t B + b -> task, packed row P
    S = np.arange(T * B)
    t = S // B
    b = S - t * B
    g = _seg_of_column(case, b, lt=mut == 'column_lt')
    P = T * b0s[g] + t * bgs[g] + (b - b0s[g])
    gm = nb(g) if mut == 'neighbour_mi' else g
    gg = nb(g) if mut == 'neighbour_gamma' else g
    inv = p.mi[gm, F:]
    xh = (v - p.mi[gm, :F]) * inv
    dx = gam[gg] * inv * (_rows_of(dxf, S if mut == 'dxf_interleaved' else P) - coef[g, :F] - xh * coef[g, F:])
    assert dx.dtype == F32
    return SimpleNamespace(mi=mi_stats, rm=rms, rv=rvs, y=y, dx=dx.reshape(T, B, F), dgamma=dgs, dbeta=dbs)


def _all_ratios(p, e):
    ratios = {}
    ratios.update(sc.stats_ratios(p, e.mi))
    if any(r is not None for r in e.rm):
        ratios.update(sc.running_ratios(p, e.rm, e.rv))
    ratios.update(sc.apply_ratios(p, e.y))
    ratios.update(sc.bwd_ratios(p, e.dx, e.dgamma, e.dbeta))
    return ratios


def _exact_ok(p, e):
    """the exact expectations of a 'count' case, as the GPU suite asserts them"""
    ex = sc.exact_expectations(p)
    F = p.case.F
    ok = np.array_equal(e.y, ex.y)
    for g in range(p.case.G):
        ok = ok and np.array_equal(e.mi[g, :F], ex.mean[g]) and np.array_equal(e.dgamma[g], ex.dgamma[g])
        ok = ok and np.array_equal(e.dbeta[g], ex.dbeta[g])
        ok = ok and np.abs(e.mi[g, F:].view(np.int32).astype(np.int64) - ex.invstd[g].view(np.int32)).max() <= 1
    return bool(ok)


def _inside(p, e):
    ratios = _all_ratios(p, e)
    ok = all(np.isfinite(r) and r <= 1.0 for r in ratios.values())
    if p.case.kind == 'count':
        ok = ok and _exact_ok(p, e)
    return ok, ratios


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bounds_leave_room_for_a_plain_fp32_emulation(case):
    p = made(case)
    e = _emulate(p)
    ok, ratios = _inside(p, e)
    assert ok, ratios
    assert set(ratios) >= {'mean', 'invstd', 'y', 'dx', 'dgamma', 'dbeta'}
    assert ('running_mean' in ratios) == any(case.has_running(g) for g in range(case.G))
    for g in range(case.G):
        assert (e.rm[g] is None) == (not case.has_running(g))


MUTATION_CASES = ['F4-T37-b0.3.7-F36-fp64', 'geom-T3-b0.1.3.4.8.9.12.14.17-F30-fp64', 'geom-T9-b0.6.7.13-F36-fp64',
                  'once-T37-b0.3.7-F260-count', 'once-T3-b0.1.3.4.8.9.12.14.17-F30-count', 'once-T9-b0.1.7.8-F30-count']


# the integer cases give every task gamma = 1 and mean_invstd = (0, 1): a neighbour's is the same, so the fp64 cases hold those
@pytest.mark.parametrize('name,mut', [(n, m) for n in MUTATION_CASES for m in MUTATIONS
                                      if not (n.endswith('count') and m.startswith('neighbour'))])
def test_a_wrong_kernel_would_leave_its_bound(name, mut):
    """the mistakes the suite exists for: the packed gradient read as if interleaved, y written interleaved, a boundary column
    or row given to the neighbouring task (< for <= in either lookup), the count taken as T B, the neighbouring task's gamma
    or mean_invstd row, one element dropped from one task's sums, dgamma and dbeta swapped"""
    p = made(BY[name])
    assert _inside(p, _emulate(p))[0]
    ok, ratios = _inside(p, _emulate(p, mut))
    assert not ok, (name, mut, ratios)


# --------------------------------------------------------------------------------------------- the argument contract
P = ctypes.c_void_p(4096)                    # never dereferenced: every call below is refused before any HIP call
INT_MAX = 2 ** 31 - 1


def _ints(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), ctypes.c_void_p)


def _ptrs(n, null_at=None):
    vals = [None if i == null_at else 4096 for i in range(n)]
    return ctypes.cast((ctypes.c_void_p * n)(*vals), ctypes.c_void_p)


G_OK, BOUNDS_OK = 3, (0, 2, 3, 5)
# name: (well-formed arguments, indices of plain pointers that must not be NULL, indices of T B F, of G, of bounds,
#        indices of host arrays of G device pointers whose entries must not be NULL)
ENTRY_ARGS = {
    'ds2_bn1d_seg_stats': (lambda: [P, P, 6, 5, 8, G_OK, _ints(BOUNDS_OK), 1e-5, 0.1, 0, _ptrs(G_OK), _ptrs(G_OK), P, P, None],
                           (0, 6, 12, 13), (2, 3, 4), 5, 6, ()),
    'ds2_bn1d_seg_apply': (lambda: [P, P, P, 6, 5, 8, G_OK, _ints(BOUNDS_OK), _ptrs(G_OK), _ptrs(G_OK), P, None],
                           (0, 2, 7, 8, 9, 10), (3, 4, 5), 6, 7, (8, 9)),
    'ds2_bn1d_seg_bwd': (lambda: [P, P, P, P, 6, 5, 8, G_OK, _ints(BOUNDS_OK), _ptrs(G_OK), P, _ptrs(G_OK), _ptrs(G_OK), P,
                                  None],
                         (0, 2, 3, 8, 9, 10, 11, 12, 13), (4, 5, 6), 7, 8, (9, 11, 12)),
}


def _refused(name, args):
    from ds2hip import lib
    handle = lib.load()
    rc = getattr(handle, name)(*args)
    assert rc == lib.ERR_ARG, (name, args, rc)
    assert name.encode() in handle.ds2_last_error()


@pytest.mark.parametrize('name', sorted(ENTRY_ARGS))
def test_seg_entry_points_refuse_null_pointers_and_empty_sizes(name):
    ok, pointers, sizes, ig, ib, arrays = ENTRY_ARGS[name]
    for i in pointers:
        args = ok()
        args[i] = None
        _refused(name, args)
    for i in arrays:
        for g in range(G_OK):                                           # a NULL inside a host array of device pointers
            args = ok()
            args[i] = _ptrs(G_OK, null_at=g)
            _refused(name, args)
    for i in sizes:
        for bad in (0, -1):
            args = ok()
            args[i] = bad
            _refused(name, args)


@pytest.mark.parametrize('name', sorted(ENTRY_ARGS))
def test_seg_entry_points_refuse_bad_segments(name):
    ok, _, sizes, ig, ib, _ = ENTRY_ARGS[name]
    for g in (0, 9, -1):
        args = ok()
        args[ig] = g
        _refused(name, args)
    # not starting at 0, not ending at B (short of it, past it), not strictly increasing (empty, decreasing)
    for bounds in ((1, 2, 3, 5), (0, 2, 3, 4), (0, 2, 3, 6), (0, 2, 2, 5), (0, 3, 2, 5), (0, 0, 3, 5), (0, 2, 5, 5)):
        args = ok()
        args[ib] = _ints(bounds)
        _refused(name, args)
    # G = 8 is the most: nine bounds that are well formed are still refused as G = 9
    args = ok()
    args[ig], args[ib], args[sizes[1]] = 9, _ints(tuple(range(10))), 9
    _refused(name, args)


@pytest.mark.parametrize('name', sorted(ENTRY_ARGS))
def test_seg_entry_points_refuse_more_rows_than_an_int_holds(name):
    """the kernels index a task's rows in int (rows = T * B_g, r = R - T * b0): T * B > INT_MAX is refused before any launch"""
    ok, _, sizes, ig, ib, _ = ENTRY_ARGS[name]
    for T, bounds in ((65536, (0, 32768)), (32768, (0, 65536)), (INT_MAX, (0, 1, 2)), (46341, (0, 3, 46341)),
                      (65536, (0, 65536)), (2 ** 20, (0, 2 ** 12, 2 ** 13))):     # the last two wrap in 32 bits
        assert T * bounds[-1] > INT_MAX
        args = ok()
        args[sizes[0]], args[sizes[1]], args[ig], args[ib] = T, bounds[-1], len(bounds) - 1, _ints(bounds)
        _refused(name, args)


def test_seg_stats_refuses_half_a_pair_of_running_buffers_and_eval_without_them():
    name = 'ds2_bn1d_seg_stats'
    ok = ENTRY_ARGS[name][0]
    for use_running in (0, 1):
        for i in (10, 11):                                              # one whole host array missing
            args = ok()
            args[9], args[i] = use_running, None
            _refused(name, args)
        for i in (10, 11):                                              # one task's buffer missing in one array
            for g in range(G_OK):
                args = ok()
                args[9], args[i] = use_running, _ptrs(G_OK, null_at=g)
                _refused(name, args)
    # use_running = 1 with a task's buffers missing altogether, or with no buffers at all
    for g in range(G_OK):
        args = ok()
        args[9], args[10], args[11] = 1, _ptrs(G_OK, null_at=g), _ptrs(G_OK, null_at=g)
        _refused(name, args)
    args = ok()
    args[9], args[10], args[11] = 1, None, None
    _refused(name, args)
