"""The BatchNorm edge suite's cases are what they claim to be (tests/bn_cases.py); no GPU.

The case table's coverage of both kernel forms of every entry point, the exactness arguments of the integer and edge-value
cases, the borderline cap, the width of the invstd interval, the share of elements on either side of both clamps, the float64
references' agreement with torch in float64, and the room the derived bounds leave a plain fp32 emulation of the kernels'
arithmetic are all checked here, so that a red GPU test speaks about the kernels.  The argument contract of the six entry
points is checked here too: a refused call returns before any HIP call, so it needs no device."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bn_cases as bc

CASES = bc.all_cases()
IDS = [c.name for c in CASES]
_made = {}


def made(case):
    """the case's operands and references, computed once for the module; the big ones are not kept"""
    if case.name in _made:
        return _made[case.name]
    p = bc.make(case)
    if case.count * case.channels <= 300000:
        _made[case.name] = p
    return p


def test_case_names_are_unique():
    assert len(IDS) == len(set(IDS))
    assert len(bc.VEC_SCALAR_SHAPES) == len(set(bc.VEC_SCALAR_SHAPES)) and all(f % 4 == 0 for _, f in bc.VEC_SCALAR_SHAPES)


def test_flat_buffers_show_a_touched_guard():
    for fill in ('nan', 'sentinel'):
        for off in range(4):
            f = bc.Flat(37, off, fill).put(np.arange(37))
            assert f.start % 4 == off and f.size % 4 == 0 and f.start >= bc.GUARD and f.size - f.start - f.n >= bc.GUARD
            assert np.array_equal(f.view(), np.arange(37, dtype=np.float32)) and f.outside_intact(f.buf)
            assert np.isfinite(f.buf[~f.inside()]).all() == (fill == 'sentinel')
            for pos in (0, f.start - 1, f.start + f.n, f.size - 1):
                buf = f.buf.copy()
                buf[pos] = 1.0
                assert not f.outside_intact(buf), (fill, off, pos)
    # the NaN-filled workspace reads as NaN doubles too
    assert np.isnan(bc.Flat(bc.ws_floats(3), 0, 'nan').view().view(np.float64)).all()
    assert bc.ws_floats(32) * 4 == 32 * 64 * 2 * 8 + 32 * 2 * 4


def test_table_covers_both_forms_of_every_entry_point():
    seen = {e: set() for e in bc.ENTRIES}
    for c in CASES:
        for e, f in c.forms().items():
            seen[e].add(f)
    for e in bc.ENTRIES:
        assert seen[e] == {'vec', 'scalar'}, (e, seen[e])
    assert any(c.tbf for c in CASES) and bc.form('bn2d_apply', {}, tbf=True) == 'tbf'
    # and in every kind: a wrong element count in one form must not hide behind the other
    for kind, flavour in (('count', 'conv'), ('count', 'seq'), ('edge', 'conv')):
        for e in bc.ENTRIES[:3] if flavour == 'conv' else bc.ENTRIES[3:]:
            forms = {c.forms()[e] for c in CASES if c.kind == kind and c.flavour == flavour}
            assert forms == {'vec', 'scalar'}, (kind, e, forms)


def test_form_mirror_on_the_cases_the_table_names():
    by = {c.name: c for c in CASES}
    f = lambda name: by[name].forms()         # noqa: E731
    assert set(f('offset-3x3x1x1027-fp64').values()) == {'vec'}
    for k in (1, 2, 3):
        assert set(f('offset-3x3x1x1027-fp64-x%d' % k).values()) == {'scalar'}
    assert f('offset-3x3x1x1027-fp64-dy1') == {'bn2d_stats': 'vec', 'bn2d_apply': 'vec', 'bn2d_bwd': 'scalar'}
    assert f('offset-3x3x1x1027-fp64-y1-dx1') == {'bn2d_stats': 'vec', 'bn2d_apply': 'scalar', 'bn2d_bwd': 'scalar'}
    params = [c for c in CASES if c.section == 'offset' and c.flavour == 'conv' and dict(c.off).get('gamma')]
    assert params and all(set(c.forms().values()) == {'vec'} for c in params)
    # the flat-buffer case: gamma alone off 16-byte alignment at F = 800
    assert f('offset-530x800-fp64-gamma1') == {'bn1d_stats': 'vec', 'bn1d_apply': 'scalar', 'bn1d_bwd': 'scalar'}
    assert f('offset-257x260-fp64-xb1') == {'bn1d_stats': 'scalar', 'bn1d_apply': 'scalar', 'bn1d_bwd': 'scalar'}
    assert f('offset-257x260-fp64-beta1') == {'bn1d_stats': 'vec', 'bn1d_apply': 'scalar', 'bn1d_bwd': 'vec'}
    assert f('offset-257x260-fp64-y1') == {'bn1d_stats': 'vec', 'bn1d_apply': 'scalar', 'bn1d_bwd': 'vec'}
    assert f('offset-257x260-fp64-dx2') == {'bn1d_stats': 'vec', 'bn1d_apply': 'vec', 'bn1d_bwd': 'scalar'}
    assert set(f('offset-257x260-fp64-rm1-rv2-dgamma3-dbeta1').values()) == {'vec'}
    assert set(f('noxb-257x260-fp64-noxb').values()) == {'vec'}
    assert all(set(c.forms().values()) == {'scalar'} for c in CASES if c.flavour == 'seq' and c.F % 4)


def test_table_reaches_every_geometry_edge():
    conv = [c for c in CASES if c.flavour == 'conv']
    seq = [c for c in CASES if c.flavour == 'seq']
    cd = bc.cdiv
    assert {1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027, 1028, 2049} <= {c.inner for c in conv}
    assert {1, 63, 64, 65, 129} <= {c.B * cd(c.inner, 1024) for c in conv}
    # every start of a plane modulo 4, at C = 1, 3 and 32
    for ch in (1, 3, 32):
        starts = {((b * c.C + k) * c.inner) & 3 for c in conv if c.C == ch and c.inner % 2 for b in range(c.B) for k in range(c.C)}
        assert starts == {0, 1, 2, 3}, ch
    # past the 64-block cap of the elementwise kernels, in each form
    assert any(cd(c.inner, 1024) > 64 and c.forms()['bn2d_bwd'] == 'vec' for c in conv)
    assert any(cd(c.inner, 256) > 64 and c.forms()['bn2d_bwd'] == 'scalar' for c in conv)
    # past the 4096-block cap of the sequence kernels, in each form
    assert any(cd(c.rows * c.F, 256) > 4096 and c.forms()['bn1d_bwd'] == 'scalar' for c in seq)
    assert any(cd(c.rows * c.F // 4, 256) > 4096 and c.forms()['bn1d_bwd'] == 'vec' for c in seq)
    assert {1, 30, 63, 64, 65, 36, 252, 256, 260, 800} <= {c.F for c in seq}
    assert {9, 63, 64, 65, 200} <= {c.F // 4 for c in seq if c.F % 4 == 0}
    assert {1, 2, 3, 255, 256, 257, 530} <= {c.rows for c in seq}
    assert any(not c.xb for c in seq) and any(not c.running for c in seq) and any(not c.running for c in conv)
    tbf = [c for c in conv if c.tbf]
    assert {31, 32, 33} <= {c.T for c in tbf} and {31, 32, 33} <= {c.C * c.D for c in tbf}
    assert {21, 61} <= {c.D for c in tbf if c.C > 1} and {1, 3} <= {c.B for c in tbf}
    assert any((c.B, c.C, c.D, c.T) == (2, 32, 61, 75) for c in conv)


@pytest.mark.parametrize('case', [c for c in CASES if c.kind == 'count'], ids=lambda c: c.name)
def test_integer_cases_are_exact_and_a_dropped_element_shows(case):
    p = made(case)
    x = p.xc
    assert np.array_equal(x, np.round(x)) and np.abs(x).min() >= 1 and np.abs(x).max() <= 4
    assert np.array_equal(p.dyc, np.round(p.dyc)) and np.abs(p.dyc).min() >= 1 and np.abs(p.dyc).max() <= 3
    # every sum of every subset is an integer below 2^24: exact in fp32 in any order
    assert (x * x).sum(1).max() < 2 ** 24 and np.abs(p.dyc * x).sum(1).max() < 2 ** 24
    # one element dropped or counted twice moves sum x^2 by at least 1 and sum x, sum dy, sum dy x by at least 1
    assert (x * x).min() >= 1 and np.abs(p.dyc * x).min() >= 1
    # ... which the assertions can see: the fp32 mean resolves S +- 1 (S / count has 24 bits, |S| <= 4 count)
    s = x.sum(1)
    for d in (-1.0, 1.0):
        assert np.all(((s + d) / case.count).astype(np.float32) != (s / case.count).astype(np.float32))
    # everything is interior under beta = 10, and mean_invstd = (0, 1) makes xhat = x
    assert p.bw.borderline == 0 and np.array_equal(p.bw.g, p.dyc) and np.array_equal(p.bw.xh, x)
    assert p.ap.pre.min() >= 6 and p.ap.pre.max() <= 14


@pytest.mark.parametrize('case', [c for c in CASES if c.kind == 'edge'], ids=lambda c: c.name)
def test_edge_cases_put_every_edge_value_in_every_channel(case):
    p = made(case)
    ex = bc.exact_expectations(p)
    for ch in range(case.channels):
        assert set(np.unique(p.xc[ch])) == set(np.unique(bc.EDGE_VALUES.astype(np.float64)))
    xn = p.x
    assert np.signbit(xn).sum() >= 2 * (xn.size // 8)                   # -1 and -0.0
    # y = x exactly under mean_invstd = (0, 1), gamma = 1, beta = 0, so the references hold bit for bit
    assert np.array_equal(p.ap.pre, p.xc) and np.array_equal(case.cm(ex.y.astype(np.float64)), p.ap.y)
    assert not np.signbit(ex.y).any()
    # strict mask: of the eight values only 1 and the float below 20 pass
    assert np.array_equal(case.cm(ex.inside), p.bw.g != 0) and ex.inside.sum() == ((xn == 1) | (xn == bc.EDGE_VALUES[4])).sum()
    assert p.bw.borderline == 0 and p.bw.keep.all()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_borderline_cap_interval_width_and_clamp_shares(case):
    p = made(case)
    assert p.bw.borderline <= bc.BORDER_CAP(case.count * case.channels), p.bw.borderline
    if case.kind != 'fp64':
        return
    st = p.st
    if case.count > 1:
        # |mean| / std stays small enough for the interval to pin invstd (a single element has var = 0: eps alone sets
        # invstd there, and the interval is as wide as t / eps; it is still the check)
        assert ((st.hi - st.lo) / st.invstd).max() < 1e-3
    if case.count > 1:
        assert (np.abs(st.mean) / np.sqrt(st.var)).max() <= 3
    if case.flavour == 'conv' and case.count >= 1000:
        assert (p.ap.pre <= 0).mean(1).min() >= 0.01 and (p.ap.pre >= 20).mean(1).min() >= 0.01
        assert ((p.ap.pre > 0) & (p.ap.pre < 20)).mean(1).min() >= 0.5


# --------------------------------------------------------------------------------------------- references against torch
TORCH_CASES = ['rowstart-3x3x1x5-fp64', 'chunk-2x3x1x1025-fp64', 'tbf-3x3x21x33-fp64', 'items-1x2x1x9-fp64',
               'rows-3x36-fp64', 'rows-257x30-fp64', 'noxb-257x65-fp64-noxb', 'F4-257x36-fp64']


@pytest.mark.parametrize('name', TORCH_CASES)
def test_references_agree_with_torch_in_float64(name):
    import torch
    import torch.nn.functional as tf
    case = {c.name: c for c in CASES}[name]
    p = made(case)
    c = case.channels
    conv = case.flavour == 'conv'
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-12, atol=1e-13)      # noqa: E731
    nat64 = case.nat(p.xc)
    shape = (case.B, case.C, case.D, case.T) if conv else (case.rows, case.F)
    x = torch.from_numpy(nat64.reshape(shape)).requires_grad_(True)
    bn = (torch.nn.BatchNorm2d if conv else torch.nn.BatchNorm1d)(c, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(p.gamma.astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(p.beta.astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(p.rm0.astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(p.rv0.astype(np.float64)))
    y = bn(x)
    if conv:
        y = tf.hardtanh(y, 0, 20)
    y.backward(torch.from_numpy(p.dy.astype(np.float64).reshape(shape)))
    st = bc.stats_ref(p.xc, case.n_run, eps=1e-5)
    run = bc.running_ref(st, p.rm0, p.rv0, momentum=0.1)
    close(run.rm, bn.running_mean)
    close(run.rv, bn.running_var)
    mi = np.concatenate([st.mean, st.invstd])
    xabs = np.abs(p.xc)
    ap = bc.apply_ref(p.xc, xabs, mi, p.gamma, p.beta, conv)
    bw = bc.bwd_ref(p.xc, xabs, p.dyc, mi, p.gamma, p.beta, conv, case.n_run, False)
    close(case.nat(ap.y).reshape(shape), y)
    close(case.nat(bw.dx).reshape(shape), x.grad)
    close(bw.dgamma, bn.weight.grad)
    close(bw.dbeta, bn.bias.grad)
    if conv:
        close(case.tbf_of(case.nat(ap.y)), y.reshape(case.B, case.C * case.D, case.T).permute(2, 0, 1))
    # eval: the running buffers (as they were before the step above) give mean_invstd, and stay what they are
    bn.eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(p.rm0.astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(p.rv0.astype(np.float64)))
        y_eval = bn(x.detach())
        if conv:
            y_eval = tf.hardtanh(y_eval, 0, 20)
    mean_e, inv_e, _ = bc.eval_ref(p.rm0, p.rv0, eps=1e-5)
    ap_e = bc.apply_ref(p.xc, xabs, np.concatenate([mean_e.astype(np.float64), inv_e]), p.gamma, p.beta, conv)
    close(case.nat(ap_e.y).reshape(shape), y_eval)


# --------------------------------------------------------------------------------------------- room in the bounds
F32 = np.float32


def _sum32(case, v):
    """per-channel sum of an fp32 array in the ABI's layout the way the scalar reduction kernels form it: one fp32 partial per
    thread in the kernel's own partition and order, the partials combined in float64"""
    if case.flavour == 'seq':
        k = bc.cdiv(case.rows, 256)
        pad = np.zeros((k * 256, case.F), F32)
        pad[:case.rows] = v
        part = np.zeros((256, case.F), F32)
        for j in range(k):                                              # thread (p, ry) takes rows 4 p + ry + 256 j
            part = part + pad[256 * j:256 * (j + 1)]
        return part.astype(np.float64).sum(0)
    b, c, inner = case.B, case.C, case.inner
    chunks = bc.cdiv(inner, 1024)
    items = b * chunks
    jn = bc.cdiv(items, 64)
    pad = np.zeros((b, c, chunks * 1024), F32)
    pad[:, :, :inner] = v.reshape(b, c, inner)
    arr = np.zeros((c, jn * 64, 1024), F32)
    arr[:, :items] = pad.reshape(b, c, chunks, 1024).transpose(1, 0, 2, 3).reshape(c, items, 1024)
    arr = arr.reshape(c, jn, 64, 4, 256)
    part = np.zeros((c, 64, 256), F32)
    for j in range(jn):                                                 # block p takes items p + 64 j, a thread 4 elements of each
        for u in range(4):
            part = part + arr[:, j, :, u, :]
    return part.astype(np.float64).sum((1, 2))


def _emulate(p):
    """the kernels' formulas in plain fp32 numpy (no contraction); returns what the entry points return"""
    case = p.case
    c, n = case.channels, case.count
    ch = (lambda a: a.astype(F32)[None, :, None]) if case.flavour == 'conv' else (lambda a: a.astype(F32)[None, :])
    v = p.x if p.xb is None else p.x + p.xb
    assert v.dtype == F32
    s0, s1 = _sum32(case, v), _sum32(case, v * v)
    mean = s0 / n
    var = np.maximum(s1 / n - mean * mean, 0)
    mi_stats = np.concatenate([mean, 1 / np.sqrt(var + bc.EPS)]).astype(F32)
    unb = var * n / (n - 1) if n > 1 else var
    rm = ((1 - bc.MOMENTUM) * p.rm0.astype(np.float64) + bc.MOMENTUM * mean).astype(F32)
    rv = ((1 - bc.MOMENTUM) * p.rv0.astype(np.float64) + bc.MOMENTUM * unb).astype(F32)
    mu, inv, ga, be = ch(p.mi[:c]), ch(p.mi[c:]), ch(p.gamma), ch(p.beta)
    xh = (v - mu) * inv
    if case.flavour == 'conv':
        sc = ga * inv
        sh = be - mu * sc
        y = np.minimum(np.maximum(v * sc + sh, F32(0)), F32(20))
        yv = ga * xh + be
        g = np.where((yv > 0) & (yv < 20), p.dy, F32(0))
        t1 = g * xh
    else:
        y = (v - mu) * (ga * inv) + be
        g = p.dy
        t1 = g * (v - mu) * inv
    assert y.dtype == F32 and t1.dtype == F32
    d0, d1 = _sum32(case, g), _sum32(case, t1)
    mg, mgx = ch((d0 / n).astype(F32)), ch((d1 / n).astype(F32))
    dx = ga * inv * (g - mg - xh * mgx)
    assert dx.dtype == F32
    return SimpleNamespace(mi=mi_stats, rm=rm, rv=rv, y=y, dx=dx, dgamma=d1.astype(F32), dbeta=d0.astype(F32))



@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bounds_leave_room_for_a_plain_fp32_emulation(case):
    p = made(case)
    e = _emulate(p)
    ratios = {}
    ratios.update(bc.stats_ratios(p, e.mi))
    ratios.update(bc.running_ratios(p, e.rm, e.rv))
    ratios.update(bc.apply_ratios(p, e.y))
    ratios.update(bc.bwd_ratios(p, e.dx, e.dgamma, e.dbeta))
    assert all(np.isfinite(r) and r <= 1.0 for r in ratios.values()), ratios
    ex = bc.exact_expectations(p)
    if case.kind == 'count':
        c = case.channels
        assert np.array_equal(e.mi[:c], ex.mean) and np.array_equal(e.dbeta, ex.dbeta) and np.array_equal(e.dgamma, ex.dgamma)
        assert np.array_equal(e.y, ex.y)
        assert np.abs(e.mi[c:].view(np.int32) - ex.invstd.view(np.int32)).max() <= 1
    if case.kind == 'edge':
        assert np.array_equal(e.y.view(np.uint32), ex.y.view(np.uint32))


def test_a_wrong_kernel_would_leave_its_bound():
    """the bounds are tight enough to see the mistakes they are there for: a lost clamp, one element dropped from a sum, a
    mean taken over one element too many, a mask that is not strict"""
    by = {c.name: c for c in CASES}
    p = made(by['chunk-2x3x1x1027-fp64'])
    e = _emulate(p)
    c, n = p.case.channels, p.case.count
    unclamped = np.where(p.case.nat(p.ap.pre) >= 20, p.case.nat(p.ap.pre), e.y).astype(F32)
    assert bc.apply_ratios(p, e.y)['y'] <= 1 < bc.apply_ratios(p, unclamped)['y']
    dropped = (e.dbeta.astype(np.float64) - p.case.cm(p.dy)[:, 5]).astype(F32)
    assert bc.bwd_ratios(p, e.dx, e.dgamma, dropped)['dbeta'] > 1
    mi = e.mi.astype(np.float64)
    mi[:c] *= n / (n + 1)
    assert bc.stats_ratios(p, mi.astype(F32))['mean'] > 1
    # a mask that lets y = 20 through: dx moves by gamma invstd dy = dy on an eighth of the elements
    q = made(by['edges-2x3x1x1027-edge'])
    eq = _emulate(q)
    assert bc.bwd_ratios(q, eq.dx, eq.dgamma, eq.dbeta)['dx'] <= 1
    assert bc.bwd_ratios(q, eq.dx + np.where(q.x == 20, q.dy, F32(0)), eq.dgamma, eq.dbeta)['dx'] > 1


# --------------------------------------------------------------------------------------------- the argument contract
P = ctypes.c_void_p(4096)                    # never dereferenced: every call below is refused before any HIP call
ENTRY_ARGS = {
    # name: (well-formed arguments, indices of pointers that must not be NULL, indices of sizes that must be positive)
    'ds2_bn2d_stats': ([P, 2, 3, 5, 1e-5, 0.1, 0, P, P, P, P, None], (0, 9, 10), (1, 2, 3)),
    'ds2_bn2d_apply_htanh': ([P, P, P, P, 2, 3, 5, 7, 0, P, None], (0, 1, 2, 3, 9), (4, 5, 6, 7)),
    'ds2_bn2d_htanh_bwd': ([P, P, P, P, P, 2, 3, 5, 7, P, P, P, P, None], (0, 1, 2, 3, 4, 9, 10, 11, 12), (5, 6, 7, 8)),
    'ds2_bn1d_stats': ([P, P, 6, 8, 1e-5, 0.1, 0, P, P, P, P, None], (0, 9, 10), (2, 3)),
    'ds2_bn1d_apply': ([P, P, P, P, P, 6, 8, P, None], (0, 2, 3, 4, 7), (5, 6)),
    'ds2_bn1d_bwd': ([P, P, P, P, P, 6, 8, P, P, P, P, None], (0, 2, 3, 4, 7, 8, 9, 10), (5, 6)),
}


def _refused(name, args):
    from ds2hip import lib
    handle = lib.load()
    rc = getattr(handle, name)(*args)
    assert rc == lib.ERR_ARG, (name, args, rc)
    assert name.encode() in handle.ds2_last_error()


@pytest.mark.parametrize('name', sorted(ENTRY_ARGS))
def test_bn_entry_points_refuse_null_pointers_and_empty_sizes(name):
    ok, pointers, sizes = ENTRY_ARGS[name]
    for i in pointers:
        args = list(ok)
        args[i] = None
        _refused(name, args)
    for i in sizes:
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            _refused(name, args)


@pytest.mark.parametrize('name', ['ds2_bn2d_stats', 'ds2_bn1d_stats'])
def test_bn_stats_refuse_half_a_pair_of_running_buffers(name):
    ok = ENTRY_ARGS[name][0]
    for use_running in (0, 1):
        for missing in ((7,), (8,)) + (((7, 8),) if use_running else ()):
            args = list(ok)
            args[6] = use_running
            for i in missing:
                args[i] = None
            _refused(name, args)


def test_bn2d_entry_points_refuse_grids_beyond_65535():
    ok = ENTRY_ARGS['ds2_bn2d_stats'][0]
    _refused('ds2_bn2d_stats', ok[:2] + [65536] + ok[3:])
    for name, ib in (('ds2_bn2d_apply_htanh', 4), ('ds2_bn2d_htanh_bwd', 5)):
        ok = ENTRY_ARGS[name][0]
        for b, c in ((65536, 1), (1, 65536), (256, 256), (21846, 3), (65536, 65536), (2 ** 20, 2 ** 12)):     # the last two wrap in 32 bits
            args = list(ok)
            args[ib], args[ib + 1] = b, c
            _refused(name, args)
    args = list(ENTRY_ARGS['ds2_bn2d_apply_htanh'][0])
    args[4], args[8] = 65536, 1                                         # layout_tbf: grid.z = B
    _refused('ds2_bn2d_apply_htanh', args)
