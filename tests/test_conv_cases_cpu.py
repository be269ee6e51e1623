"""The convolution edge suite's cases are what they claim to be (tests/conv_cases.py); no GPU.

The table's reach -- every kernel form the release library can launch, both sides of every threshold of the launchers --, the
integer caps, the float64 references' agreement with torch in float64, and what a plain fp32 emulation of every case gives
(exact for the integer and selection cases, inside the bound for the float64 ones; NOT so with one tap dropped, shifted by a
column or counted twice) are all checked here, so that a red GPU test speaks about the kernels.  The argument contract of the
three entry points is checked here too: a refused call returns before any HIP call, so it needs no device."""
import ctypes

import numpy as np
import pytest

from tests import conv_cases as cc

CASES = cc.all_cases()
IDS = [c.name for c in CASES]
FORMS = {c.name: c.form() for c in CASES}
F32, F64 = np.float32, np.float64


def test_case_names_are_unique_and_operands_fit():
    assert len(IDS) == len(set(IDS))
    for c in CASES:
        assert max(int(np.prod(s)) for s in c.shapes()) * 4 <= 42e6, c.name           # the largest operand: about 40 MB
        assert 0 <= c.off < 4


def test_workspace_sizes_mirror_the_library():
    from ds2hip import lib
    for which in (1, 2):
        assert lib.query('ds2_conv_wt_ws_floats', which) == cc.wt_ws_floats(which)
    for b, t1 in ((1, 11), (3, 139), (289, 11), (2, 1600)):
        assert lib.query('ds2_conv2_dgrad_ws_floats', b, t1) == cc.dgrad_ws_floats(b, t1)


# --------------------------------------------------------------------------------------------- the table's reach
RELEASE_KERNELS = {
    'fwd': {'gather6-nt1', 'gather6-nt2', 'gather9-nt1', 'gather9-nt2', 'direct-nt2-ks4', 'direct-nt2-ks2', 'direct-nt2-ks1',
            'conv1-nt1-ks1', 'conv1-nt2-ks1'},
    'dgrad': {'dgrad-gather6', 'dgrad-gather9', 'dgrad-direct-nt2-ks4'},
    'wgrad': {'wgrad%d-%s' % (w, f) for w in (1, 2) for f in ('direct', 'lds', 'split')},
}


def _wg(which, kind, pred):
    return lambda c, f: f.kernel == 'wgrad%d-%s' % (which, kind) and pred(f)


# name -> predicate(case, form): every one must hold for at least one case of each reference kind listed
EDGES = {
    # forward, gather: cdiv(M, 64) = 1535 | 1536, per product count
    'fwd gather6 one below 64 pos/wave': lambda c, f: f.kernel == 'gather6-nt1' and f.get('side') == -1,
    'fwd gather6 at 64 pos/wave': lambda c, f: f.kernel == 'gather6-nt2' and f.get('side') == 0,
    'fwd gather9 one below 64 pos/wave': lambda c, f: f.kernel == 'gather9-nt1' and f.get('side') == -1,
    'fwd gather9 at 64 pos/wave': lambda c, f: f.kernel == 'gather9-nt2' and f.get('side') == 0,
    'fwd gather nt2 with 24 batch elements': lambda c, f: f.kernel == 'gather6-nt2' and c.B == 24,
    'fwd gather one partly filled workgroup': lambda c, f: f.kernel.startswith('gather') and f.get('M') < 128,
    'fwd gather tiles % 8 != 0, several XCD shares': lambda c, f: f.kernel.startswith('gather') and f.get('tiles8') and f.get('tiles') > 8,
    'fwd gather nt2 ragged last workgroup': lambda c, f: f.kernel == 'gather6-nt2' and f.get('ragged'),
    # forward, direct conv2: 700 and 4096 tiles (a batch element adds 21)
    'fwd direct ks4 below 700': lambda c, f: f.kernel == 'direct-nt2-ks4' and 679 <= f.get('ntiles') < 700,
    'fwd direct ks2 from 700': lambda c, f: f.kernel == 'direct-nt2-ks2' and 700 <= f.get('ntiles') < 721,
    'fwd direct ks2 below 4096': lambda c, f: f.kernel == 'direct-nt2-ks2' and 4075 <= f.get('ntiles') < 4096,
    'fwd direct ks1 from 4096': lambda c, f: f.kernel == 'direct-nt2-ks1' and 4096 <= f.get('ntiles') < 4117,
    'fwd direct ks2 empty slot (odd tiles)': lambda c, f: f.kernel == 'direct-nt2-ks2' and f.get('empty_slots') == 1,
    'fwd direct ks2 even tiles': lambda c, f: f.kernel == 'direct-nt2-ks2' and f.get('empty_slots') == 0,
    'fwd direct ks1 tiles % 4 != 0': lambda c, f: f.kernel == 'direct-nt2-ks1' and f.get('empty_slots') > 0,
    'fwd direct ks1 tiles % 4 == 0': lambda c, f: f.kernel == 'direct-nt2-ks1' and f.get('empty_slots') == 0,
    'fwd direct several time tiles, ragged': lambda c, f: f.kernel == 'direct-nt2-ks4' and f.get('ragged') and c.T > 74,
    # forward, conv1
    'fwd conv1 nt2, even T_in': lambda c, f: f.kernel == 'conv1-nt2-ks1' and c.T % 2 == 0,
    'fwd conv1 nt2, odd T_in': lambda c, f: f.kernel == 'conv1-nt2-ks1' and c.T % 2 == 1,
    'fwd conv1 nt1': lambda c, f: f.kernel == 'conv1-nt1-ks1' and not f.get('pad_only'),
    'fwd conv1 nt1 every tap in the padding': lambda c, f: f.kernel == 'conv1-nt1-ks1' and f.get('pad_only'),
    'fwd conv1 one frame': lambda c, f: c.entry == 'fwd' and c.which == 1 and c.T == 1,
    # data gradient, gather
    'dgrad K splits 2 | 3': lambda c, f: f.get('nsplit') == (2, 3),
    'dgrad K splits 1 | 2, one fill for both': lambda c, f: f.get('nsplit') == (1, 2) and f.get('zero_fill'),
    'dgrad K splits 3 | 3': lambda c, f: f.get('nsplit') == (3, 3),
    'dgrad 2 | 3 with five batch elements': lambda c, f: f.get('nsplit') == (2, 3) and c.B == 5,
    'dgrad plans NT 2 | 1, merged on NT 2': lambda c, f: f.get('plan_nt') == (2, 1) and f.get('merged') and f.get('nts') == (2, 2),
    'dgrad plans NT 2 | 1 with ten batch elements': lambda c, f: f.get('plan_nt') == (2, 1) and f.get('merged') and c.B == 10,
    'dgrad merged, NT 1, no fill': lambda c, f: f.get('merged') and f.get('nts') == (1, 1) and not f.get('zero_fill'),
    'dgrad row walk across batch elements': lambda c, f: f.get('merged') and f.get('two_batch') and f.get('walk') == (True, True),
    'dgrad one parity walks, the other splits': lambda c, f: f.get('walk') == (True, False) and f.get('zero_fill') and c.T == 11,
    'dgrad a workgroup spans more than 20 rows': lambda c, f: (f.get('max_rows') or 0) > 20,
    'dgrad a workgroup spans 2..20 rows': lambda c, f: 2 <= (f.get('max_rows') or 0) <= 20,
    'dgrad gather, 9 products': lambda c, f: f.kernel == 'dgrad-gather9',
    'dgrad walk off (DGRAD_ROWS=0)': lambda c, f: f.kernel == 'dgrad-gather6' and f.get('walk') == (False, False) and f.get('nsplit') == (1, 1),
    'dgrad merge off': lambda c, f: f.kernel == 'dgrad-gather6' and not f.get('merged') and f.get('nsplit') == (1, 1),
    # data gradient, default choice: B T1 = 999 | 1000
    'dgrad default below 1000 is direct': lambda c, f: not c.env and f.kernel.startswith('dgrad-direct') and f.get('side') == -1,
    'dgrad default at 1000 is gather': lambda c, f: not c.env and f.kernel == 'dgrad-gather6' and f.get('side') == 0,
    'dgrad default one above 1000': lambda c, f: not c.env and f.kernel == 'dgrad-gather6' and f.get('side') == 1,
    'dgrad default below, several batch elements': lambda c, f: not c.env and f.kernel.startswith('dgrad-direct') and c.B > 1,
    'dgrad direct forced, ragged': lambda c, f: c.envd().get('DS2_CONV_SPLIT_DGRAD') == '0' and f.get('ragged'),
    'dgrad direct forced, T1 = 64': lambda c, f: c.envd().get('DS2_CONV_SPLIT_DGRAD') == '0' and c.T == 64,
    'dgrad direct forced, T1 = 65': lambda c, f: c.envd().get('DS2_CONV_SPLIT_DGRAD') == '0' and c.T == 65,
}
for _w in (1, 2):
    for _k in ('lds', 'split'):
        EDGES['wgrad%d %s split > rows' % (_w, _k)] = _wg(_w, _k, lambda f: f.get('clamp') > 0)
        EDGES['wgrad%d %s split < rows, uneven' % (_w, _k)] = _wg(_w, _k, lambda f: f.get('clamp') < 0 and f.get('uneven'))
        EDGES['wgrad%d %s two time chunks' % (_w, _k)] = _wg(_w, _k, lambda f: f.get('tchunks') == 2 and f.get('ragged') == 1)
        EDGES['wgrad%d %s one full chunk' % (_w, _k)] = _wg(_w, _k, lambda f: f.get('tchunks') == 1 and f.get('ragged') == 0)
    EDGES['wgrad%d direct nsplit clamped' % _w] = _wg(_w, 'direct', lambda f: f.get('clamp') > 0)
    EDGES['wgrad%d direct nsplit not clamped' % _w] = _wg(_w, 'direct', lambda f: f.get('clamp') <= 0)
    # TOUT = 1 needs t_in_frames <= 0 in conv1 (refused): its smallest TOUT is 6
    for _t in ((6, 7, 8, 63, 64, 65) if _w == 1 else (1, 7, 8, 63, 64, 65)):
        for _k in ('direct', 'lds', 'split'):
            EDGES['wgrad%d %s TOUT %d' % (_w, _k, _t)] = _wg(_w, _k, lambda f, t=_t: f.get('tout') == t)
for _k in ('lds', 'split'):
    EDGES['wgrad2 %s rows == split' % _k] = _wg(2, _k, lambda f: f.get('clamp') == 0)      # (61 B = 256 has no solution in conv1)
for _k in ('direct', 'lds', 'split'):
    EDGES['wgrad1 %s every tap in the padding' % _k] = _wg(1, _k, lambda f: f.get('pad_only'))


def test_table_reaches_every_release_kernel():
    for entry, want in RELEASE_KERNELS.items():
        for ref in ('int', 'sel'):
            got = {FORMS[c.name].kernel for c in CASES if c.entry == entry and c.ref == ref}
            assert got == want, (entry, ref, got ^ want)
        got = {FORMS[c.name].kernel for c in CASES if c.entry == entry and c.ref == 'fp64'}
        assert got == want - {'gather9-nt2', 'dgrad-gather9'}, (entry, got ^ want)


@pytest.mark.parametrize('edge', sorted(EDGES))
def test_table_sits_on_both_sides_of_every_threshold(edge):
    hit = [c for c in CASES if EDGES[edge](c, FORMS[c.name])]
    assert {c.ref for c in hit} >= {'int', 'sel'}, (edge, [c.name for c in hit])


def test_only_case_on_its_side_is_missed_when_removed():
    """the edges are named so that a case table without its only case on one side fails the reach test above"""
    alone = {}
    for edge, pred in EDGES.items():
        hit = {(c.entry, c.which, c.B, c.T, c.env) for c in CASES if pred(c, FORMS[c.name])}
        if len(hit) == 1:
            alone[edge] = next(iter(hit))
    for edge, (entry, which, b, t, env) in alone.items():
        rest = [c for c in CASES if (c.entry, c.which, c.B, c.T, c.env) != (entry, which, b, t, env)]
        assert not any(EDGES[edge](c, FORMS[c.name]) for c in rest)
    assert len(alone) >= 20                         # most thresholds have exactly one smallest shape on a side


def test_mirror_on_the_shapes_the_issue_names():
    f = cc.fwd_form
    assert f(2, 6, 400).get('M') == 49140 and f(2, 2, 2349).kernel == 'gather6-nt1' and f(2, 1, 4689).kernel == 'gather6-nt2'
    assert [f(2, b, 11, {'DS2_CONV_SPLIT': '0'}).kernel[-3:] for b in (33, 34, 35, 195, 196)] == ['ks4', 'ks2', 'ks2', 'ks2', 'ks1']
    assert f(1, 2, 629).kernel == 'conv1-nt2-ks1' and f(1, 9, 120).kernel == 'conv1-nt1-ks1' and f(1, 2, 121).kernel == 'conv1-nt1-ks1'
    on = {'DS2_CONV_SPLIT_DGRAD': '1'}
    d = cc.dgrad_form
    assert d(1, 530, on).get('nsplit') == (2, 3) and d(1, 1060, on).get('nsplit') == (1, 2) and d(3, 11, on).get('nsplit') == (3, 3)
    assert d(96, 11, on).get('walk') == (True, False) and d(100, 11, on).get('two_batch')
    for bt1 in (3170, 3274):
        assert d(1, bt1, on).get('plan_nt') == (2, 1) and d(1, bt1, on).get('merged')
    assert d(1, 3169, on).get('plan_nt') == (1, 1) and d(1, 3275, on).get('plan_nt') == (2, 2)
    w = cc.wgrad_form
    assert w(1, 8, 21, cc.WGRAD_ENV['direct']).get('nsplit') == 122 and w(1, 9, 21, cc.WGRAD_ENV['direct']).get('nsplit') == 137
    assert w(2, 5, 23).get('split') == 105 and w(2, 4, 21).get('split') == 84 and w(1, 4, 30).get('split') == 244


# --------------------------------------------------------------------------------------------- operands and references
_made = {}


def made(case):
    """operands, the expected result and the fp32 emulation of a case, once per (entry, layer, shape, reference kind)"""
    key = case.key()
    if key in _made:
        return _made[key]
    data, other, bias, extra = cc.make_ops(case)
    emu = cc.convolve(case.entry, case.which, data, other, F32, bias)
    m = dict(data=data, other=other, bias=bias, extra=extra, emu=emu)
    if case.entry == 'wgrad':
        m['emu_b'] = cc.bias_grad(other, F32)
    if case.ref == 'sel':
        m['want'] = cc.sel_reference(case, data, extra)
    else:
        m['want'] = cc.convolve(case.entry, case.which, data, other, F64, bias)
    if max(data.size, emu.size) <= 400000:
        _made[key] = m
    return m


UNIQUE = list({c.key(): c for c in CASES}.values())


@pytest.mark.parametrize('case', UNIQUE, ids=lambda c: '%s%d-%dx%d-%s' % c.key())
def test_fp32_emulation_is_exact_or_bounded_and_a_wrong_tap_shows(case):
    m = made(case)
    emu, want = m['emu'], m['want']
    assert np.isfinite(emu).all()
    if case.ref == 'int':
        v = m['extra']
        amax, bmax = float(np.abs(m['data']).max()), float(np.abs(m['other']).max())
        bias_max = float(np.abs(m['bias']).max()) if m['bias'] is not None else 0.0
        assert amax <= v and bmax <= v and amax >= 1 and bmax >= 1
        assert 2 * amax * bmax * case.K() + bias_max < 2 ** 24, 'the integer cap'
        assert np.array_equal(emu.astype(F64), want)
        if case.entry == 'wgrad':
            assert np.array_equal(m['emu_b'].astype(F64), cc.bias_grad(m['other'], F64))
            assert np.abs(cc.bias_grad(m['other'], F64)).max() < 2 ** 24
    elif case.ref == 'sel':
        if case.entry == 'wgrad':
            want, want_b = want
            assert np.array_equal(m['emu_b'], want_b)
        assert np.array_equal(emu, want)
        nz = np.count_nonzero(want)
        assert nz >= want.size // 64 or case.which == 1, 'a selection case that selects almost nothing'
        assert nz > 0
    else:
        form = case.form()
        scale = cc.convolve(case.entry, case.which, np.abs(m['data']), np.abs(m['other']), F64,
                            None if m['bias'] is None else np.abs(m['bias']))
        ratio = cc.worst_ratio(np.abs(emu.astype(F64) - want), cc.fp64_bound(form, scale))
        assert ratio <= 1.0, ratio
        if case.entry == 'wgrad':
            sb = cc.bias_grad(np.abs(m['other']), F64)
            assert (np.abs(m['emu_b'].astype(F64) - cc.bias_grad(m['other'], F64)) <= cc.fp64_bound(form, sb)).all()
        return
    tap = cc.tamper_tap(case, m['extra'])
    for kind in ('drop', 'shift', 'twice'):
        bad = cc.tampered(case.entry, case.which, m['data'], m['other'], emu, kind, tap)
        assert not np.array_equal(bad.astype(want.dtype), want), (kind, tap)


def test_selection_cases_use_every_bf16_plane_and_the_filter_corners():
    case = next(c for c in CASES if c.entry == 'fwd' and c.which == 2 and c.ref == 'sel' and c.B * c.T < 200)
    m = made(case)
    ci, taps, sg = m['extra']
    assert {(0, 0), (0, 10), (20, 0), (20, 10), (19, 8), (1, 7)} <= set(taps) and set(sg) == {-1.0, 1.0}
    assert {0, 1, 30, 31} <= set(ci.tolist())
    bits = m['data'].view(np.uint32)
    assert (bits & 1).all(), 'the last significand bit is in use: the third bf16 plane is not zero'
    dcase = next(c for c in CASES if c.entry == 'dgrad' and c.ref == 'sel')
    assert sorted(cc.make_ops(dcase)[3][0].tolist()) == list(range(32))


def _torch_conv(which, x, w, b):
    import torch.nn.functional as F
    return F.conv2d(x, w, b, stride=(2, 2), padding=(0, 10)) if which == 1 else F.conv2d(x, w, b, stride=(2, 1))


@pytest.mark.parametrize('which,b,t', [(1, 2, 30), (1, 1, 5), (1, 3, 33), (2, 2, 15), (2, 1, 11), (2, 3, 40)])
def test_references_agree_with_torch_in_float64(which, b, t):
    import torch
    g = cc.GEOM[which]
    rng = np.random.default_rng(which * 100 + t)
    x = rng.standard_normal((b, g.cin, g.fin, t))
    w = rng.standard_normal((32, g.cin, g.kf, g.kt))
    bias = rng.standard_normal(32)
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, bias))
    out = _torch_conv(which, xt, wt, bt)
    dy = rng.standard_normal(tuple(out.shape))
    out.backward(torch.from_numpy(dy))
    tol = 1e-12 * g.cin * g.kf * g.kt
    assert np.abs(cc.convolve('fwd', which, x, w, F64, bias) - out.detach().numpy()).max() <= tol
    assert np.abs(cc.convolve('wgrad', which, x, dy, F64) - wt.grad.numpy()).max() <= 1e-12 * dy.size
    assert np.abs(cc.bias_grad(dy, F64) - bt.grad.numpy()).max() <= 1e-12 * dy.size
    if which == 2:
        assert np.abs(cc.convolve('dgrad', 2, dy, w, F64) - xt.grad.numpy()).max() <= tol


def test_tout_and_padding_of_conv1_below_eleven_frames():
    for tin in range(1, 11):
        assert cc.conv_tout(1, tin) == (tin + 20 - 11) // 2 + 1 >= 6
        xp = cc.padded(1, np.ones((1, 1, 161, tin)), F32)
        tout = cc.conv_tout(1, tin)
        for t in range(tout):                       # every output's 11-tap window touches the padding
            assert (xp[0, 0, 0, 2 * t:2 * t + 11] == 0).any()


# --------------------------------------------------------------------------------------------- the argument contract
P = ctypes.c_void_p(4096)                    # never dereferenced: every call below is refused before any HIP call
WS2 = cc.wt_ws_floats(2)
ENTRY_ARGS = {
    # name: (well-formed arguments, indices of pointers that must not be NULL, index of B)
    'ds2_conv_fwd': ([2, P, P, P, 2, 50, P, P, None], (1, 2, 3, 6, 7), 4),
    'ds2_conv2_dgrad': ([P, P, 2, 50, P, P, WS2, None], (0, 1, 4, 5), 2),
    'ds2_conv_wgrad': ([2, P, P, 2, 50, P, P, None], (1, 2, 5, 6), 3),
}


def _refused(name, args):
    from ds2hip import lib
    handle = lib.load()
    rc = getattr(handle, name)(*args)
    assert rc == lib.ERR_ARG, (name, args, rc)
    assert name.encode() in handle.ds2_last_error()


def _with(name, **kw):
    args = list(ENTRY_ARGS[name][0])
    for i, v in kw.items():
        args[int(i[1:])] = v
    return args


@pytest.mark.parametrize('name', sorted(ENTRY_ARGS))
def test_conv_entry_points_refuse_null_pointers_and_empty_batches(name):
    ok, pointers, ib = ENTRY_ARGS[name]
    for i in pointers:
        _refused(name, _with(name, **{'a%d' % i: None}))
    for bad in (0, -1):
        _refused(name, _with(name, **{'a%d' % ib: bad}))


@pytest.mark.parametrize('name', ['ds2_conv_fwd', 'ds2_conv_wgrad'])
def test_conv_entry_points_refuse_a_layer_outside_1_and_2(name):
    for which in (0, 3, -1):
        _refused(name, _with(name, a0=which))


@pytest.mark.parametrize('name,it', [('ds2_conv_fwd', 5), ('ds2_conv_wgrad', 4), ('ds2_conv2_dgrad', 3)])
def test_conv2_refuses_inputs_of_ten_frames_and_fewer(name, it):
    for t in (10, 1, 0, -5):
        _refused(name, _with(name, **{'a%d' % it: t}))


def test_conv2_dgrad_refuses_a_workspace_one_float_short():
    from ds2hip import lib
    assert lib.query('ds2_conv_wt_ws_floats', 2) == WS2
    _refused('ds2_conv2_dgrad', _with('ds2_conv2_dgrad', a6=WS2 - 1))


@pytest.mark.parametrize('name,it', [('ds2_conv_fwd', 5), ('ds2_conv_wgrad', 4)])
@pytest.mark.parametrize('t', range(-10, 1))
def test_conv1_refuses_zero_and_negative_frame_counts(name, it, t):
    """conv1's output length (t + 9) / 2 + 1 stays positive for t = -10 .. 0 under C's truncating division, and TIN * 4
    then made a buffer descriptor of negative -- enormous -- length: t_in_frames > 0 is checked on its own"""
    _refused(name, _with(name, a0=1, **{'a%d' % it: t}))
