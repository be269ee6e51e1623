"""Every form of the bidirectional GRU recurrence against a float64 reference at the real width (H = 800).

The reference is oracle/gru.py, the recurrence written out on the CPU in float64 (tests/test_gru_ref_cpu.py ties it to torch
autograd and torch.nn.GRU in double).  The yardstick is the SAME code run in float32 on the same inputs: its error against
float64, e32, is what correctly rounded fp32 arithmetic in another summation order costs on exactly this input.  For every
output tensor of every form the test computes e64 (kernel against float64) and asserts e64 <= K * e32, as max-abs and as rms.
K is one number per tensor family, fixed from one measured run of all forms (profiles/gru_fp64_errors.md has the table and the
derivation: twice the worst measured ratio of the family, rounded up to a power of two); e32 never comes from a kernel.

What this file leaves to the agree-with-step tests of test_kernels_gpu.py: hand-off freshness over many repeated launches on
one workspace, launches beside other kernels, and the bounded spins.
"""
import pytest
import torch

from oracle import gru as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# gain, s: w_hh = gain * U(+-1/sqrt(H)), gi = s * N(0,1); d_out = 0.1 * N(0,1)
REGIMES = {'init': (1.0, 1.0),          # the distribution of the agree-with-step tests
           'trained': (4.0, 1.0),       # the recurrent term dominates, max|d(gi)| grows to ~1
           'saturated': (3.0, 3.0)}     # about a third of r / z within 0.05 of 0 or 1, |pre-activation| beyond 10
# (gain 6 is chaotic -- the fp32 and fp64 trajectories separate, the gradient overflows -- and must not be used)

# e64 <= K * e32, per tensor family: see profiles/gru_fp64_errors.md
K = {'fwd': 8.0, 'bwd': 8.0, 'dw': 16.0}
FAMILY = {'rzn': 'fwd', 'ghn': 'fwd', 'hout0': 'fwd', 'hout1': 'fwd', 'coef': 'fwd', 'dgi': 'bwd', 'dghn': 'bwd',
          'dw0': 'dw', 'dw1': 'dw'}
# Below this absolute size an error cannot be seen in float32 results of magnitude >= 1e-4 at all; it only keeps the ratio
# finite where the float32 restatement happens to be exact (e.g. gh_n of a first step, 0 on every side).
TINY = 1e-12
# A regime is usable only where the recurrence is well conditioned: the float32 restatement itself must stay this close
# to float64 (times max(1, max|ref|)), otherwise no bound on a kernel means anything.  A case that misses it FAILS.
CONDITION = 1e-5

SWITCHES = ('DS2_GRU_FWD', 'DS2_GRU_BWD', 'DS2_GRU_FWD_WIDE', 'DS2_GRU_P2_BF16', 'DS2_GRU_P2_BF16_BWD', 'DS2_GRU_BWD_DH')


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


def _errors(x, r64):
    """(max abs, rms) of x - r64, in float64 on r64's device."""
    e = x.to(r64.device, torch.float64) - r64
    if e.numel() == 0:
        return 0.0, 0.0
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


_refs = {}


def reference(t, bsz, hid, regime, dev=DEV):
    """Inputs (float32, on ``dev``), the float64 reference of every tensor (on ``dev``) and the float32 restatement's own
    errors e32 = {tensor: (max, rms)}.  Computed once per (T, B, H, regime) and shared by the forms."""
    key = (t, bsz, hid, regime)
    if key in _refs:
        return _refs[key]
    gain, s = REGIMES[regime]
    g = torch.Generator().manual_seed(1)
    k = 1.0 / hid ** 0.5
    w_hh = (torch.rand(2, 3 * hid, hid, generator=g) * 2 - 1) * (k * gain)
    gi = torch.randn(t, bsz, 2, 3 * hid, generator=g) * s
    d_out = torch.randn(t, bsz, hid, generator=g) * 0.1
    out = {}
    for dt in (torch.float64, torch.float32):
        w, x, dy = w_hh.to(dt), gi.to(dt), d_out.to(dt)
        rzn, ghn, hout = ref.gru_bidir_fwd(x, w)
        coef = ref.gru_bwd_coef(rzn, ghn, hout)
        dgi, dghn, _ = ref.gru_bidir_bwd(rzn, ghn, hout, dy, w)
        dw = ref.gru_dw_hh(dgi, dghn, hout)
        out[dt] = {'rzn': rzn, 'ghn': ghn, 'hout0': hout[0], 'hout1': hout[1], 'coef': coef, 'dgi': dgi, 'dghn': dghn,
                   'dw0': dw[0], 'dw1': dw[1]}
    r64 = {name: v.to(dev) for name, v in out[torch.float64].items()}
    e32 = {name: _errors(out[torch.float32][name], r64[name]) for name in r64}
    scale = {name: max(1.0, float(v.abs().max())) for name, v in r64.items()}
    _refs[key] = {'w_hh': w_hh.to(dev), 'gi': gi.to(dev), 'd_out': d_out.to(dev), 'r64': r64, 'e32': e32, 'scale': scale}
    return _refs[key]


class _Table:
    """Rows (form, regime, tensor, e64, e32, ratio as max and rms), printed as they are measured; the bound is asserted at the
    end of the case so that one run shows every figure of it."""

    def __init__(self, form, regime, case):
        self.form, self.regime, self.case, self.bad = form, regime, case, []

    def add(self, variant, name, got):
        r64, (m32, s32) = self.case['r64'][name], self.case['e32'][name]
        m64, s64 = _errors(got, r64)
        rm, rs = m64 / max(m32, TINY), s64 / max(s32, TINY)
        form = self.form + ('/' + variant if variant else '')
        print('GRUFP64|%s|%s|%s|%.3e|%.3e|%.2f|%.3e|%.3e|%.2f' % (form, self.regime, name, m64, m32, rm, s64, s32, rs))
        if m32 >= CONDITION * self.case['scale'][name]:
            self.bad.append('BAD CASE %s %s %s: the float32 restatement itself is off by %.3e' % (form, self.regime, name, m32))
        bound = K[FAMILY[name]]
        if not (rm <= bound and rs <= bound):
            self.bad.append('%s %s %s: e64 / e32 = %.2f (max: %.3e / %.3e), %.2f (rms: %.3e / %.3e) > K = %g'
                            % (form, self.regime, name, rm, m64, m32, rs, s64, s32, bound))


def _dw_hh(ops, dgi, dghn, hout, t, bsz, hid):
    """dW_hh of both directions from the kernel's outputs, through ops.gemm as the model and test_gru_recurrence_fwd_bwd form
    it: dGH[1:]^T h[:-1] (forward direction), dGH[:-1]^T h[1:] (reverse)."""
    rows = (t - 1) * bsz
    dgh0 = torch.cat([dgi[1:, :, 0, :2 * hid], dghn[1:, :, 0, :]], -1).reshape(rows, 3 * hid).contiguous()
    dgh1 = torch.cat([dgi[:-1, :, 1, :2 * hid], dghn[:-1, :, 1, :]], -1).reshape(rows, 3 * hid).contiguous()
    return (ops.gemm(dgh0, hout[0, :-1].reshape(rows, hid).contiguous(), trans_a=True),
            ops.gemm(dgh1, hout[1, 1:].reshape(rows, hid).contiguous(), trans_a=True))


def run_case(ops, monkeypatch, form, regime, mode, t, bsz, hid, env=(), dh='model', spare_cus=(-1,)):
    """One forward launch and one backward launch per (spare_cus, planes) variant of one form on one input.
    ``dh``: 'model' = what codes/model.py does (ask the forward pass for the planes; the d(h) hand-off runs where
    ops.gru_bwd_dh_wanted says so), 'off' = DS2_GRU_BWD_DH=0 (the d(gh)-hand-off forms), 'on' = DS2_GRU_BWD_DH=1, each
    backward variant run with the forward launch's own planes and with ops.gru_bwd_coef's."""
    case = reference(t, bsz, hid, regime)
    table = _Table(form, regime, case)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    if dh != 'model':
        monkeypatch.setenv('DS2_GRU_BWD_DH', '1' if dh == 'on' else '0')
    monkeypatch.setattr(ops, 'GRU_MODE', mode)
    w_hh, d_out = case['w_hh'], case['d_out']
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    wanted = ops.gru_bwd_dh_wanted(w_hh.device, bsz, hid)
    if dh == 'on':
        assert wanted
    elif dh == 'off' or mode == 'step':
        assert not wanted
    elif hid == 800:
        assert wanted == (9 <= bsz <= 12)           # B = 9 .. 12 trains through the d(h) hand-off whatever DS2_GRU_BWD says
    g = case['gi'].clone()
    ghn, hout, coef = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid, want_coef=True)
    torch.cuda.synchronize()
    ops.check_async_errors()
    assert (coef is not None) == wanted
    table.add('', 'rzn', g)
    table.add('', 'ghn', ghn)
    table.add('', 'hout0', hout[0])
    table.add('', 'hout1', hout[1])
    planes = [('', None)]
    if wanted:
        table.add('own planes', 'coef', coef)
        planes = [('own planes', coef)]
        if dh == 'on':
            again = ops.gru_bwd_coef(g, ghn, hout, t, bsz, hid)
            table.add('gru_bwd_coef', 'coef', again)
            planes.append(('gru_bwd_coef', again))
    for spare in spare_cus:
        for label, c in planes:
            variant = ', '.join(x for x in ('spare_cus=%d' % spare if spare >= 0 else '', label) if x)
            dgi, dghn = g.clone(), ghn.clone()          # the backward launch overwrites r,z,n and gh_n
            ops.gru_bidir_bwd(dgi, dghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=spare, coef=c)
            torch.cuda.synchronize()
            ops.check_async_errors()
            table.add(variant, 'dgi', dgi)
            table.add(variant, 'dghn', dghn)
            if t > 1:
                dw0, dw1 = _dw_hh(ops, dgi, dghn, hout, t, bsz, hid)
                torch.cuda.synchronize()
                table.add(variant, 'dw0', dw0)
                table.add(variant, 'dw1', dw1)
    if mode == 'persistent':
        assert not ops._persistent_off              # no launch fell back to the launch-per-step kernels
    assert not table.bad, '\n'.join(table.bad)


ALL = ('init', 'trained', 'saturated')
LONG, SHORT = 746, 128


def _cases():
    c = []

    def add(form, mode, t, bsz, hid=800, regimes=('trained',), **kw):
        for regime in regimes:
            c.append(pytest.param(form, regime, mode, t, bsz, hid, kw, id='%s-%s' % (form.replace(' ', '_'), regime)))

    # the launch-per-step kernels: every agree-with-step test inherits from them
    add('step B=10', 'step', LONG, 10, regimes=ALL)
    add('step B=32', 'step', SHORT, 32)
    add('step B=5 H=72', 'step', 33, 5, hid=72)
    # the forms the batch size selects by default, driven as codes/model.py drives them
    for bsz in (4, 8, 10, 12, 13, 16, 17, 32, 64):
        add('default B=%d' % bsz, 'persistent', LONG if bsz == 10 else SHORT, bsz, regimes=ALL if bsz == 10 else ('trained',))
    # both MFMA forms of each persistent kernel, forced (the d(gh) hand-off: B = 9 .. 12 would run the d(h) form otherwise)
    for bsz in (10, 32):
        for f in ('4', '16'):
            add('FWD=%s BWD=%s B=%d' % (f, f, bsz), 'persistent', SHORT, bsz, env=(('DS2_GRU_FWD', f), ('DS2_GRU_BWD', f)), dh='off')
    add('FWD_WIDE=0 B=10', 'persistent', LONG, 10, env=(('DS2_GRU_FWD_WIDE', '0'),))
    # the two-part forms in the f32 and the split-operand bf16 family
    for bsz in (17, 32, 64):
        for v in ('0', '1'):
            add('P2_BF16=%s P2_BF16_BWD=%s B=%d' % (v, v, bsz), 'persistent', LONG if bsz == 32 else SHORT, bsz,
                env=(('DS2_GRU_P2_BF16', v), ('DS2_GRU_P2_BF16_BWD', v)))
    # the three-part d(gh)-hand-off backward kernel with 20 / 24 / 28 hidden units per workgroup
    for bsz in (9, 10, 12):
        add('d(gh) B=%d' % bsz, 'persistent', SHORT, bsz, dh='off', spare_cus=(0, 52, 82))
    # the d(h)-hand-off backward kernel, with the forward launch's planes and with the elementwise pass's
    for bsz in (5, 8, 9, 10, 12):
        add('d(h) B=%d' % bsz, 'persistent', SHORT, bsz, dh='on', spare_cus=(0, 52, 82) if bsz >= 9 else (-1,))
    # ... and where it peels its first step: T = 1, 2, an odd length, and the narrow width
    add('d(h) T=1 B=10', 'persistent', 1, 10, dh='on', spare_cus=(0, 82))
    add('d(h) T=2 B=9', 'persistent', 2, 9, dh='on', spare_cus=(0, 82))
    add('d(h) T=33 B=8', 'persistent', 33, 8, dh='on')
    add('d(h) T=7 B=12 H=64', 'persistent', 7, 12, hid=64, dh='on', spare_cus=(0, 82))
    add('d(h) T=33 B=5 H=64', 'persistent', 33, 5, hid=64, dh='on')
    return c


@pytest.mark.parametrize('form,regime,mode,t,bsz,hid,kw', _cases())
def test_gru_form_against_fp64(ops, monkeypatch, form, regime, mode, t, bsz, hid, kw):
    run_case(ops, monkeypatch, form, regime, mode, t, bsz, hid, **kw)
