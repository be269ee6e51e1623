"""oracle/gru.py (the written-out bidirectional GRU recurrence the HIP forms are held to in tests/test_gru_fp64_gpu.py)
against torch itself, all in float64: both sides differ in summation order only."""
import pytest
import torch

from oracle import gru as ref

RTOL = 1e-12


def _close(a, b):
    scale = max(float(b.abs().max()), 1.0)
    assert float((a - b).abs().max()) <= RTOL * scale


def _inputs(t, bsz, hid, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / hid ** 0.5
    w_hh = (torch.rand(2, 3 * hid, hid, generator=g, dtype=torch.float64) * 2 - 1) * k * 2.0
    gi = torch.randn(t, bsz, 2, 3 * hid, generator=g, dtype=torch.float64)
    d_out = torch.randn(t, bsz, hid, generator=g, dtype=torch.float64)
    return gi, w_hh, d_out


def _autograd_forward(gi, w_hh):
    """The same recurrence through torch ops that autograd records: the direction sum (T,B,H)."""
    t_len, _, _, h3 = gi.shape
    hid = h3 // 3
    outs = []
    for d in (0, 1):
        h = torch.zeros(gi.shape[1], hid, dtype=gi.dtype)
        hs = [None] * t_len
        for t in (range(t_len) if d == 0 else range(t_len - 1, -1, -1)):
            gh = h @ w_hh[d].t()
            r = torch.sigmoid(gi[t, :, d, :hid] + gh[:, :hid])
            z = torch.sigmoid(gi[t, :, d, hid:2 * hid] + gh[:, hid:2 * hid])
            n = torch.tanh(gi[t, :, d, 2 * hid:] + r * gh[:, 2 * hid:])
            h = (1.0 - z) * n + z * h
            hs[t] = h
        outs.append(torch.stack(hs, 0))
    return outs[0] + outs[1]


CASES = [(t, bsz, hid) for t in (1, 2, 7) for bsz in (1, 3) for hid in (8, 24)]


@pytest.mark.parametrize('t,bsz,hid', CASES)
def test_written_out_backward_equals_autograd_in_double(t, bsz, hid):
    gi, w_hh, d_out = _inputs(t, bsz, hid, 100 * t + 10 * bsz + hid)
    rzn, ghn, hout = ref.gru_bidir_fwd(gi, w_hh)
    dgi, dghn, _ = ref.gru_bidir_bwd(rzn, ghn, hout, d_out, w_hh)
    dw = ref.gru_dw_hh(dgi, dghn, hout)
    gi_a, w_a = gi.clone().requires_grad_(True), w_hh.clone().requires_grad_(True)
    ysum = _autograd_forward(gi_a, w_a)
    _close(hout[0] + hout[1], ysum.detach())
    ysum.backward(d_out)
    _close(dgi, gi_a.grad)                       # both directions: d(gi)[:, :, 0] and [:, :, 1]
    _close(dw, w_a.grad)
    # d(gh_n) = dn_pre * r, by its definition in include/ds2hip.h
    _close(dghn, dgi[..., 2 * hid:] * rzn[..., :hid])


@pytest.mark.parametrize('t,bsz,hid', CASES)
def test_forward_equals_torch_gru_in_double(t, bsz, hid):
    torch.manual_seed(t + bsz + hid)
    n_in = 5
    gru = torch.nn.GRU(n_in, hid, bias=False, bidirectional=True).double()
    x = torch.randn(t, bsz, n_in, dtype=torch.float64)
    with torch.no_grad():
        y, _ = gru(x)
        w_ih = torch.cat([gru.weight_ih_l0, gru.weight_ih_l0_reverse], 0)              # (6H, In)
        w_hh = torch.stack([gru.weight_hh_l0, gru.weight_hh_l0_reverse], 0)
        gi = (x.reshape(t * bsz, n_in) @ w_ih.t()).reshape(t, bsz, 2, 3 * hid)
        rzn, ghn, hout = ref.gru_bidir_fwd(gi, w_hh)
    _close(hout[0], y[:, :, :hid])
    _close(hout[1], y[:, :, hid:])
    # the saved tensors against the explicit one-direction restatement
    from oracle.model import gru_direction_explicit
    for d, (wi, wh) in enumerate(((gru.weight_ih_l0, gru.weight_hh_l0), (gru.weight_ih_l0_reverse, gru.weight_hh_l0_reverse))):
        sv = gru_direction_explicit(x, wi.detach(), wh.detach(), reverse=d == 1)
        _close(rzn[:, :, d, :hid], sv['r'])
        _close(rzn[:, :, d, hid:2 * hid], sv['z'])
        _close(rzn[:, :, d, 2 * hid:], sv['n'])
        _close(ghn[:, :, d], sv['ghn'])


@pytest.mark.parametrize('t,bsz,hid', CASES)
def test_coefficient_planes_satisfy_their_identity(t, bsz, hid):
    """d(gh)_t = dh_t * c_g[t] for the three planes, dh_t being the whole gradient that reaches h_t."""
    gi, w_hh, d_out = _inputs(t, bsz, hid, 7 * t + bsz + hid)
    rzn, ghn, hout = ref.gru_bidir_fwd(gi, w_hh)
    dgi, dghn, dh = ref.gru_bidir_bwd(rzn, ghn, hout, d_out, w_hh)
    coef = ref.gru_bwd_coef(rzn, ghn, hout)
    assert coef.shape == (t, bsz, 2, 3 * hid)
    _close(dh * coef[..., :hid], dgi[..., :hid])
    _close(dh * coef[..., hid:2 * hid], dgi[..., hid:2 * hid])
    _close(dh * coef[..., 2 * hid:], dghn)
    # dh itself: the last step of each direction sees d_out alone
    _close(dh[t - 1, :, 0], d_out[t - 1])
    _close(dh[0, :, 1], d_out[0])


def test_float32_runs_the_same_code():
    gi, w_hh, d_out = _inputs(7, 3, 24, 5)
    r64 = ref.gru_bidir_fwd(gi, w_hh)
    r32 = ref.gru_bidir_fwd(gi.float(), w_hh.float())
    for a, b in zip(r32, r64):
        assert a.dtype == torch.float32 and float((a.double() - b).abs().max()) < 1e-5
    b32 = ref.gru_bidir_bwd(*r32, d_out.float(), w_hh.float())
    b64 = ref.gru_bidir_bwd(*r64, d_out, w_hh)
    for a, b in zip(b32, b64):
        assert a.dtype == torch.float32 and float((a.double() - b).abs().max()) < 1e-5
