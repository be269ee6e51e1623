"""The bidirectional GRU recurrence of include/ds2hip.h written out step by step on the CPU, with the library's own
interface: the tensors go in and come out in the layouts the C ABI defines, so a test compares them one to one.

Everything runs in the dtype of its inputs.  In float64 it is the reference the HIP recurrence forms are held to
(tests/test_gru_fp64_gpu.py); in float32 the SAME code is the yardstick: what correctly rounded fp32 arithmetic in another
summation order costs on the same inputs.  Nothing goes through autograd (tests/test_gru_ref_cpu.py checks the backward
against autograd in float64); each time step is one batched matmul over the two directions.

    gi     (T,B,2,3H)  input projections, gate order r,z,n; dir 0 forward, dir 1 reverse over the PADDED length
    w_hh   (2,3H,H)    recurrent weights, dir-major
    r = sigmoid(gi_r + gh_r); z = sigmoid(gi_z + gh_z); n = tanh(gi_n + r * gh_n); h' = (1 - z) * n + z * h; h_0 = 0
"""
import torch


def _step_time(s, t_len):
    """Time index of each direction at recurrence step s: (forward, reverse)."""
    return s, t_len - 1 - s


def gru_bidir_fwd(gi, w_hh):
    """ds2_gru_bidir_fwd: returns (rzn (T,B,2,3H), ghn (T,B,2,H), hout (2,T,B,H))."""
    t_len, b, _, h3 = gi.shape
    hid = h3 // 3
    w_t = w_hh.transpose(1, 2).contiguous()                       # (2,H,3H)
    rzn = torch.empty_like(gi)
    ghn = gi.new_empty(t_len, b, 2, hid)
    hout = gi.new_empty(2, t_len, b, hid)
    h = gi.new_zeros(2, b, hid)
    for s in range(t_len):
        tt = _step_time(s, t_len)
        g = torch.stack([gi[tt[0], :, 0], gi[tt[1], :, 1]], 0)    # (2,B,3H)
        gh = torch.bmm(h, w_t)
        r = torch.sigmoid(g[..., :hid] + gh[..., :hid])
        z = torch.sigmoid(g[..., hid:2 * hid] + gh[..., hid:2 * hid])
        gn = gh[..., 2 * hid:]
        n = torch.tanh(g[..., 2 * hid:] + r * gn)
        h = (1.0 - z) * n + z * h
        for d in (0, 1):
            rzn[tt[d], :, d, :hid] = r[d]
            rzn[tt[d], :, d, hid:2 * hid] = z[d]
            rzn[tt[d], :, d, 2 * hid:] = n[d]
            ghn[tt[d], :, d] = gn[d]
            hout[d, tt[d]] = h[d]
    return rzn, ghn, hout


def _h_prev(hout):
    """(T,B,2,H): the state each (t, direction) step started from (h_0 = 0)."""
    _, t_len, b, hid = hout.shape
    hp = hout.new_zeros(t_len, b, 2, hid)
    hp[1:, :, 0] = hout[0, :-1]
    hp[:-1, :, 1] = hout[1, 1:]
    return hp


def gru_bidir_bwd(rzn, ghn, hout, d_out, w_hh):
    """ds2_gru_bidir_bwd (BPTT; d_out (T,B,H) is the gradient w.r.t. the direction sum, so it feeds both directions).
    Returns (dgi (T,B,2,3H) = [dr_pre, dz_pre, dn_pre], dghn (T,B,2,H) = dn_pre * r, dh (T,B,2,H)), dh being the whole
    gradient that reaches h_t of each direction: d_out[t] plus what flows back from the step after it."""
    t_len, b, _, h3 = rzn.shape
    hid = h3 // 3
    hp_all = _h_prev(hout)
    dgi = torch.empty_like(rzn)
    dghn = torch.empty_like(ghn)
    dh_all = torch.empty_like(ghn)
    carry = rzn.new_zeros(2, b, hid)                              # d(h_t) from the later step of each direction
    for s in range(t_len - 1, -1, -1):
        tt = _step_time(s, t_len)
        sel = lambda x: torch.stack([x[tt[0], :, 0], x[tt[1], :, 1]], 0)
        g, gn, hp = sel(rzn), sel(ghn), sel(hp_all)
        r, z, n = g[..., :hid], g[..., hid:2 * hid], g[..., 2 * hid:]
        dh = torch.stack([d_out[tt[0]], d_out[tt[1]]], 0) + carry
        dn_pre = dh * (1.0 - z) * (1.0 - n * n)
        dz_pre = dh * (hp - n) * z * (1.0 - z)
        dr_pre = dn_pre * gn * r * (1.0 - r)
        dgn = dn_pre * r
        dgh = torch.cat([dr_pre, dz_pre, dgn], -1)                # (2,B,3H)
        carry = dh * z + torch.bmm(dgh, w_hh)
        for d in (0, 1):
            dgi[tt[d], :, d, :hid] = dr_pre[d]
            dgi[tt[d], :, d, hid:2 * hid] = dz_pre[d]
            dgi[tt[d], :, d, 2 * hid:] = dn_pre[d]
            dghn[tt[d], :, d] = dgn[d]
            dh_all[tt[d], :, d] = dh[d]
    return dgi, dghn, dh_all


def gru_bwd_coef(rzn, ghn, hout):
    """ds2_gru_bwd_coef: the (T,B,2,3H) coefficient planes (c_r | c_z | c_n) of the d(h)-hand-off backward recurrence,
    d(gh)_t[b, g, j] = dh_t[b, j] * c_g[t, b, j]:
        c_r = (1 - z)(1 - n^2) gh_n r (1 - r),   c_z = (h_prev - n) z (1 - z),   c_n = (1 - z)(1 - n^2) r"""
    hid = ghn.shape[-1]
    r, z, n = rzn[..., :hid], rzn[..., hid:2 * hid], rzn[..., 2 * hid:]
    an = (1.0 - z) * (1.0 - n * n)
    return torch.cat([an * ghn * r * (1.0 - r), (_h_prev(hout) - n) * z * (1.0 - z), an * r], -1)


def gru_dw_hh(dgi, dghn, hout):
    """(2,3H,H): the recurrent weights' gradient as the model forms it from the backward pass's outputs, dGH^T h_prev per
    direction with dGH = (dr_pre | dz_pre | d(gh_n))."""
    t_len, b, _, h3 = dgi.shape
    hid = h3 // 3
    dgh = torch.cat([dgi[..., :2 * hid], dghn], -1)               # (T,B,2,3H)
    hp = _h_prev(hout)
    return torch.stack([dgh[:, :, d].reshape(t_len * b, h3).t() @ hp[:, :, d].reshape(t_len * b, hid) for d in (0, 1)], 0)
