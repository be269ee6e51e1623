"""Per-kernel parity of the HIP path (through the C ABI) against the CPU oracle.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------- GEMM
@pytest.fixture
def gemm_family(ops, request):
    """Kernel family of ds2_gemm_f32 for one test (0: f32-input MFMA, 6 / 9: bf16 split-operand kernels)."""
    before = ops.gemm_split_mode()
    assert ops.gemm_split_mode(request.param) == request.param
    yield request.param
    ops.gemm_split_mode(before)


@pytest.mark.parametrize('gemm_family', [0, 6], indirect=True)
@pytest.mark.parametrize('ta,tb', [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize('m,n,k', [(128, 128, 16), (300, 200, 100), (37, 29, 800), (1000, 4800, 672),
                                   (29, 800, 555), (5, 7, 3), (257, 129, 33),
                                   (4240, 4800, 800), (3001, 2999, 301), (2100, 4000, 17), (8200, 4100, 40),
                                   (1330, 800, 4800), (260, 192, 2100)])     # edge tiles of 32 / 64 columns + split-K
def test_gemm_matches_fp64(ops, gemm_family, ta, tb, m, n, k):
    rng = np.random.default_rng(m * 7 + n * 3 + k + ta * 2 + tb)
    a = rng.standard_normal((k, m) if ta else (m, k)).astype(np.float32)
    b = rng.standard_normal((n, k) if tb else (k, n)).astype(np.float32)
    ref = (a.T if ta else a).astype(np.float64) @ (b.T if tb else b).astype(np.float64)
    out = ops.gemm(_t(a), _t(b), trans_a=bool(ta), trans_b=bool(tb)).cpu().numpy()
    # fp32 accumulation noise: rounding of partial sums whose magnitude grows like sqrt(k), over k terms (outputs ~ sqrt(k))
    np.testing.assert_allclose(out, ref, rtol=0, atol=max(8e-6 * np.sqrt(k), 4e-7 * k))


@pytest.mark.parametrize('ta,tb,m,n,k,split_k', [(0, 1, 1000, 800, 672, 1), (0, 0, 1111, 800, 4800, 1), (1, 0, 4800, 800, 3001, 1),
                                                 (1, 0, 1600, 800, 4240, 0), (1, 1, 384, 256, 512, 1), (0, 1, 512, 512, 2048, 1)])
def test_gemm_split_operand_kernels_are_as_accurate_as_the_f32_kernels(ops, ta, tb, m, n, k, split_k):
    """ds2_gemm_f32's default kernels multiply on the bf16 matrix pipe after an error-free three-way split of every fp32
    operand (include/ds2hip.h).  Error against an fp64 product, relative to sum_k |a||b| (the scale fp32 rounding errors
    are proportional to), for the f32-input kernels (mode 0), the six-product kernels (6, the default) and the
    nine-product kernels (9): the split kernels must be no worse than mode 0 -- on operands of order one and on operands
    whose magnitudes spread over e^(+-24) (the last shape), where a dropped low-order product would show."""
    torch.manual_seed(m + k)
    a = torch.randn((k, m) if ta else (m, k), device=DEV)
    b = torch.randn((n, k) if tb else (k, n), device=DEV)
    if k == 2048:
        a = a * torch.exp(8 * torch.randn_like(a))
        b = b * torch.exp(8 * torch.randn_like(b))
    a64, b64 = (a.t() if ta else a).double(), (b.t() if tb else b).double()
    ref, scale = a64 @ b64, a64.abs() @ b64.abs()
    before = ops.gemm_split_mode()
    err = {}
    try:
        for mode in (0, 6, 9):
            ops.gemm_split_mode(mode)
            c = ops.gemm(a, b, trans_a=bool(ta), trans_b=bool(tb), split_k=split_k)
            e = (c.double() - ref).abs() / scale
            err[mode] = (float(e.max()), float(e.pow(2).mean().sqrt()))
    finally:
        ops.gemm_split_mode(before)
    for mode in (6, 9):
        assert err[mode][0] <= 1.25 * err[0][0] + 1e-8, err            # max
        assert err[mode][1] <= 1.25 * err[0][1] + 1e-9, err            # rms
    assert err[6][0] <= 3e-6 and err[0][0] <= 3e-6, err               # and all of them are fp32-grade in absolute terms


def test_gemm_six_products_adversarial_aligned_residuals(ops):
    """The six-product family leaves out a2 b3 + a3 b2 + a3 b3 of every product.  The WORST case for it: both residual
    terms of every operand element as large as round-to-nearest allows and of the SAME sign along the whole of k, so that
    what is left out adds up instead of averaging out -- at the model's deepest contraction, K = 4800 (the dX GEMM).
    Element pattern: 1.m + 0.1111111|0|111111 (binary, at 2^-8): a1 = 1.m, a2 = +(2^-8 - 2^-16) (99.6 % of half an ulp of
    a1), a3 = +(2^-17 - 2^-23); every product then misses 2 a2 a3 + a3^2 ~ 2^-24 of itself, all with one sign.
    What the case showed when it was first run (round 4): the dropped products are invisible -- the nine-product family, which
    leaves nothing out, had exactly the six-product family's error -- but fp32 ACCUMULATION is not: with one accumulator per
    output the small partial products (a1 b3, a3 b1: 2^-16 of a term) were rounded away against a running sum of ~10^4, every
    time: 1.8e-5 of the result lost, against 7.5e-6 for the f32-input kernels (whose own accumulation of 4800 same-sign terms
    is biased too).  Since then the residual-carrying products have an accumulator of their own (split_bf16.h::split_mfma2):
    1.5e-6.  Asserted: six == nine (the dropped terms stay below everything else), and the split families are no worse than
    the f32-input kernels on their worst case."""
    k, m, n = 4800, 256, 256
    rng = np.random.default_rng(9)
    resid = (2.0 ** -8 - 2.0 ** -16) + (2.0 ** -17 - 2.0 ** -23)     # 0.1111111|0|111111 at 2^-8: a2 rounds DOWN, a3 > 0

    def operand(rows):
        lead = 1.0 + rng.integers(0, 128, size=(rows, k)) / 128.0          # a1: any 8-bit significand in [1, 2)
        v = (lead + resid).astype(np.float32)
        assert np.array_equal(v.astype(np.float64), lead + resid)            # exactly representable: the pattern is what is fed
        return v
    a, b = operand(m), operand(n)
    # the split the kernels perform (round to nearest even, three times) leaves residuals of one sign, as intended
    a1 = _t(a).bfloat16().float().cpu().numpy()
    a2 = _t(a - a1).bfloat16().float().cpu().numpy()
    a3 = a - a1 - a2
    assert (a2 > 0).all() and (a3 > 0).all() and float(a2.min()) > 0.99 * 2.0 ** -8 and float(a3.min()) > 0.49 * 2.0 ** -16
    ref = a.astype(np.float64) @ b.astype(np.float64).T                       # all terms positive: scale = ref
    before = ops.gemm_split_mode()
    err = {}
    try:
        for mode in (0, 6, 9):
            ops.gemm_split_mode(mode)
            c = ops.gemm(_t(a), _t(b), trans_b=True, split_k=1).cpu().numpy().astype(np.float64)
            err[mode] = float((np.abs(c - ref) / ref).max())
    finally:
        ops.gemm_split_mode(before)
    assert abs(err[6] - err[9]) <= 2.0 ** -23, err                    # what six products leave out: at most its stated bound
    assert err[6] <= err[0] + 2.0 ** -24 and err[9] <= err[0] + 2.0 ** -24, err
    assert err[6] <= 4e-6, err                                        # (1.5e-6 measured; 1.8e-5 with a single accumulator)


@pytest.mark.parametrize('gemm_family', [0, 6, 9], indirect=True)
def test_gemm_exact_on_small_integers(ops, gemm_family):
    """Integer operands whose products and sums fit 24 bits: every family must return the exact result (the split terms
    carry all 24 bits of an operand, the partial products are exact)."""
    rng = np.random.default_rng(5)
    a = rng.integers(-2047, 2048, size=(256, 64)).astype(np.float32)
    b = rng.integers(-63, 64, size=(192, 64)).astype(np.float32)
    out = ops.gemm(_t(a), _t(b), trans_b=True).cpu().numpy()
    assert np.array_equal(out, a.astype(np.int64) @ b.astype(np.int64).T)
    a[3, 5] = 16777215.0                                               # all 24 bits set: needs all three terms
    b[:, 5] = 0.0
    b[7, 5] = 1.0
    a[3, :5] = 0.0
    a[3, 6:] = 0.0
    out = ops.gemm(_t(a), _t(b), trans_b=True).cpu().numpy()
    assert out[3, 7] == 16777215.0


def test_gemm_beta_and_splitk(ops):
    rng = np.random.default_rng(1)
    a = rng.standard_normal((5000, 96)).astype(np.float32)      # stored K x M (trans_a)
    b = rng.standard_normal((5000, 200)).astype(np.float32)
    c0 = rng.standard_normal((96, 200)).astype(np.float32)
    ref = a.astype(np.float64).T @ b.astype(np.float64) + c0
    c = _t(c0.copy())
    ops.gemm(_t(a), _t(b), trans_a=True, out=c, beta=1.0)
    np.testing.assert_allclose(c.cpu().numpy(), ref, atol=1e-3)
    c = _t(c0.copy())
    ops.gemm(_t(a), _t(b), trans_a=True, out=c, beta=1.0, split_k=4)
    np.testing.assert_allclose(c.cpu().numpy(), ref, atol=1e-3)


def test_gemm_identity_asymmetric(ops):
    # A = I with an asymmetric B catches a transposed C write
    b = np.arange(64 * 96, dtype=np.float32).reshape(64, 96)
    out = ops.gemm(_t(np.eye(64, dtype=np.float32)), _t(b)).cpu().numpy()
    assert np.array_equal(out, b)
    out = ops.gemm(_t(b), _t(np.eye(96, dtype=np.float32))).cpu().numpy()
    assert np.array_equal(out, b)


def test_gemm_strided_views(ops):
    rng = np.random.default_rng(2)
    big_a = rng.standard_normal((50, 48)).astype(np.float32)   # use columns 8..23 (lda = 48)
    b = rng.standard_normal((40, 16)).astype(np.float32)
    ta_, tb_ = _t(big_a), _t(b)
    out = torch.zeros(50, 40, device=DEV)
    ops.gemm_raw(0, 1, 50, 40, 16, ta_.data_ptr() + 8 * 4, 48, tb_.data_ptr(), 16, out.data_ptr(), 40)
    ref = big_a[:, 8:24].astype(np.float64) @ b.astype(np.float64).T
    np.testing.assert_allclose(out.cpu().numpy(), ref, atol=1e-4)


# ------------------------------------------------------------------------------------------- misc
def test_transposes(ops):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 77, 161)).astype(np.float32)
    assert np.array_equal(ops.transpose_btf(_t(x)).cpu().numpy(), x.transpose(0, 2, 1))
    y = rng.standard_normal((45, 1000)).astype(np.float32)
    assert np.array_equal(ops.transpose2d(_t(y), 45, 1000).cpu().numpy(), y.T)


def test_softmax_argmax_collapse(ops):
    from oracle import host
    rng = np.random.default_rng(4)
    for a in (29, 43):
        x = rng.standard_normal((301, a)).astype(np.float32)
        x[5, 3] = x[5, 9] = 10.0                         # a tie -> lowest index
        ref = torch.softmax(torch.from_numpy(x), -1).numpy()
        np.testing.assert_allclose(ops.softmax_rows(_t(x), 301, a).cpu().numpy(), ref, atol=1e-6)
        assert np.array_equal(ops.argmax_rows(_t(x), 301, a).cpu().numpy(), x.argmax(1))
    labels = ['_'] + [chr(65 + i) for i in range(28)]
    probs = rng.random((4, 150, 29)).astype(np.float32)
    probs[:, :, 0] += 0.4                                # plenty of blanks
    probs[1, 10:20, 5] = 9.0                             # a run of repeats
    sizes = np.asarray([150, 97, 1, 0], dtype=np.int32)
    best = ops.argmax_rows(_t(probs.reshape(-1, 29)), 600, 29).reshape(4, 150)
    ids, offs, lens = ops.greedy_collapse(best, _t(sizes))
    strings, offsets = host.greedy_decode(probs, sizes, labels)
    for b in range(4):
        n = int(lens[b])
        got = ''.join(labels[i] for i in ids[b, :n].cpu().numpy())
        assert got == strings[b]
        assert np.array_equal(offs[b, :n].cpu().numpy(), offsets[b])


# ------------------------------------------------------------------------------------------- frontend
def test_spectrogram_matches_oracle(ops):
    from oracle import spectrogram as ospec
    rng = np.random.default_rng(5)
    lens = [16000, 37923, 24000, 161, 16159]
    wavs = [np.clip(0.1 * rng.standard_normal(n), -1, 1).astype(np.float32) for n in lens]
    ref, pct = ospec.batch_log_spectrogram(wavs)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = ops.spectrogram(_t(np.concatenate(wavs)), _t(offs), ref.shape[1]).cpu().numpy()
    assert out.shape == ref.shape
    np.testing.assert_allclose(out, ref, rtol=0, atol=2e-4)
    # un-normalised log-magnitudes too
    raw = ops.spectrogram(_t(wavs[0]), _t(np.asarray([0, lens[0]], np.int64)), 101, normalize=False).cpu().numpy()[0]
    np.testing.assert_allclose(raw, np.log1p(ospec.stft_magnitude(wavs[0])), atol=2e-5)


# ------------------------------------------------------------------------------------------- conv
def _conv_ref(which, x, w, b):
    if which == 1:
        return F.conv2d(x, w, b, stride=(2, 2), padding=(0, 10))
    return F.conv2d(x, w, b, stride=(2, 1))


@pytest.mark.parametrize('which,bsz,t_in,form', [(1, 2, 121, '0'), (1, 3, 64, '0'), (2, 2, 66, '0'), (2, 1, 43, '0'),
                                                 (1, 1, 301, '0'), (2, 3, 139, '0'),
                                                 (2, 2, 66, 'dgrad-split'), (2, 3, 139, 'dgrad-split'), (2, 1, 43, 'dgrad-split'),
                                                 (2, 4, 301, 'dgrad-split'), (2, 1, 1060, 'dgrad-split')])
def test_conv_fwd_bwd(ops, monkeypatch, which, bsz, t_in, form):
    """('dgrad-split': the data gradient through the gather kernel on the bf16 matrix pipe, csrc/conv_split.hip, which the
    forward pass uses by default.  The direct forward kernel is covered by test_conv2_forward_families_agree.
    B = 1, t1 = 1060: the even-row launch (31 rows) has 1024+ waves and does not split K, the odd-row launch (30 rows) has
    fewer and does -- the output's one zero fill must precede BOTH (round 3's second launch wiped the first one's rows).)"""
    if form == 'dgrad-split':
        monkeypatch.setenv('DS2_CONV_SPLIT_DGRAD', '1')
    rng = np.random.default_rng(10 * which + bsz)
    cin, fin, kf = (1, 161, 41) if which == 1 else (32, 61, 21)
    x = torch.from_numpy(rng.standard_normal((bsz, cin, fin, t_in)).astype(np.float32)).requires_grad_(True)
    w = torch.from_numpy((rng.standard_normal((32, cin, kf, 11)) / np.sqrt(cin * kf * 11)).astype(np.float32))
    w.requires_grad_(True)
    b = torch.from_numpy(rng.standard_normal(32).astype(np.float32)).requires_grad_(True)
    ref = _conv_ref(which, x, w, b)
    dy = torch.from_numpy(rng.standard_normal(tuple(ref.shape)).astype(np.float32))
    ref.backward(dy)
    out = ops.conv_fwd(which, x.detach().to(DEV).contiguous().view(bsz, cin * fin, t_in) if which == 1
                       else x.detach().to(DEV), w.detach().to(DEV), b.detach().to(DEV), t_in)
    np.testing.assert_allclose(out.cpu().numpy(), ref.detach().numpy(), atol=2e-5)
    dw = torch.empty_like(w, device=DEV)
    db = torch.empty(32, device=DEV)
    ops.conv_wgrad(which, x.detach().to(DEV), dy.to(DEV), t_in, dw, db)
    np.testing.assert_allclose(dw.cpu().numpy(), w.grad.numpy(), rtol=1e-4, atol=1e-5 * float(w.grad.abs().max()) + 2e-4)
    np.testing.assert_allclose(db.cpu().numpy(), b.grad.numpy(), rtol=1e-4, atol=2e-4)
    if which == 2:
        dx = ops.conv2_dgrad(dy.to(DEV), w.detach().to(DEV), t_in)
        np.testing.assert_allclose(dx.cpu().numpy(), x.grad.numpy(), atol=2e-5)


@pytest.mark.parametrize('bsz,t1', [(12, 90), (10, 415), (3, 500), (1, 1060)])
def test_conv2_dgrad_row_walk_and_single_launch_hold_the_plain_walks_bits(ops, monkeypatch, bsz, t1):
    """Round 5: a workgroup of the gather data gradient walks only the tap groups whose filter rows reach an output row from
    its input rows, and both input-row parities run in one launch (csrc/conv_split.hip).  What is skipped are products with
    the zero border, so the result must equal the plain walk's (every group, two launches) BIT FOR BIT -- at shapes where
    the launch does not split K (12 x 90: a tile of 128 positions spans two or three input rows; 10 x 415: the bench's mean
    bin; 1 x 1060: one parity splits K, so the two-launch path with one row-walking launch) -- and F.conv2d's gradient."""
    monkeypatch.setenv('DS2_CONV_SPLIT_DGRAD', '1')
    rng = np.random.default_rng(bsz * 1000 + t1)
    w = torch.from_numpy((rng.standard_normal((32, 32, 21, 11)) / np.sqrt(32 * 21 * 11)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((bsz, 32, 21, t1 - 10)).astype(np.float32))
    got = ops.conv2_dgrad(dy.to(DEV), w.to(DEV), t1).cpu()
    monkeypatch.setenv('DS2_CONV_DGRAD_ROWS', '0')
    monkeypatch.setenv('DS2_CONV_DGRAD_MERGE', '0')
    plain = ops.conv2_dgrad(dy.to(DEV), w.to(DEV), t1).cpu()
    if (bsz, t1) != (1, 1060):                       # (float atomics where K is split: not bitwise reproducible)
        assert torch.equal(got, plain)
    else:
        np.testing.assert_allclose(got.numpy(), plain.numpy(), atol=2e-6)
    x = torch.zeros(bsz, 32, 61, t1, requires_grad=True)
    F.conv2d(x, w, None, stride=(2, 1)).backward(dy)
    np.testing.assert_allclose(got.numpy(), x.grad.numpy(), atol=2e-5)


def test_conv2_dgrad_workspace_contract(ops, monkeypatch):
    """ds2_conv2_dgrad takes the SIZE of its workspace (ABI revision 400): with the filter-layout size only it must run the
    direct kernel -- not write its gather form's zero-bordered copy of d_out past the end -- and with less than that return
    DS2_ERR_ARG; both answers are the same numbers as with the full workspace."""
    from ds2hip import lib
    monkeypatch.setenv('DS2_CONV_SPLIT_DGRAD', '1')                       # the gather form whenever there is room for it
    torch.manual_seed(2)
    bsz, t1 = 3, 139
    dy = torch.randn(bsz, 32, 21, t1 - 10, device=DEV)
    w = torch.randn(32, 32, 21, 11, device=DEV) / np.sqrt(32 * 21 * 11)
    full = ops.conv2_dgrad(dy, w, t1)
    small_n = lib.query('ds2_conv_wt_ws_floats', 2)
    assert small_n < lib.query('ds2_conv2_dgrad_ws_floats', bsz, t1)
    guard = 4096
    ws = torch.full((small_n + guard,), 7.0, device=DEV)
    d_in = torch.empty(bsz, 32, 61, t1, device=DEV)
    lib.call('ds2_conv2_dgrad', dy, w, bsz, t1, d_in, ws, small_n)
    torch.cuda.synchronize()
    assert bool((ws[small_n:] == 7.0).all()), 'wrote past the workspace it was given'
    np.testing.assert_allclose(d_in.cpu().numpy(), full.cpu().numpy(), atol=2e-5)
    with pytest.raises(lib.Ds2Error) as ei:
        lib.call('ds2_conv2_dgrad', dy, w, bsz, t1, d_in, ws, small_n - 1)
    assert ei.value.code == lib.ERR_ARG


def test_conv2_wgrad_lds_form_repeatable_at_training_size(ops, monkeypatch):
    """The operands-through-LDS weight-gradient kernel against the direct one at a training shape (B = 10, 6 s: 105 row
    splits x 58 tap groups, ragged last 64-step chunk), launched 50 times on the same operands: the two differ and the
    repeats vary only in the last bits of the atomic sums."""
    torch.manual_seed(3)
    t1, t = ops.conv_out_frames(601)
    a1 = torch.randn(10, 32, 61, t1, device=DEV)
    dy2 = torch.randn(10, 32, 21, t, device=DEV)
    monkeypatch.setenv('DS2_CONV_WGRAD_LDS', '0')
    dw_ref, db_ref = torch.empty(32, 32, 21, 11, device=DEV), torch.empty(32, device=DEV)
    ops.conv_wgrad(2, a1, dy2, t1, dw_ref, db_ref)
    monkeypatch.setenv('DS2_CONV_WGRAD_LDS', '1')
    for bf16 in ('0', '1'):                              # the f32-input MFMA form, then the split-operand form (the default)
        monkeypatch.setenv('DS2_CONV_WGRAD_BF16', bf16)
        worst_w = worst_b = 0.0
        for _ in range(50):
            dw, db = torch.empty_like(dw_ref), torch.empty_like(db_ref)
            ops.conv_wgrad(2, a1, dy2, t1, dw, db)
            worst_w = max(worst_w, float((dw - dw_ref).abs().max()))
            worst_b = max(worst_b, float((db - db_ref).abs().max()))
        assert worst_w <= 5e-6 * float(dw_ref.abs().max()), bf16
        assert worst_b <= 5e-6 * float(db_ref.abs().max()), bf16


@pytest.mark.parametrize('which,bsz,t_in', [(2, 3, 139), (2, 10, 75), (1, 2, 301), (1, 5, 130)])
def test_conv_wgrad_families_agree(ops, monkeypatch, which, bsz, t_in):
    """The weight gradients three ways against an fp64 reference: the direct kernel, the operands-through-LDS kernel on the
    f32-input matrix instruction, and (round 4, the default) the same with error-free split operands on the bf16 matrix pipe
    (csrc/conv.hip conv_wgrad_split_kernel).  Error relative to sum |d(out)| |in| per filter entry, as in the GEMM and
    conv2-forward family tests: the split form no worse than the f32 forms.  Operands in the training ranges: conv1's input
    is a normalised spectrogram, conv2's the clipped-ReLU output of conv1; d(out) small and same-signed in places."""
    torch.manual_seed(100 * which + bsz)
    cin, fin, kf = (1, 161, 41) if which == 1 else (32, 61, 21)
    x = (torch.randn(bsz, cin, fin, t_in) if which == 1 else torch.rand(bsz, cin, fin, t_in) * 20.0)
    w = (torch.randn(32, cin, kf, 11) / np.sqrt(cin * kf * 11)).double().requires_grad_(True)
    b = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    out = _conv_ref(which, x.double(), w, b)
    dy = torch.randn(tuple(out.shape)) * 1e-3 + 2e-4
    out.backward(dy.double())
    wa = torch.ones_like(w).requires_grad_(True)                       # sum |dy| |x| per filter entry: the error's scale
    _conv_ref(which, x.double().abs(), wa, torch.zeros(32, dtype=torch.float64)).backward(dy.double().abs())
    scale = wa.grad
    xd, dyd = x.to(DEV), dy.to(DEV)
    err, errb = {}, {}
    for name, env in (('direct', {'DS2_CONV_WGRAD_LDS': '0'}), ('lds-f32', {'DS2_CONV_WGRAD_LDS': '1', 'DS2_CONV_WGRAD_BF16': '0'}),
                      ('split', {'DS2_CONV_WGRAD_LDS': '1', 'DS2_CONV_WGRAD_BF16': '1'})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dw, db = torch.empty(32, cin, kf, 11, device=DEV), torch.empty(32, device=DEV)
        ops.conv_wgrad(which, xd, dyd, t_in, dw, db)
        err[name] = float(((dw.cpu().double() - w.grad).abs() / scale).max())
        errb[name] = float((db.cpu().double() - b.grad).abs().max() / float(dy.abs().sum(dim=(0, 2, 3)).max()))
    assert err['direct'] <= 2e-6 and err['lds-f32'] <= 2e-6, err
    assert err['split'] <= 1.25 * max(err['direct'], err['lds-f32']) + 1e-8, err
    assert max(errb.values()) <= 2e-6, errb


@pytest.mark.parametrize('bsz,t1', [(2, 56), (1, 33), (3, 129), (10, 150), (6, 400), (2, 1501 // 2)])
def test_conv2_forward_families_agree(ops, monkeypatch, bsz, t1):
    """conv2's forward pass three ways against torch: the gather kernel on the bf16 matrix pipe (default; 6 and 9 partial
    products; 32 or 64 positions per wave depending on the number of positions) and the direct kernel on the f32-input
    matrix instruction.  Error relative to sum |w||x| as in the GEMM family test: the split kernels no worse than the
    direct ones."""
    torch.manual_seed(bsz * 1000 + t1)
    x = torch.rand(bsz, 32, 61, t1, device=DEV) * 20.0                   # the clipped-ReLU range of conv1's output
    w = torch.randn(32, 32, 21, 11, device=DEV) / np.sqrt(32 * 21 * 11)
    b = torch.randn(32, device=DEV)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=(2, 1))
    scale = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=(2, 1))
    err = {}
    for name, env in (('split6', {'DS2_CONV_SPLIT': '6'}), ('split9', {'DS2_CONV_SPLIT': '9'}),
                      ('direct', {'DS2_CONV_SPLIT': '0'})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ops.conv_fwd(2, x, w, b, t1)
        assert out.shape == ref.shape
        err[name] = float(((out.double() - ref).abs() / scale).max())
    assert err['direct'] <= 2e-6, err
    assert err['split6'] <= 1.25 * err['direct'] + 1e-8, err
    assert err['split9'] <= 1.25 * err['direct'] + 1e-8, err


# ------------------------------------------------------------------------------------------- BN
@pytest.mark.parametrize('bsz,c,d,t,gb', [
    pytest.param(3, 32, 21, 57, ((0.5, 1.5), (-1, 6)), id='3-32-21-57'),
    pytest.param(2, 32, 1, 3, ((0.5, 1.5), (-1, 6)), id='2-32-1-3'),
    pytest.param(2, 32, 4, 8, ((0.5, 1.5), (-1, 6)), id='2-32-4-8'),
    pytest.param(1, 32, 61, 131, ((0.5, 1.5), (-1, 6)), id='1-32-61-131'),
    pytest.param(5, 32, 1, 2, ((0.5, 1.5), (-1, 6)), id='5-32-1-2'),
    pytest.param(3, 32, 21, 57, ((7, 9), (9, 11)), id='3-32-21-57-both-clamps')])
def test_bn2d_train_eval_and_backward(ops, bsz, c, d, t, gb):
    """(the planes of the 16-byte kernels start at every 4-byte offset: inner = d * t odd, < 4, a multiple of 4; with gamma in
    [7, 9] and beta in [9, 11] a tenth of the elements sits on either side of Hardtanh(0, 20), with the other ranges none
    reaches 20)"""
    rng = np.random.default_rng(20)
    x = torch.from_numpy((3 * rng.standard_normal((bsz, c, d, t)) + 5).astype(np.float32)).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(*gb[0], c).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.uniform(*gb[1], c).astype(np.float32)))
    rm, rv = bn.running_mean.clone().to(DEV), bn.running_var.clone().to(DEV)
    y = F.hardtanh(bn(x), 0, 20)
    dy = torch.from_numpy(rng.standard_normal((bsz, c, d, t)).astype(np.float32))
    y.backward(dy)
    g, be = bn.weight.detach().to(DEV), bn.bias.detach().to(DEV)
    xd = x.detach().to(DEV)
    mi = ops.bn2d_stats(xd, rm, rv, training=True)
    out = ops.bn2d_apply_htanh(xd, mi, g, be, layout_tbf=False)
    np.testing.assert_allclose(out.cpu().numpy(), y.detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(rm.cpu().numpy(), bn.running_mean.numpy(), atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), bn.running_var.numpy(), rtol=1e-5)
    out_t = ops.bn2d_apply_htanh(xd, mi, g, be, layout_tbf=True)
    ref_t = y.detach().reshape(bsz, c * d, t).permute(2, 0, 1).contiguous().numpy()
    np.testing.assert_allclose(out_t.cpu().numpy(), ref_t, atol=2e-5)
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx = ops.bn2d_htanh_bwd(xd, dy.to(DEV), mi, g, be, dg, db)
    np.testing.assert_allclose(dx.cpu().numpy(), x.grad.numpy(), atol=2e-5)
    np.testing.assert_allclose(dg.cpu().numpy(), bn.weight.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(db.cpu().numpy(), bn.bias.grad.numpy(), rtol=1e-4, atol=1e-4)
    bn.eval()
    with torch.no_grad():
        y_eval = F.hardtanh(bn(x.detach()), 0, 20)
    mi_e = ops.bn2d_stats(xd, rm, rv, training=False)
    out_e = ops.bn2d_apply_htanh(xd, mi_e, g, be, layout_tbf=False)
    np.testing.assert_allclose(out_e.cpu().numpy(), y_eval.numpy(), atol=2e-5)


def test_bn1d_with_direction_sum(ops):
    rng = np.random.default_rng(21)
    rows, feat = 530, 800
    xa = torch.from_numpy(rng.standard_normal((rows, feat)).astype(np.float32)).requires_grad_(True)
    xb = torch.from_numpy((2 * rng.standard_normal((rows, feat)) + 1).astype(np.float32))
    bn = torch.nn.BatchNorm1d(feat)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, feat).astype(np.float32)))
        bn.bias.copy_(torch.from_numpy(rng.uniform(-1, 1, feat).astype(np.float32)))
    rm, rv = bn.running_mean.clone().to(DEV), bn.running_var.clone().to(DEV)
    y = bn(xa + xb)
    dy = torch.from_numpy(rng.standard_normal((rows, feat)).astype(np.float32))
    y.backward(dy)
    g, be = bn.weight.detach().to(DEV), bn.bias.detach().to(DEV)
    a_, b_ = xa.detach().to(DEV), xb.to(DEV)
    mi = ops.bn1d_stats(a_, b_, rows, feat, rm, rv, training=True)
    out = ops.bn1d_apply(a_, b_, mi, g, be, rows, feat)
    np.testing.assert_allclose(out.cpu().numpy(), y.detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(rm.cpu().numpy(), bn.running_mean.numpy(), atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), bn.running_var.numpy(), rtol=1e-5)
    dg, db = torch.empty(feat, device=DEV), torch.empty(feat, device=DEV)
    dx = ops.bn1d_bwd(a_, b_, dy.to(DEV), mi, g, rows, feat, dg, db)
    np.testing.assert_allclose(dx.cpu().numpy(), xa.grad.numpy(), atol=2e-5)
    np.testing.assert_allclose(dg.cpu().numpy(), bn.weight.grad.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(db.cpu().numpy(), bn.bias.grad.numpy(), rtol=1e-4, atol=1e-4)
    # single-input form
    mi1 = ops.bn1d_stats(a_, None, rows, feat, None, None, training=True)
    ref1 = F.batch_norm(xa.detach(), None, None, bn.weight.detach(), bn.bias.detach(), True)
    np.testing.assert_allclose(ops.bn1d_apply(a_, None, mi1, g, be, rows, feat).cpu().numpy(), ref1.numpy(), atol=2e-5)


# ------------------------------------------------------------------------------------------- GRU
@pytest.mark.parametrize('mode', ['step', 'persistent'])
@pytest.mark.parametrize('t,bsz,n_in,hid', [(9, 3, 24, 32), (6, 10, 40, 800), (5, 20, 16, 64), (4, 40, 16, 72),
                                            (3, 64, 8, 800), (1, 2, 8, 16), (40, 33, 8, 256), (25, 17, 8, 512),
                                            (7, 8, 16, 800), (5, 32, 16, 800), (6, 16, 16, 800)])
def test_gru_recurrence_fwd_bwd(ops, monkeypatch, mode, t, bsz, n_in, hid):
    if mode == 'persistent' and hid % 16 != 0:
        pytest.skip('persistent kernel needs H % 16 == 0 (falls back to the per-step kernels)')
    monkeypatch.setattr(ops, 'GRU_MODE', mode)
    torch.manual_seed(t * 100 + bsz)
    gru = torch.nn.GRU(n_in, hid, bidirectional=True, bias=False)
    x = torch.randn(t, bsz, n_in, requires_grad=True)
    y, _ = gru(x)
    ysum = y[:, :, :hid] + y[:, :, hid:]
    dy = torch.randn(t, bsz, hid)
    ysum.backward(dy)
    w_ih = torch.cat([gru.weight_ih_l0, gru.weight_ih_l0_reverse], 0).detach().to(DEV).contiguous()   # (6H, In)
    w_hh = torch.stack([gru.weight_hh_l0, gru.weight_hh_l0_reverse], 0).detach().to(DEV).contiguous()  # (2,3H,H)
    xd = x.detach().to(DEV)
    gates = ops.gemm(xd.view(t * bsz, n_in), w_ih, trans_b=True).view(t, bsz, 2, 3 * hid)
    ghn, hout = ops.gru_bidir_fwd(gates, w_hh, t, bsz, hid)
    got = (hout[0] + hout[1]).cpu().numpy()
    np.testing.assert_allclose(got, ysum.detach().numpy(), atol=3e-5)
    np.testing.assert_allclose(hout[0].cpu().numpy(), y[:, :, :hid].detach().numpy(), atol=3e-5)
    # saved tensors against the explicit restatement (forward direction)
    from oracle.model import gru_direction_explicit
    sv = gru_direction_explicit(x.detach(), gru.weight_ih_l0.detach(), gru.weight_hh_l0.detach())
    np.testing.assert_allclose(gates[:, :, 0, :hid].cpu().numpy(), sv['r'].numpy(), atol=3e-5)
    np.testing.assert_allclose(gates[:, :, 0, 2 * hid:].cpu().numpy(), sv['n'].numpy(), atol=3e-5)
    np.testing.assert_allclose(ghn[:, :, 0].cpu().numpy(), sv['ghn'].numpy(), atol=3e-5)
    # backward
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    ops.gru_bidir_bwd(gates, ghn, hout, dy.to(DEV), w_hh_t, t, bsz, hid)
    dgi = gates.view(t * bsz, 6 * hid)
    dx = ops.gemm(dgi, w_ih)                                    # (TB, In)
    np.testing.assert_allclose(dx.view(t, bsz, n_in).cpu().numpy(), x.grad.numpy(), atol=5e-5)
    dw_ih = ops.gemm(dgi, xd.view(t * bsz, n_in), trans_a=True)  # (6H, In)
    ref_dw_ih = torch.cat([gru.weight_ih_l0.grad, gru.weight_ih_l0_reverse.grad], 0).numpy()
    np.testing.assert_allclose(dw_ih.cpu().numpy(), ref_dw_ih, rtol=1e-4, atol=1e-4)
    if t > 1:
        # dW_hh (forward direction) = dGH[1:]^T h[:-1]
        dgh = torch.cat([gates[1:, :, 0, :2 * hid], ghn[1:, :, 0, :]], -1).reshape((t - 1) * bsz, 3 * hid).contiguous()
        hprev = hout[0, :-1].reshape((t - 1) * bsz, hid).contiguous()
        dw_hh = ops.gemm(dgh, hprev, trans_a=True)
        np.testing.assert_allclose(dw_hh.cpu().numpy(), gru.weight_hh_l0.grad.numpy(), rtol=1e-4, atol=1e-4)
        dgh_r = torch.cat([gates[:-1, :, 1, :2 * hid], ghn[:-1, :, 1, :]], -1).reshape((t - 1) * bsz, 3 * hid)
        hnext = hout[1, 1:].reshape((t - 1) * bsz, hid).contiguous()
        dw_hh_r = ops.gemm(dgh_r.contiguous(), hnext, trans_a=True)
        np.testing.assert_allclose(dw_hh_r.cpu().numpy(), gru.weight_hh_l0_reverse.grad.numpy(), rtol=1e-4, atol=1e-4)


def _persistent_forms_against_step_kernels(ops, monkeypatch, t, bsz, hid, env, spare_cus=-1, dh=False):
    """One forward and one backward recurrence with the persistent kernels that ``env`` selects, against the launch-per-step
    kernels on the same inputs.  ``dh``: the persistent backward pass is the d(h) hand-off, on the forward pass's own
    coefficient planes."""
    torch.manual_seed(t + bsz)
    k = 1.0 / hid ** 0.5
    w_hh = ((torch.rand(2, 3 * hid, hid) * 2 - 1) * k).to(DEV)
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    gi = torch.randn(t, bsz, 2, 3 * hid).to(DEV)
    d_out = torch.randn(t, bsz, hid).to(DEV)
    res = {}
    for mode in ('step', 'persistent'):
        monkeypatch.setattr(ops, 'GRU_MODE', mode)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        g = gi.clone()
        out = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid, want_coef=dh)
        ghn, hout, coef = out if dh else out + (None,)
        assert (coef is not None) == (dh and mode == 'persistent')
        fwd = (g.clone(), ghn.clone(), hout.clone())
        ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=spare_cus, coef=coef)
        torch.cuda.synchronize()
        ops.check_async_errors()
        res[mode] = fwd + (g, ghn)
    for a, b in zip(res['persistent'], res['step']):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=3e-5, rtol=1e-4)


@pytest.mark.parametrize('fwd_form,bwd_form', [('4', '4'), ('16', '16'), ('4', '16'), ('16', '4')])
@pytest.mark.parametrize('t,bsz,hid', [(7, 10, 800), (5, 27, 256), (4, 32, 800), (6, 5, 64), (9, 8, 800)])
def test_gru_persistent_mfma_forms_agree_with_step_kernels(ops, monkeypatch, fwd_form, bwd_form, t, bsz, hid):
    """Both MFMA forms of each persistent kernel (4x4x1 and 16x16x4; the default depends on the batch size) against
    the launch-per-step kernels on the same inputs."""
    _persistent_forms_against_step_kernels(ops, monkeypatch, t, bsz, hid, {'DS2_GRU_FWD': fwd_form, 'DS2_GRU_BWD': bwd_form})


_P16_FP32 = {'DS2_GRU_P2_BF16': '0', 'DS2_GRU_P2_BF16_BWD': '0'}
_P16_BF16 = {'DS2_GRU_P2_BF16': '1', 'DS2_GRU_P2_BF16_BWD': '1'}


@pytest.mark.parametrize('bsz,env', [(5, {'DS2_GRU_FWD': '16', 'DS2_GRU_BWD': '16'}), (17, _P16_FP32), (17, _P16_BF16),
                                     (33, _P16_FP32), (33, _P16_BF16)],
                         ids=['b5-whole', 'b17-fp32', 'b17-bf16', 'b33-fp32', 'b33-bf16'])
@pytest.mark.parametrize('hid', [32, 64, 128, 256, 384])
def test_gru_persistent_16x16_narrow_widths_agree_with_step_kernels(ops, monkeypatch, hid, bsz, env):
    """The instantiations of the 16x16 kernels (gru_persist16.hip) that the H = 800 cases do not reach: these five widths run
    k blocks per wave (KBW) 1, 1, 1, 2, 4 (forward fp32), 1, 1, 1, 1, 2 (forward bf16), 1, 2, 4, 8, 19 (backward fp32) and
    1, 1, 2, 5, 5 (backward bf16).  B = 5: the whole-batch forms with 5 live rows of one tile; B = 17: the two-part forms
    with parts of 9 and 8 rows; B = 33: two batch tiles per part, 17 rows (one in the second tile) and 16 (an empty second
    tile).  T = 5 uses both ring slots and a steady-state step.  The whole-batch forms with 2 and 4 batch tiles exist in the
    tuning library only and are not run here."""
    _persistent_forms_against_step_kernels(ops, monkeypatch, 5, bsz, hid, dict(env, DS2_GRU_BWD_DH='0'))
    assert not ops._persistent_off


_P4 = {'DS2_GRU_FWD': '4', 'DS2_GRU_BWD': '4'}
# (id, hid, bsz, env, spare_cus, dh)
_P4_NARROW = [('h%d-b%d-%s' % (hid, bsz, 'cus%d' % spare if spare >= 0 else 'default'), hid, bsz, _P4, spare, False)
              for hid in (64, 256, 384) for bsz in (3, 4, 5, 7, 8, 9, 10, 12, 16, 24)
              for spare in ((0, 52, 82) if 9 <= bsz <= 12 else (-1,))]
_P4_NARROW += [('h%d-b10-default-narrowfwd' % hid, hid, 10, dict(_P4, DS2_GRU_FWD_WIDE='0'), -1, False) for hid in (64, 256, 384)]
_P4_NARROW += [('h64-b%d-cus52-dh' % bsz, 64, bsz, dict(_P4, DS2_GRU_BWD_DH='1'), 52, True) for bsz in (9, 10, 12)]


@pytest.mark.parametrize('hid,bsz,env,spare_cus,dh', [c[1:] for c in _P4_NARROW], ids=[c[0] for c in _P4_NARROW])
def test_gru_persistent_4x4_narrow_widths_agree_with_step_kernels(ops, monkeypatch, hid, bsz, env, spare_cus, dh):
    """The instantiations of the 4x4x1 kernels (gru_persist.hip) that the H = 800 cases do not reach: these three widths run
    backward k groups per wave (NGI) 1, 2, 3 and forward NGI 1.  B = 3, 4: one part, speculative (backward NRG = 2, forward
    P = 1); 5, 7, 8: two parts (3 / 2, 4 / 3, 4 / 4 rows), the backward broadcast deal with NRG = 4 and forward P = 2;
    9, 10, 12: three parts of 3 / 3 / 3, 4 / 4 / 2 and 4 / 4 / 4 rows, the broadcast deal with 20, 24 and 28 units by spare_cus (NRG = 5, 6, 7) and the forward
    20-unit form (UGX = 5; 24 units with DS2_GRU_FWD_WIDE=0); 16 and 24: the counted protocol, backward NRG = 4 and 6, forward
    two batch-row passes (NBT = 2).  The d(h) hand-off exists at H = 64 and 800 only: its 24-unit form at H = 64, which the
    short-sequence d(h) test (spare_cus 0 and 82) does not reach.  T = 5 uses every ring slot and a steady-state step."""
    _persistent_forms_against_step_kernels(ops, monkeypatch, 5, bsz, hid, dict({'DS2_GRU_BWD_DH': '0'}, **env), spare_cus, dh)
    assert not ops._persistent_off


def _long_sequence_case(ops, monkeypatch, bsz, reps, during=None, spare_cus=(-1,)):
    t, hid = 746, 800
    torch.manual_seed(1)
    k = 1.0 / hid ** 0.5
    w_hh = ((torch.rand(2, 3 * hid, hid) * 2 - 1) * k).to(DEV)
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    gi = torch.randn(t, bsz, 2, 3 * hid).to(DEV)
    d_out = (0.1 * torch.randn(t, bsz, hid)).to(DEV)
    res = {}
    for rep, mode in enumerate(['step'] + ['persistent'] * reps):
        monkeypatch.setattr(ops, 'GRU_MODE', mode)
        g = gi.clone()
        torch.cuda.synchronize()
        if during is not None and mode != 'step':
            during()
        ghn, hout = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid)
        fwd = (g.clone(), ghn.clone(), hout.clone())
        ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=spare_cus[rep % len(spare_cus)])
        torch.cuda.synchronize()
        ops.check_async_errors()
        cur = fwd + (g, ghn)
        if mode == 'step':
            res = cur
        else:
            for a, b, tol in zip(cur, res, (2e-5, 2e-5, 2e-5, 2e-4, 2e-4)):
                scale = float(b.abs().max())
                assert float((a - b).abs().max()) <= tol * max(scale, 1.0)
    assert not ops._persistent_off                      # no launch fell back to the per-step kernels


@pytest.mark.parametrize('bsz', [4, 8, 10, 12, 13, 16, 17, 32, 64])
def test_gru_persistent_long_sequence_matches_step_kernels(ops, monkeypatch, bsz):
    """T = 746 steps of the real layer shape, repeatedly: every hand-off must be fresh (a stale h would show up as an O(1)
    difference), and the bounded spins must never trip.  The batch sizes cover every hand-off protocol and kernel form:
    4 (speculative, one part), 8 (speculative, two parts), 10 (speculative, three parts: the headline), 12 (the last batch
    size of the speculative protocol), 13 and 16 (forward: the first of the two-part split-operand forms; backward: the 4x4x1
    forms with the counted protocol), 17 (the first of the two-part 16x16x4 backward forms), 32 and 64."""
    _long_sequence_case(ops, monkeypatch, bsz, 3 if bsz <= 12 else 2)


@pytest.mark.parametrize('bsz', [9, 10, 12])
def test_gru_backward_forms_by_spare_cus_match_step_kernels(ops, monkeypatch, bsz):
    """ds2_gru_bidir_bwd_persistent_ex: the three-part speculative backward kernel with 20, 24 and 28 hidden units per workgroup
    (240 / 204 / 174 workgroups at H = 800: spare_cus 0, 52, 82 -- what codes/model.py asks for under the top layer and under
    the others) against the launch-per-step kernels at T = 746; twice each, interleaved, on ONE exchange workspace (the ring
    layout does not depend on the form: a launch must not read what another form's launch left there)."""
    _long_sequence_case(ops, monkeypatch, bsz, 6, spare_cus=(0, 82, 52))


def test_transpose2d_group_matches_single_transposes(ops):
    """ds2_transpose2d_group: separately placed inputs of `batch` matrices each, one launch (the recurrent weights of all
    layers for the backward recurrence)."""
    torch.manual_seed(5)
    for cnt, batch, rows, cols in ((5, 2, 96, 32), (1, 1, 33, 70), (8, 2, 2400, 800)):
        xs = [torch.randn(batch, rows, cols).to(DEV) for _ in range(cnt)]
        out = torch.empty(cnt, batch, cols, rows, device=DEV)
        ops.transpose2d_group(xs, batch, rows, cols, out)
        for i, x in enumerate(xs):
            assert torch.equal(out[i], x.transpose(1, 2).contiguous())


def _dh_case(ops, monkeypatch, t, bsz, hid, spare_cus, reps=2, own_coef=True):
    """The d(h)-hand-off backward recurrence (ds2_gru_bidir_bwd_persistent_dh) against the launch-per-step kernels AND against
    the d(gh)-hand-off form on the same forward pass."""
    torch.manual_seed(3 * t + bsz)
    k = 1.0 / hid ** 0.5
    w_hh = ((torch.rand(2, 3 * hid, hid) * 2 - 1) * k).to(DEV)
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    gi = torch.randn(t, bsz, 2, 3 * hid).to(DEV)
    d_out = (0.1 * torch.randn(t, bsz, hid)).to(DEV)
    monkeypatch.setattr(ops, 'GRU_MODE', 'step')
    g = gi.clone()
    ghn, hout = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid)
    ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid)
    torch.cuda.synchronize()
    ref = (g, ghn)
    monkeypatch.setattr(ops, 'GRU_MODE', 'persistent')
    monkeypatch.setenv('DS2_GRU_BWD_DH', '1')
    assert ops.gru_bwd_dh_wanted(gi.device, bsz, hid)
    for rep in range(reps):
        for spare in spare_cus:
            g = gi.clone()
            ghn, hout, coef = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid, want_coef=True)
            assert coef is not None
            # the planes the forward launch produced (its own gate threads at B = 9 .. 12, H = 800; the elementwise pass
            # elsewhere) against the elementwise pass run here on the same saved tensors
            again = ops.gru_bwd_coef(g, ghn, hout, t, bsz, hid)
            scale = max(float(again.abs().max()), 1.0)
            assert float((coef - again).abs().max()) <= 2e-6 * scale
            ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=spare, coef=coef if own_coef else again)
            torch.cuda.synchronize()
            ops.check_async_errors()
            for a, b in zip((g, ghn), ref):
                scale = max(float(b.abs().max()), 1.0)
                assert float((a - b).abs().max()) <= 2e-4 * scale
    assert not ops._persistent_off


@pytest.mark.parametrize('bsz', [5, 8, 9, 10, 12])
def test_gru_backward_dh_handoff_matches_step_kernels_long_sequence(ops, monkeypatch, bsz):
    """T = 746 at the real width: every form of the d(h)-hand-off kernel (two parts of 16 units for B = 5 .. 8; three parts of
    20 / 24 / 28 units for B = 9 .. 12, chosen by spare_cus), twice each, interleaved on ONE exchange workspace with the forward
    launches.  A stale dh fragment or a coefficient fragment of the wrong step is an O(1) difference."""
    _dh_case(ops, monkeypatch, 746, bsz, 800, (0, 82, 52) if bsz >= 9 else (-1,))


@pytest.mark.parametrize('t,bsz', [(1, 10), (2, 9), (7, 12), (9, 5), (33, 8)])
def test_gru_backward_dh_handoff_short_sequences_and_narrow_width(ops, monkeypatch, t, bsz):
    """T = 1 (the peeled first step only), T = 2, odd lengths; H = 64 (2 runs per wave: one partly filled register)."""
    _dh_case(ops, monkeypatch, t, bsz, 64, (0, 82) if bsz >= 9 else (-1,), reps=1)
    _dh_case(ops, monkeypatch, t, bsz, 800, (82,) if bsz >= 9 else (-1,), reps=1, own_coef=False)


def test_gru_backward_dh_handoff_is_the_default_where_the_forward_kernel_writes_the_planes(ops, monkeypatch):
    monkeypatch.delenv('DS2_GRU_BWD_DH', raising=False)
    monkeypatch.setattr(ops, 'GRU_MODE', 'persistent')
    dev = torch.device(DEV)
    assert ops.gru_bwd_dh_wanted(dev, 10, 800) and ops.gru_bwd_dh_wanted(dev, 9, 800) and ops.gru_bwd_dh_wanted(dev, 12, 800)
    assert not ops.gru_bwd_dh_wanted(dev, 8, 800) and not ops.gru_bwd_dh_wanted(dev, 13, 800) and not ops.gru_bwd_dh_wanted(dev, 10, 256)
    monkeypatch.setenv('DS2_GRU_BWD_DH', '0')
    assert not ops.gru_bwd_dh_wanted(dev, 10, 800)
    monkeypatch.setattr(ops, 'GRU_MODE', 'step')
    monkeypatch.delenv('DS2_GRU_BWD_DH', raising=False)
    assert not ops.gru_bwd_dh_wanted(dev, 10, 800)


@pytest.mark.parametrize('bsz,fwd_bf16,bwd_bf16', [(17, '0', '0'), (32, '0', '0'), (64, '0', '0'), (17, '1', '1'), (32, '1', '1'),
                                                   (64, '1', '1')])
def test_gru_two_part_forms_f32_and_split_operand_families(ops, monkeypatch, bsz, fwd_bf16, bwd_bf16):
    """The two-part 16x16 recurrences (B >= 17) in both arithmetic families against the launch-per-step kernels: the
    f32-input MFMA forms (the default backward form; the forward one is DS2_GRU_P2_BF16=0) and the split-operand forms on the
    bf16 matrix pipe (the default forward form; the backward twin is DS2_GRU_P2_BF16_BWD=1), whose new state crosses the
    exchange ring as three bf16 planes."""
    monkeypatch.setenv('DS2_GRU_P2_BF16', fwd_bf16)
    monkeypatch.setenv('DS2_GRU_P2_BF16_BWD', bwd_bf16)
    _long_sequence_case(ops, monkeypatch, bsz, 1)


_co_resident = {}


def co_resident_load(duration_ms=300.0, wgs=32, mbytes=64, iters=10):
    """Launch the RCCL stand-in (tests/co_resident_kernel.hip: `wgs` long-lived workgroups streaming HBM) back to back on a
    stream of its own for about ``duration_ms`` of stand-alone time (one launch is timed once per process; beside other
    work it runs longer); returns (stream, event recorded behind the last launch, buffer)."""
    import ctypes
    if 'lib' not in _co_resident:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libco_resident.so'))
        lib.co_resident_stream.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.co_resident_stream.restype = ctypes.c_int
        _co_resident['lib'] = lib
    lib = _co_resident['lib']
    buf = torch.zeros(mbytes << 18, dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    key = (wgs, mbytes, iters)
    if key not in _co_resident:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            assert lib.co_resident_stream(buf.data_ptr(), buf.numel() * 4, wgs, iters, stream.cuda_stream) == 0
            e0.record(stream)
            for _ in range(4):
                assert lib.co_resident_stream(buf.data_ptr(), buf.numel() * 4, wgs, iters, stream.cuda_stream) == 0
            e1.record(stream)
        e1.synchronize()
        _co_resident[key] = e0.elapsed_time(e1) / 4.0
        print('co-resident stand-in: %d workgroups, %.3f ms per launch stand-alone' % (wgs, _co_resident[key]))
    launches = max(8, int(duration_ms / _co_resident[key]) + 1)
    for _ in range(launches):
        assert lib.co_resident_stream(buf.data_ptr(), buf.numel() * 4, wgs, iters, stream.cuda_stream) == 0
    done = torch.cuda.Event()
    done.record(stream)
    return stream, done, buf


def test_gru_persistent_long_sequence_narrow_forward_form(ops, monkeypatch):
    """B = 9 .. 12 runs the forward recurrence on 240 CUs (20-unit slices) by default; the 24-unit form on 204 CUs that the
    backward pass uses stays selectable (DS2_GRU_FWD_WIDE=0) and is checked here."""
    monkeypatch.setenv('DS2_GRU_FWD_WIDE', '0')
    _long_sequence_case(ops, monkeypatch, 10, 2)


@pytest.mark.parametrize('bsz', [8, 10, 32])
def test_gru_persistent_long_sequence_beside_a_streaming_kernel(ops, monkeypatch, bsz):
    """The same check with 32 workgroups of another kernel streaming HBM on a third stream the whole time (the condition
    of a data-parallel step, where RCCL's channel kernels run beside the recurrence, and of tools/interference_probe.py):
    the speculative hand-off is timing dependent by design, so it is exercised under a neighbour's memory traffic too
    (B = 32: the counted protocol of the two-part forms, the forward one on the bf16 pipe)."""
    held = []

    def during():
        held.append(co_resident_load(duration_ms=60.0))

    _long_sequence_case(ops, monkeypatch, bsz, 2, during=during)
    for _, done, _ in held:
        done.synchronize()


# ------------------------------------------------------------------------------------------- CTC
def _ctc_case(ops, t_max, bsz, nalpha, label_lens, act_lens, seed, repeat_first=True):
    from oracle import ctc as octc
    rng = np.random.default_rng(seed)
    acts = (2 * rng.standard_normal((t_max, bsz, nalpha))).astype(np.float32)
    labels = rng.integers(1, nalpha, size=int(sum(label_lens))).astype(np.int32)
    if repeat_first and label_lens[0] > 1:
        labels[1] = labels[0]
    offs = np.concatenate([[0], np.cumsum(label_lens)[:-1]]).astype(np.int32)
    costs, grad = ops.ctc_loss_grad(_t(acts), _t(labels), _t(offs), _t(np.asarray(label_lens, np.int32)),
                                    _t(np.asarray(act_lens, np.int32)), int(max(label_lens)))
    ref_costs, ref_grad = octc.ctc_loss_and_grad(acts, labels, act_lens, label_lens)
    return costs.cpu().numpy(), grad.cpu().numpy(), ref_costs, ref_grad


@pytest.mark.parametrize('nalpha', [29, 43])
def test_ctc_ragged(ops, nalpha):
    costs, grad, rc, rg = _ctc_case(ops, 60, 5, nalpha, [7, 0, 12, 3, 20], [60, 31, 44, 9, 41], seed=nalpha)
    np.testing.assert_allclose(costs, rc, rtol=1e-4)
    np.testing.assert_allclose(grad, rg, atol=2e-5)
    assert np.all(grad[31:, 1] == 0)


def test_ctc_infeasible_and_long(ops):
    # utterance 1 needs 3 labels + 2 repeats > 4 frames: cost +inf, zero gradient
    from oracle import ctc as octc
    acts = np.random.default_rng(7).standard_normal((8, 2, 5)).astype(np.float32)
    labels = np.asarray([1, 2, 3, 3, 3], np.int32)
    costs, grad = ops.ctc_loss_grad(_t(acts), _t(labels), _t(np.asarray([0, 2], np.int32)),
                                    _t(np.asarray([2, 3], np.int32)), _t(np.asarray([8, 4], np.int32)), 3)
    rc, rg = octc.ctc_loss_and_grad(acts, labels, [8, 4], [2, 3])
    assert np.isinf(costs.cpu().numpy()[1]) and np.isinf(rc[1])
    np.testing.assert_allclose(costs.cpu().numpy()[0], rc[0], rtol=1e-5)
    assert np.all(grad.cpu().numpy()[:, 1] == 0)
    np.testing.assert_allclose(grad.cpu().numpy()[:, 0], rg[:, 0], atol=2e-5)
    # the training step's rule (codes/engine.py:24-30): one infinite cost zeroes the WHOLE batch's gradient
    costs2, grad2 = ops.ctc_loss_grad(_t(acts), _t(labels), _t(np.asarray([0, 2], np.int32)),
                                      _t(np.asarray([2, 3], np.int32)), _t(np.asarray([8, 4], np.int32)), 3,
                                      zero_batch_if_inf=True)
    assert np.array_equal(costs2.cpu().numpy(), costs.cpu().numpy())
    assert np.all(grad2.cpu().numpy() == 0)
    # long utterance: T = 746, L = 200 (S = 401 states, two states per thread)
    costs, grad, rc, rg = _ctc_case(ops, 746, 2, 29, [200, 150], [746, 700], seed=9)
    np.testing.assert_allclose(costs, rc, rtol=1e-4)
    np.testing.assert_allclose(grad, rg, atol=5e-5)
    # S = 601 states: the 1024-thread form; utterance lengths around the 32-frame staging chunks of the emissions (1 frame, one
    # chunk exactly, one chunk + 1, two chunks - 1), a one-label and an empty transcript, 43 symbols (23-frame chunks)
    costs, grad, rc, rg = _ctc_case(ops, 700, 3, 29, [300, 260, 1], [700, 655, 1], seed=10)
    np.testing.assert_allclose(costs, rc, rtol=1e-4)
    np.testing.assert_allclose(grad, rg, atol=5e-5)
    for nalpha, lens in ((29, [33, 34, 63, 2]), (43, [24, 25, 46, 47])):
        costs, grad, rc, rg = _ctc_case(ops, 64, 4, nalpha, [5, 0, 9, 1], lens, seed=11)
        np.testing.assert_allclose(costs, rc, rtol=1e-4)
        np.testing.assert_allclose(grad, rg, atol=2e-5)


# ------------------------------------------------------------------------------------------- optimiser
def test_clip_sgd_matches_torch(ops):
    torch.manual_seed(0)
    n = 100003
    p = torch.nn.Parameter(torch.randn(n))
    opt = torch.optim.SGD([p], lr=3e-4, momentum=0.9, nesterov=True)
    n_pad = (n + 3) // 4 * 4
    pd = torch.zeros(n_pad, device=DEV); pd[:n] = p.detach().to(DEV)
    buf = torch.zeros(n_pad, device=DEV)
    for step, scale in enumerate((10.0, 0.01, 50.0)):
        g = torch.randn(n) * scale
        p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([p], 400.0)
        opt.step()
        gd = torch.zeros(n_pad, device=DEV); gd[:n] = g.to(DEV)
        ss = ops.sumsq(gd)
        assert abs(float(ss.item()) ** 0.5 - float(total)) < 1e-3 * float(total)
        ops.clip_sgd_nesterov(pd, gd, buf, ss, 1.0, 400.0, 3e-4, 0.9, step == 0)
        np.testing.assert_allclose(pd[:n].cpu().numpy(), p.detach().numpy(), atol=2e-6)


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_gru_persistent_lost_arrival_times_out_instead_of_hanging(which):
    """Every spin in the persistent kernels is bounded: with one workgroup's arrival suppressed the launch ends after
    the timeout (5 s in the release library, 1.5 s in the fault-injection build this test runs), the STICKY flag survives later launches until the host checks it, the device falls back to the
    per-step kernels for later launches, and after the host's reset the persistent kernels work again.  Runs against
    the fault-injection build in a fresh process (tests/fault_inject_worker.py); the release library has no such hook."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'tests', 'fault_inject_worker.py'), which],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, DS2_GRU_MODE='auto'))
    assert out.returncode == 0 and 'OK ' + which in out.stdout, out.stderr[-3000:]


def test_release_library_ignores_the_debug_variable(ops, monkeypatch):
    """DS2_GRU_DBG must not change results of the shipped library (it used to skip waits / MFMAs / arrivals)."""
    t, bsz, hid = 5, 10, 800
    torch.manual_seed(1)
    w_hh = (torch.randn(2, 3 * hid, hid) * 0.02).to(DEV)
    gi = torch.randn(t, bsz, 2, 3 * hid).to(DEV)
    monkeypatch.setattr(ops, 'GRU_MODE', 'persistent')
    res = []
    for dbg in ('0', '67'):
        monkeypatch.setenv('DS2_GRU_DBG', dbg)
        g = gi.clone()
        ghn, hout = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid)
        torch.cuda.synchronize()
        ops.check_async_errors()
        res.append((g, ghn, hout))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_gemm_tn_group_matches_separate_launches(ops):
    """The grouped TN launch (the four dW_hh problems of a BiGRU layer in one kernel) against fp64."""
    rng = np.random.default_rng(11)
    k, n = 1234, 200
    ms = [400, 200, 400, 200]
    a = [_t(rng.standard_normal((k, m + 8)).astype(np.float32)) for m in ms]          # leading dimension > M
    b = [_t(rng.standard_normal((k, n)).astype(np.float32)) for _ in range(2)]
    c = [torch.full((m, n), 7.0, device=DEV) for m in ms]                               # must be overwritten, not added to
    problems = [(a[i].data_ptr(), a[i].shape[1], ms[i], b[i // 2].data_ptr(), n, c[i].data_ptr(), n) for i in range(4)]
    ops.gemm_tn_group(problems, n, k)
    for i in range(4):
        ref = a[i].cpu().numpy()[:, :ms[i]].astype(np.float64).T @ b[i // 2].cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(c[i].cpu().numpy(), ref, rtol=0, atol=2e-6 * np.sqrt(k) * 4)
    for ci in c:                                                                        # accumulate: C += A^T B
        ci.fill_(7.0)
    ops.gemm_tn_group(problems, n, k, accumulate=True)
    for i in range(4):
        ref = a[i].cpu().numpy()[:, :ms[i]].astype(np.float64).T @ b[i // 2].cpu().numpy().astype(np.float64) + 7.0
        np.testing.assert_allclose(c[i].cpu().numpy(), ref, rtol=0, atol=2e-6 * np.sqrt(k) * 4)
    ops.gemm_tn_group(problems[:1], n, k)                                               # a group of one
    ref = a[0].cpu().numpy()[:, :ms[0]].astype(np.float64).T @ b[0].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(c[0].cpu().numpy(), ref, rtol=0, atol=2e-6 * np.sqrt(k) * 4)
