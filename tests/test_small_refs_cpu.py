"""The references of tests/small_refs.py against torch and the oracle, on the CPU."""
import numpy as np
import pytest
import torch

from oracle import host
from oracle import spectrogram as ospec
from tests import small_refs as refs


@pytest.mark.parametrize('grad_scale,max_norm', [(1.0, 40.0), (0.125, 5.0), (-0.125, 5.0), (-2.0, 1e9)])
def test_nesterov_clip_step_matches_torch_sgd_in_float64(grad_scale, max_norm):
    """Three steps of clip_grad_norm_ + SGD(nesterov=True) on float64 tensors; the gradient scales make the first and the
    third step clip and the second not (norms about 317, 0.3 and 1585 times |grad_scale|; max_norm = 1e9: never)."""
    rng = np.random.default_rng(0)
    n, lr, momentum = 1003, 3e-4, 0.9
    p0 = rng.standard_normal(n)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([pt], lr=lr, momentum=momentum, nesterov=True)
    p, buf, coefs = p0.copy(), rng.standard_normal(n), []              # (the first step must ignore what buf holds)
    for step, scale in enumerate((10.0, 0.01, 50.0)):
        g = rng.standard_normal(n) * scale
        pt.grad = torch.from_numpy(g * grad_scale)
        total = float(torch.nn.utils.clip_grad_norm_([pt], max_norm))
        opt.step()
        p, buf, coef = refs.nesterov_clip_step(p, g, buf, grad_scale, max_norm, lr, momentum, step == 0)
        coefs.append(coef)
        assert abs(coef - min(1.0, max_norm / (total + 1e-6))) <= 1e-12
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(buf, opt.state[pt]['momentum_buffer'].numpy(), rtol=0, atol=1e-12 * 50 * abs(grad_scale))
    if max_norm < 1e9:
        assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0
    else:
        assert coefs == [1.0, 1.0, 1.0]


def test_nesterov_clip_step_without_clip_and_with_a_given_sumsq():
    rng = np.random.default_rng(1)
    p, g, buf = rng.standard_normal(50), 100 * rng.standard_normal(50), rng.standard_normal(50)
    a = refs.nesterov_clip_step(p, g, buf, -0.5, 1.0, 0.01, 0.9, False, clip=False)
    assert a[2] == 1.0
    np.testing.assert_allclose(a[1], 0.9 * buf - 0.5 * g, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a[0], p - 0.01 * (-0.5 * g + 0.9 * a[1]), rtol=0, atol=1e-12)
    b = refs.nesterov_clip_step(p, g, buf, -0.5, 1.0, 0.01, 0.9, False, sumsq=float((g * g).sum()))
    c = refs.nesterov_clip_step(p, g, buf, -0.5, 1.0, 0.01, 0.9, False)
    assert b[2] == c[2] < 1.0 and np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1])
    d = refs.nesterov_clip_step(p, g, buf, -0.5, 1.0, 0.01, 0.9, False, sumsq=4.0 * float((g * g).sum()))
    assert abs(d[2] - 1.0 / (np.sqrt((g * g).sum()) + 1e-6)) < 1e-12         # twice the norm, times |grad_scale| = 1/2


def test_collapse_agrees_with_the_oracle_greedy_decode():
    """The case of tests/test_kernels_gpu.py::test_softmax_argmax_collapse, and the sizes the oracle does not take."""
    rng = np.random.default_rng(4)
    for a in (29, 43):
        rng.standard_normal((301, a))                           # (that test's earlier draws: the same probabilities)
    labels = ['_'] + [chr(65 + i) for i in range(28)]
    probs = rng.random((4, 150, 29)).astype(np.float32)
    probs[:, :, 0] += 0.4
    probs[1, 10:20, 5] = 9.0
    sizes = np.asarray([150, 97, 1, 0], dtype=np.int32)
    strings, offsets = host.greedy_decode(probs, sizes, labels)
    best = probs.argmax(axis=2)
    for b in range(4):
        ids, offs = refs.collapse(best[b], sizes[b], 0)
        assert ''.join(labels[i] for i in ids) == strings[b]
        assert np.array_equal(np.asarray(offs, np.int32), offsets[b])
    row = [3, 3, 0, 3, 5, 5, 5, 0, 0, 7]
    assert refs.collapse(row, 10, 0) == ([3, 3, 5, 7], [0, 3, 4, 9])
    assert refs.collapse(row, 17, 0) == refs.collapse(row, 10, 0)          # a size beyond the row is the row
    assert refs.collapse(row, 0, 0) == ([], []) and refs.collapse(row, -3, 0) == ([], [])
    assert refs.collapse(row, 10, 5) == ([3, 0, 3, 0, 7], [0, 2, 3, 7, 9])  # another blank: 0 is a label like any other
    assert refs.collapse(row, 1, 3) == ([], [])


def test_softmax64_matches_torch_and_zeroes_minus_inf():
    rng = np.random.default_rng(2)
    x = 4 * rng.standard_normal((7, 65))
    x[2, 5:9] = -np.inf
    got = refs.softmax64(x)
    np.testing.assert_allclose(got, torch.softmax(torch.from_numpy(x), -1).numpy(), rtol=1e-13, atol=0)
    assert np.all(got[2, 5:9] == 0.0) and np.all(np.abs(got.sum(-1) - 1.0) < 1e-14)
    np.testing.assert_allclose(refs.softmax64(x + 1e4), got, rtol=1e-10, atol=0)      # (x + 1e4 rounds x to 2e-12)


def test_argmax_nan_first_equals_torch_argmax():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, 70)).astype(np.float32)
    x[1, 5] = x[1, 69] = 10.0                                   # ties
    x[2, 0] = x[2, 3] = x[2, 64] = 10.0
    x[3, :] = -np.inf
    x[4, 7] = np.inf
    x[5, 9] = -np.inf
    x[6, :] = np.nan
    x[7, 40] = np.nan                                           # one NaN beside larger finite values
    x[7, 3] = 50.0
    x[8, 66] = x[8, 2] = np.nan                                 # two: the first wins
    x[9, 11] = np.nan                                           # NaN against +inf: NaN still wins
    x[9, 4] = np.inf
    x[10, 8] = np.inf                                           # two +inf
    x[10, 30] = np.inf
    want = torch.argmax(torch.from_numpy(x), dim=1).numpy()
    assert np.array_equal(refs.argmax_nan_first(x), want)
    assert list(want[[1, 2, 3, 4, 6, 7, 8, 9, 10]]) == [5, 0, 0, 7, 0, 40, 2, 11, 8]


def test_float64_frontend_is_the_oracle_and_truncation_renormalises():
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(4000)).astype(np.float32)
    full = refs.log_spectrogram64(x)
    assert full.shape == (26, 161)
    np.testing.assert_allclose(full, ospec.log_spectrogram(x, dtype=np.float64), rtol=0, atol=1e-12)
    raw = np.log1p(ospec.stft_magnitude(x))
    cut = refs.log_spectrogram64(x, max_frames=17)
    want = (raw[:17] - raw[:17].mean()) / (raw[:17].std(ddof=1) + 1e-9)
    np.testing.assert_allclose(cut, want, rtol=0, atol=1e-12)
    batch = refs.batch_log_spectrogram64([x, x[:700]], 17)
    assert batch.shape == (2, 17, 161) and np.array_equal(batch[0], cut) and np.all(batch[1, 5:] == 0)
    np.testing.assert_allclose(batch[1, :5], ospec.log_spectrogram(x[:700], dtype=np.float64), rtol=0, atol=1e-12)
    silent = refs.log_spectrogram64(np.zeros(1000, np.float32))
    assert np.all(silent == 0.0)                                # 0 / (0 + eps)


def test_float32_frontend_is_the_same_formula():
    """The float32 CPU run differs from the float64 oracle by float32 rounding only."""
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(16000)).astype(np.float32)
    assert refs.log_spectrogram32(x).shape == (101, 161)
    assert refs.fp32_frontend_error(x, False) < 2e-5            # (the bounds the existing kernel test gives the kernel)
    assert refs.fp32_frontend_error(x, True) < 2e-4
    assert refs.log_spectrogram32(x, max_frames=17).shape == (17, 161)
