"""Plain references for the small kernels around the training step, the decode head and the frontend (TEST INFRASTRUCTURE
ONLY): float64 numpy / torch or exact integer arithmetic, no call into the library.  tests/test_small_refs_cpu.py pins them
against torch and the oracle on the CPU; tests/test_small_kernels_gpu.py holds the HIP kernels to them."""
import numpy as np
import torch

from oracle import spectrogram as ospec


# ------------------------------------------------------------------------------------------- optimiser
def nesterov_clip_step(p, g, buf, grad_scale, max_norm, lr, momentum, first_step, clip=True, sumsq=None):
    """One ``clip_grad_norm_(max_norm)`` + ``SGD(momentum, nesterov=True)`` step on the gradient ``g * grad_scale``, in float64.

    The clip coefficient is ``min(1, max_norm / (norm + 1e-6))`` with the norm taken over ``g * |grad_scale|``; ``clip=False``
    leaves the gradient alone.  ``sumsq``: the sum of squares of ``g`` (before ``grad_scale``) to derive the norm from instead
    of computing it here -- a test hands in the value its kernel was given, so that the comparison is about the update.
    Returns ``(p_new, buf_new, coef)`` as float64; ``buf`` is ignored on the first step."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    coef = 1.0
    if clip:
        ss = float((g * g).sum()) if sumsq is None else float(sumsq)
        norm = np.sqrt(ss) * abs(float(grad_scale))
        coef = min(1.0, float(max_norm) / (norm + 1e-6))
    ge = g * (float(grad_scale) * coef)
    b = ge.copy() if first_step else float(momentum) * np.asarray(buf, np.float64) + ge
    return p - float(lr) * (ge + float(momentum) * b), b, coef


# ------------------------------------------------------------------------------------------- decode head
def softmax64(x):
    """Row softmax in float64; a row's ``-inf`` entries come out as exactly 0."""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def argmax_nan_first(x):
    """Row argmax with torch.max's order: NaN is the largest value and the first one wins; ties -> lowest index."""
    return np.argmax(np.asarray(x), axis=-1)


def collapse(best_row, size, blank):
    """Greedy CTC collapse of one row of per-frame labels: frame t < min(size, T) is kept iff its label is not ``blank`` and
    (t == 0 or it differs from frame t-1's label).  Returns (ids, offsets) as python lists."""
    ids, offs = [], []
    for t in range(min(int(size), len(best_row))):
        c = int(best_row[t])
        if c == blank or (t != 0 and c == int(best_row[t - 1])):
            continue
        ids.append(c)
        offs.append(t)
    return ids, offs


# ------------------------------------------------------------------------------------------- frontend
def _normalise(s, eps):
    if s.size < 2:
        return s
    return (s - s.mean()) / (s.std(ddof=1) + eps)


def log_spectrogram64(x, normalize=True, eps=1e-9, max_frames=None):
    """The oracle's frontend in float64 with the collate's truncation: the log-magnitudes of the first ``max_frames`` frames
    (all of them if None), normalised over exactly those frames.  (T, 161) float64."""
    s = np.log1p(ospec.stft_magnitude(x, dtype=np.float64))
    if max_frames is not None:
        s = s[:max_frames]
    return _normalise(s, eps) if normalize else s


def batch_log_spectrogram64(wavs, t_max, normalize=True, eps=1e-9):
    """(B, t_max, 161) float64: every clip cut to ``t_max`` frames, zero rows behind a shorter clip's own frames."""
    out = np.zeros((len(wavs), t_max, ospec.NBINS), np.float64)
    for i, w in enumerate(wavs):
        s = log_spectrogram64(w, normalize, eps, t_max)
        out[i, :s.shape[0]] = s
    return out


def log_spectrogram32(x, normalize=True, eps=1e-9, max_frames=None):
    """The same formula carried out in FLOAT32 on the CPU (torch.stft on float32 input with the symmetric Hann window and
    centre reflect padding, then log1p and the normalisation in float32): what a sound fp32 implementation loses against the
    float64 oracle on this input -- the yardstick a kernel's tolerance is taken from.  (T, 161) float32."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    win = torch.hann_window(ospec.FRAME, periodic=False, dtype=torch.float32)
    s = torch.stft(xt, ospec.FRAME, ospec.HOP, ospec.FRAME, win, center=True, pad_mode='reflect',
                   return_complex=True).abs().T
    s = torch.log1p(s)
    if max_frames is not None:
        s = s[:max_frames]
    if normalize and s.numel() > 1:
        s = (s - s.mean()) / (s.std() + np.float32(eps))
    return s.contiguous().numpy()


def fp32_frontend_error(x, normalize, eps=1e-9):
    """max |float32 CPU frontend - float64 oracle| on clip ``x``."""
    return float(np.abs(log_spectrogram32(x, normalize, eps).astype(np.float64) - log_spectrogram64(x, normalize, eps)).max())
