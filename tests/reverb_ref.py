"""Numpy float64 restatement of the reverberation stage (``ds2_reverb``, include/ds2hip.h "reverberation"), the reference
the device kernel is held to, plus the bank rule and helpers that make test inputs.

    h      = s[p : p + max_taps] / s[p],  s = int16 / 32768,  p = first argmax |s|;  trailing zeros stripped;  float32
    y[n]   = sum_{k=0}^{min(n, K-1)} h[k] x[n-k]         n in [0, N): the tail is cut, the history before the clip is zero
    S[n]   = sum_k |h[k]| |x[n-k]|                        the scale every error bound is relative to
    gain   = sqrt(sum x^2 / sum y^2)                      1 when sum y^2 == 0 or the quotient is not finite

Nothing here imports the product."""
import os

import numpy as np

DIRECT_LIMIT = 1 << 22                  # N * K up to which conv_ref convolves directly


def rir_rule(pcm16, max_taps):
    """The bank rule for one file's int16 samples -> float32 taps (ValueError for an empty or all-zero file)."""
    s = np.asarray(pcm16, np.int16).astype(np.float64) / 32768.0
    if s.size == 0 or not np.any(s != 0):
        raise ValueError('no impulse')
    p = int(np.flatnonzero(np.abs(s) == np.abs(s).max())[0])
    h = s[p:p + int(max_taps)] / s[p]
    last = int(np.flatnonzero(h != 0)[-1])
    return h[:last + 1].astype(np.float32)


def conv_direct(x, h):
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    return np.convolve(x, h)[:x.size] if x.size and h.size else np.zeros(x.size)


def conv_fft(x, h):
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if not (x.size and h.size):
        return np.zeros(x.size)
    n = 1
    while n < x.size + h.size - 1:
        n *= 2
    return np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)[:x.size]


def conv_ref(x, h):
    """y (float64, len(x)): direct for small shapes, FFT for long ones."""
    return conv_direct(x, h) if len(x) * len(h) <= DIRECT_LIMIT else conv_fft(x, h)


def abs_sum(x, h):
    """S[n] = sum_k |h[k]| |x[n-k]|."""
    return conv_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(h, np.float64)))


def gain_ref(x32, y32):
    """The level gain in float64 from the float32 clip and the float32 convolution."""
    x, y = np.asarray(x32, np.float32).astype(np.float64), np.asarray(y32, np.float32).astype(np.float64)
    ex, ey = float(np.dot(x, x)), float(np.dot(y, y))
    if not ey > 0.0:
        return 1.0
    with np.errstate(all='ignore'):
        g = np.sqrt(ex / ey)
        finite = np.isfinite(np.float32(g))
    return float(g) if finite else 1.0


def chain32(x32, h32):
    """The same sum carried in float32 on the CPU in tap order: acc += h[k] * x_shifted, k = 0 .. K-1 (two roundings per
    tap).  The yardstick for the kernel's rounding error."""
    x, h = np.asarray(x32, np.float32), np.asarray(h32, np.float32)
    acc = np.zeros(x.size, np.float32)
    for k in range(min(h.size, x.size)):
        acc[k:] += h[k] * x[:x.size - k]
    return acc


def synth_rir_taps(k, rt60, seed):
    """A make_rir-style RIR of exactly ``k`` float32 taps: h[0] = 1, then exponentially decaying Gaussian noise."""
    rng = np.random.RandomState(seed)
    t = np.arange(k) / 16000.0
    h = rng.standard_normal(k) * np.exp(-6.907755278982137 * t / rt60) * 0.3
    h[0] = 1.0
    if k > 1 and h[-1] == 0:
        h[-1] = 1e-4
    return h.astype(np.float32)


def speech_like(n, seed, scale=1.0 / 32768.0):
    """A 16-bit clip with speech-like dynamics (amplitude-modulated coloured noise) times the amplitude scale, float32."""
    rng = np.random.RandomState(seed)
    w = rng.standard_normal(n + 8)
    c = np.convolve(w, np.ones(8) / 8.0)[8:n + 8]
    env = 0.05 + np.abs(np.sin(np.arange(n) * (2 * np.pi / 3000.0) + rng.uniform(0, 6)))
    q = np.round(np.clip(c * env * 12000.0, -32768, 32767))
    return (q.astype(np.float32) * np.float32(scale)).astype(np.float32)


def write_rir_dir(root, files):
    """files: {relative path: int16 samples} -> written as 16-bit mono 16 kHz WAV."""
    from tests.noise_ref import write_wav
    for rel, x in files.items():
        write_wav(os.path.join(root, rel), x)
    return root
