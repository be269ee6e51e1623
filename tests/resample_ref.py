"""Float64 reference of the sample-rate conversion (include/ds2hip.h, "sample-rate conversion"; ds2hip/ops.py
resample_design / resample): the filter design, the sum over the definition, the quantisation rule and the output-length rule.
numpy only; nothing here is imported by the product."""
import math

import numpy as np

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)
LMK = {8000: (2, 1, 53), 11025: (640, 441, 53), 22050: (320, 441, 71), 24000: (2, 3, 77), 32000: (1, 2, 103),
       44100: (160, 441, 141), 48000: (1, 3, 153), 96000: (1, 6, 305)}


def ratio(rate_in, rate_out=16000):
    g = math.gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def kernel(x, c, zeros=24, beta=9.0):
    """The continuous filter h(x), x in input samples: c sinc(c x) times a Kaiser window that ends at zeros / c."""
    x = np.asarray(x, np.float64)
    a = np.abs(x) * c / zeros
    win = np.i0(beta * np.sqrt(np.maximum(1.0 - a * a, 0.0))) / np.i0(beta)
    return np.where(a > 1.0, 0.0, c * np.sinc(c * x) * win)


def cutoff(L, M, rolloff=0.95):
    return rolloff * min(1.0, L / M)


def design64(rate_in, rate_out=16000, zeros=24, rolloff=0.95, beta=9.0):
    """(L, M, taps) with taps (L, K) float64: taps[p][k] = h((k - half) - p / L).  Equal rates: the identity."""
    L, M = ratio(rate_in, rate_out)
    if L == M:
        return 1, 1, np.ones((1, 1), np.float64)
    c = cutoff(L, M, rolloff)
    half = int(math.ceil(zeros / c))
    K = 2 * half + 1
    u = (np.arange(K, dtype=np.float64)[None, :] - half) - np.arange(L, dtype=np.float64)[:, None] / L
    return L, M, kernel(u, c, zeros, beta)


def design(rate_in, rate_out=16000, zeros=24, rolloff=0.95, beta=9.0):
    """The table the device reads: design64 rounded to float32 once."""
    L, M, taps = design64(rate_in, rate_out, zeros, rolloff, beta)
    return L, M, taps.astype(np.float32)


def out_len(n_frames, L, M):
    return (int(n_frames) * L + M - 1) // M


def downmix(pcm, channels):
    """Interleaved int16 -> the exact integer channel sums, as float64."""
    pcm = np.asarray(pcm)
    assert pcm.size % channels == 0
    return pcm.astype(np.int64).reshape(-1, channels).sum(axis=1).astype(np.float64)


def convolve(s, L, M, taps, ms=None, absolute=False, origin=0, n=None):
    """y[m] = sum_k taps[p][k] s[i0 + k - h], t = m M, i0 = t // L, p = t % L, s zero outside the clip: the sum of the
    definition in float64, for every output (or the outputs ``ms``).  ``absolute``: the sum of |taps s| instead.
    ``origin``, ``n``: s holds only the frames [origin, origin + len(s)) of a clip of n frames (a window of a long clip); the
    outputs asked for must not need a frame of the clip outside it."""
    s = np.asarray(s, np.float64)
    taps = np.asarray(taps, np.float64)
    K = taps.shape[1]
    h = (K - 1) // 2
    n = len(s) if n is None else int(n)
    ms = np.arange(out_len(n, L, M), dtype=np.int64) if ms is None else np.asarray(ms, np.int64)
    y = np.zeros(len(ms), np.float64)
    step = max(1, (1 << 22) // K)
    for a in range(0, len(ms), step):
        t = ms[a:a + step] * M
        i0, p = t // L, t % L
        j = i0[:, None] + np.arange(K, dtype=np.int64)[None, :] - h
        inside = (j >= 0) & (j < n)
        w = j - origin
        assert ((w >= 0) & (w < len(s)))[inside].all(), 'the window does not hold every frame these outputs read'
        sv = np.where(inside, s[np.clip(w, 0, max(len(s) - 1, 0))] if len(s) else 0.0, 0.0)
        prod = taps[p] * sv
        y[a:a + step] = (np.abs(prod) if absolute else prod).sum(axis=1)
    return y


def direct(s, L, M, c, zeros=24, beta=9.0):
    """The definition without phases: y(m) = sum_j h(m M / L - j) s[j] over every sample of the clip."""
    s = np.asarray(s, np.float64)
    n = len(s)
    m = np.arange(out_len(n, L, M), dtype=np.float64)
    x = m[:, None] * M / L - np.arange(n, dtype=np.float64)[None, :]
    return (kernel(x, c, zeros, beta) * s[None, :]).sum(axis=1)


def quantise(y, channels=1):
    """(int16 result, v): v = y / channels in float64; rint is round-half-to-even."""
    v = np.asarray(y, np.float64) / channels
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16), v


def resample(pcm, channels, L, M, taps):
    """One clip, interleaved int16 in, mono int16 out."""
    return quantise(convolve(downmix(pcm, channels), L, M, taps), channels)[0]


def resample_flat(pcm, offsets, channels, L, M, taps):
    """The flat form: (concatenated outputs, out_offsets)."""
    outs = [resample(pcm[offsets[b]:offsets[b + 1]], channels, L, M, taps) for b in range(len(offsets) - 1)]
    offs = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64)
    return (np.concatenate(outs) if outs else np.zeros(0, np.int16)), offs
