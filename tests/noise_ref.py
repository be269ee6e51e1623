"""Numpy float64 restatement of the noise-injection stage (``ds2_noise_mix``, include/ds2hip.h "noise injection"), the
reference the device kernel is held to, plus the host-side start rule and a writer of small int16 WAV directories.

    nz[i]  = float32(bank[lo + (start + i) mod length]) * float32(scale)        one float32 rounding, as the kernel
    coef   = level * sqrt(sum wav^2 / n) / sqrt(sum nz^2 / n)                   float64; 0 when the crop is silent
    out[i] = wav[i] + coef * nz[i]                                              float64

Nothing here imports the product."""
import os
import wave

import numpy as np


def noise_crop(bank16, lo, length, start, n, scale):
    """The n noise samples a clip sees, as float32 (the recording repeats when it is shorter than the clip)."""
    idx = int(lo) + (int(start) + np.arange(int(n), dtype=np.int64)) % int(length)
    return np.asarray(bank16)[idx].astype(np.float32) * np.float32(scale)


def mix_ref(wav32, bank16, lo, length, start, level, scale):
    """One clip.  wav32: float32 samples; the draw as ``ds2_noise_mix`` takes it (length 0 = no noise; ``level`` is
    rounded to float32 first, as the C ABI carries it).  Returns (out float64 (n,), coef float64)."""
    wav = np.asarray(wav32, np.float32).astype(np.float64)
    n = wav.size
    if int(length) == 0 or n == 0:
        return wav.copy(), 0.0
    assert 0 <= int(start) < int(length)
    nz = noise_crop(bank16, lo, length, start, n, scale).astype(np.float64)
    ex, en = float(np.dot(wav, wav)), float(np.dot(nz, nz))
    coef = float(np.float32(level)) * np.sqrt(ex / n) / np.sqrt(en / n) if en > 0.0 else 0.0
    return wav + coef * nz, coef


def start_rule(u, noise_len, n):
    """First sample of the crop from the uniform draw u in [0, 1): floor(u * (noise_len - n)) when the recording is at
    least as long as the clip, floor(u * noise_len) (with wrap-around) otherwise."""
    noise_len, n = int(noise_len), int(n)
    if noise_len >= n:
        return min(int(np.floor(float(u) * (noise_len - n))), noise_len - n, noise_len - 1)
    return min(int(np.floor(float(u) * noise_len)), noise_len - 1)


def write_wav(path, samples, rate=16000, channels=1, width=2):
    """samples: int16 array (interleaved when channels > 1)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples, dtype='<i2').tobytes())
    return path


def write_noise_dir(root, lengths=(4000, 2500, 700), seed=0, amplitude=3000):
    """A small noise set: ``root/b/n1.wav``, ``root/a/n0.wav``, ``root/n2.wav`` ... written in an order that is NOT the sorted
    one.  Returns ({relative path: int16 samples}); the bank is the samples in sorted order of the full paths."""
    rng = np.random.RandomState(seed)
    subdirs = ['b', 'a', '']
    out = {}
    for k, n in enumerate(lengths):
        rel = os.path.join(subdirs[k % 3], 'n%d.wav' % k)
        x = (rng.standard_normal(n) * amplitude).clip(-32768, 32767).astype(np.int16)
        write_wav(os.path.join(root, rel), x)
        out[rel] = x
    return out


def bank_of(root, files):
    """(bank int16, starts, lengths) of ``write_noise_dir``'s result in the listing order NoiseInjection must use."""
    order = sorted(files, key=lambda rel: os.path.join(root, rel))
    lengths = [len(files[r]) for r in order]
    starts = [0] + list(np.cumsum(lengths[:-1]))
    return np.concatenate([files[r] for r in order]), [int(s) for s in starts], lengths, order
