#!/usr/bin/env python
"""Time one noise-mixing launch (ds2_noise_mix) and the frontend with and without it, one JSON line.

    python tools/noise_time.py [--reps 50]

Input: B = 10 clips of 15 s (240 000 samples) of seeded white noise, each mixed with a crop at a seeded position of a
one-hour int16 bank (60 recordings of 60 s, seeded, generated on the device: 115 MB).  ``mix_ms``: device events around one
``ops.noise_mix`` call in place (its small upload and workspace allocation included), median of --reps after warm-up.
``bytes``: what the two kernels must move -- per sample 4 B of speech and 2 B of noise read twice (energy, then mix) and 4 B
written -- and ``gbps`` = bytes / mix_ms.  ``frontend_ms`` / ``frontend_noise_ms``: ``BatchSpectrogram`` on the same clips
as int16 with a drawn tempo and gain each (decode, WSOLA, gain, spectrogram), without and with the noise draws, alternating.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    import torch
    from codes.transforms import BatchSpectrogram, NoiseInjection, PCMClip, RawAudioBatch
    from ds2hip import ops
    assert torch.cuda.is_available(), 'noise_time.py measures on the GPU'
    B, N, RATE, FILES, FILE_LEN = 10, 240000, 16000, 60, 60 * 16000
    rng = np.random.RandomState(0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    bank = (torch.randn(FILES * FILE_LEN, device='cuda', generator=gen) * 2500).clamp_(-32768, 32767).to(torch.int16)
    # a NoiseInjection over that bank without an hour of files on disk: the description a directory listing would give
    ni = NoiseInjection.__new__(NoiseInjection)
    ni.__setstate__(dict(path='<synthetic>', sample_rate=RATE, prob=1.0, noise_levels=(0.0, 0.5), device='cuda',
                         max_bank_seconds=3600, scale=ops.UNIT_SCALE, paths=['%02d.wav' % i for i in range(FILES)],
                         lengths=[FILE_LEN] * FILES, starts=[i * FILE_LEN for i in range(FILES)], _banks={}))
    ni._banks[torch.device('cuda', torch.cuda.current_device())] = bank
    draws = [(int(rng.randint(FILES)), float(rng.uniform(0.0, 0.5)), float(rng.uniform())) for _ in range(B)]

    pcm = [torch.from_numpy((rng.standard_normal(N) * 3277).clip(-32768, 32767).astype(np.int16)) for _ in range(B)]
    flat, offs = ops.decode_augment(torch.cat(pcm).cuda(), [N * b for b in range(B + 1)])
    lo, ln, st, lv = ni.params(draws, [N] * B)
    work = flat.clone()
    mix = lambda: ops.noise_mix(work, offs, bank, lo, ln, st, lv, ops.UNIT_SCALE, out=work)      # noqa: E731
    _timed(mix, 5)
    ts = _timed(mix, args.reps)

    tempos, gains = [float(v) for v in rng.uniform(0.85, 1.15, B)], [float(v) for v in rng.uniform(-6, 8, B)]
    plain = RawAudioBatch.from_clips([PCMClip(p, t, g) for p, t, g in zip(pcm, tempos, gains)]).to('cuda')
    noisy = RawAudioBatch.from_clips([PCMClip(p, t, g, d) for p, t, g, d in zip(pcm, tempos, gains, draws)]).to('cuda')
    front = BatchSpectrogram(noise=ni)
    for _ in range(3):
        front(plain), front(noisy)
    torch.cuda.synchronize()
    without, with_ = [], []
    for _ in range(max(args.reps // 2, 5)):                       # alternating: both see the same machine
        without += _timed(lambda: front(plain), 1)
        with_ += _timed(lambda: front(noisy), 1)
    nbytes = B * N * (2 * (4 + 2) + 4)
    mix_ms, f0, f1 = float(np.median(ts)), float(np.median(without)), float(np.median(with_))
    print(json.dumps({'B': B, 'clip_samples': N, 'bank_seconds': FILES * FILE_LEN // RATE, 'reps': args.reps,
                      'mix_ms': round(mix_ms, 4), 'mix_ms_min': round(min(ts), 4), 'bytes': nbytes,
                      'gbps': round(nbytes / (mix_ms * 1e-3) / 1e9, 1), 'gbps_at_min': round(nbytes / (min(ts) * 1e-3) / 1e9, 1),
                      'frontend_ms': round(f0, 3), 'frontend_noise_ms': round(f1, 3),
                      'frontend_ms_spread': [round(min(without), 3), round(max(without), 3)],
                      'noise_share_of_frontend': round((f1 - f0) / f0, 4)}))


if __name__ == '__main__':
    main()
