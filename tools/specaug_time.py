#!/usr/bin/env python
"""Time one SpecAugment launch (ds2_spec_augment) and the frontend with and without it, one JSON line.

    python tools/specaug_time.py [--reps 50]

Input: B = 10 clips of 15 s (240 000 samples, 1501 frames) of seeded white noise; the draws are SpecAugment's own under a
seed, with the default settings (two frequency masks up to 27 bins, two time masks up to 100 frames) and, for the warp
leg, ``time_warp = 80``.  ``mask_ms``: device events around one ``ops.spec_augment`` call without a warp, in place (its
small upload included), median of --reps after warm-up; ``warp_ms``: the same with the warp, into a second tensor that is
allocated once outside the timed region.  ``bytes``: the spectrogram batch, B x 1501 x 161 floats -- the mask-only launch
stores a fraction of it and loads nothing, the warp launch loads up to twice and stores once.  ``frontend_ms`` /
``frontend_specaug_ms`` / ``frontend_specaug_warp_ms``: ``BatchSpectrogram`` on the same clips as int16 with a drawn
tempo and gain each (decode, WSOLA, gain, spectrogram), without the draws, with them, and with them and a warp,
alternating so that all three see the same machine.
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
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, SpecAugment
    from ds2hip import ops
    assert torch.cuda.is_available(), 'specaug_time.py measures on the GPU'
    B, N, WARP = 10, 240000, 80
    T = 1 + N // 160
    rng = np.random.RandomState(0)
    masks, warped = SpecAugment(), SpecAugment(time_warp=WARP)
    draws_m, draws_w = [masks.draw(rng) for _ in range(B)], [warped.draw(rng) for _ in range(B)]

    gen = torch.Generator(device='cuda').manual_seed(0)
    spect = torch.randn(B, T, 161, device='cuda', generator=gen)
    _, fm, tm = masks.params(draws_m, [T] * B)
    wp, fmw, tmw = warped.params(draws_w, [T] * B)
    work, out = spect.clone(), torch.empty_like(spect)
    mask = lambda: ops.spec_augment(work, [T] * B, None, fm, tm, 0.0)                     # noqa: E731
    warp = lambda: ops.spec_augment(spect, [T] * B, wp, fmw, tmw, 0.0, out=out)           # noqa: E731
    _timed(mask, 5), _timed(warp, 5)
    t_mask, t_warp = _timed(mask, args.reps), _timed(warp, args.reps)
    masked = float((work == 0).sum()) / work.numel()

    pcm = [torch.from_numpy((rng.standard_normal(N) * 3277).clip(-32768, 32767).astype(np.int16)) for _ in range(B)]
    tempos, gains = [float(v) for v in rng.uniform(0.85, 1.15, B)], [float(v) for v in rng.uniform(-6, 8, B)]
    batch = lambda draws: RawAudioBatch.from_clips(                                        # noqa: E731
        [PCMClip(p, t, g, None, d) for p, t, g, d in zip(pcm, tempos, gains, draws)]).to('cuda')
    plain, with_m, with_w = batch([None] * B), batch(draws_m), batch(draws_w)
    front_m, front_w = BatchSpectrogram(spec_augment=masks), BatchSpectrogram(spec_augment=warped)
    for _ in range(3):
        front_m(plain), front_m(with_m), front_w(with_w)
    torch.cuda.synchronize()
    f0, f1, f2 = [], [], []
    for _ in range(max(args.reps // 2, 5)):                       # alternating: all three see the same machine
        f0 += _timed(lambda: front_m(plain), 1)
        f1 += _timed(lambda: front_m(with_m), 1)
        f2 += _timed(lambda: front_w(with_w), 1)
    med = lambda v: float(np.median(v))                                                    # noqa: E731
    nbytes = B * T * 161 * 4
    print(json.dumps({'B': B, 'frames': T, 'reps': args.reps, 'bytes': nbytes, 'time_warp': WARP,
                      'masked_share': round(masked, 4),
                      'mask_ms': round(med(t_mask), 4), 'mask_ms_min': round(min(t_mask), 4),
                      'warp_ms': round(med(t_warp), 4), 'warp_ms_min': round(min(t_warp), 4),
                      'warp_gbps_moved_at_least': round(2 * nbytes / (med(t_warp) * 1e-3) / 1e9, 1),
                      'frontend_ms': round(med(f0), 3), 'frontend_specaug_ms': round(med(f1), 3),
                      'frontend_specaug_warp_ms': round(med(f2), 3),
                      'frontend_ms_spread': [round(min(f0), 3), round(max(f0), 3)],
                      'specaug_share_of_frontend': round((med(f1) - med(f0)) / med(f0), 4),
                      'specaug_warp_share_of_frontend': round((med(f2) - med(f0)) / med(f0), 4)}))


if __name__ == '__main__':
    main()
