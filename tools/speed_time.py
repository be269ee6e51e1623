#!/usr/bin/env python
"""Time speed perturbation of a minibatch (ds2_resample_var) against the same work done with ds2_resample, one JSON line.

    python tools/speed_time.py [--reps 20]

Input: B = 10 clips of 15 s (240 000 samples) of seeded int16 noise, factors cycling 0.9 / 1.0 / 1.1 (``ops.speed_design``).
``var_ms``: device events around one ``ops.resample_var`` call (its one small upload and the allocation of its output
included), median of --reps after warm-up.  ``var_wall_ms`` / ``grouped_wall_ms``: wall clock from an idle device to an idle
device (a synchronise on either side) of that call, and of the same work in the only form ``ds2_resample`` allows: per factor
a gather of its clips, one ``ops.resample`` call -- which waits on the stream to read the offsets back -- and a gather of the
outputs back into batch order; the two alternate in the same run.  ``grouped_equal``: the two forms gave the same bits.
``copy_ms``: a device-to-device copy that moves the same number of bytes (half of them read, half written);
``copy_share``: ``copy_ms / var_ms``.  ``frontend_ms`` / ``frontend_speed_ms``: ``BatchSpectrogram`` on the same clips with a
drawn tempo and gain each, without and with the stage (device events, alternating)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

B, N, FACTORS = 10, 240000, (0.9, 1.0, 1.1)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    import torch
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, SpeedPerturb
    from ds2hip import ops
    assert torch.cuda.is_available(), 'speed_time.py measures on the GPU'
    rng = np.random.RandomState(0)
    clips = [torch.from_numpy((rng.standard_normal(N) * 3277).clip(-32768, 32767).astype(np.int16)) for _ in range(B)]
    pcm = torch.cat(clips).cuda()
    offs = [N * b for b in range(B + 1)]
    sp = SpeedPerturb(factors=FACTORS)
    draws = [b % len(FACTORS) for b in range(B)]
    ids, tables = sp.table_ids(draws), sp.tables()
    tables_d = [(L, M, torch.from_numpy(np.array(taps)).cuda()) for L, M, taps in tables]      # (ds2_resample's, uploaded once)

    def var():
        return ops.resample_var(pcm, offs, ids, tables)

    def grouped():
        parts = [None] * B
        for t in sorted(set(ids)):
            members = [b for b in range(B) if ids[b] == t]
            flat = torch.cat([pcm[offs[b]:offs[b + 1]] for b in members])
            out, out_off = ops.resample(flat, [N * i for i in range(len(members) + 1)], 16000, taps=tables_d[t])
            for i, b in enumerate(members):
                parts[b] = out[out_off[i]:out_off[i + 1]]
        return torch.cat(parts)

    out, out_off = var()
    equal = bool(torch.equal(out, grouped()))
    half = (pcm.numel() + out.numel()) // 2                          # a copy that moves the same bytes: half read, half written
    src = torch.empty(half, dtype=torch.int16, device='cuda').copy_(pcm.repeat(2)[:half])
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)                                    # noqa: E731
    for f in (var, grouped, copy):
        for _ in range(3):
            _timed(f)
    t_var, t_copy, w_var, w_grouped = [], [], [], []
    for _ in range(args.reps):                                       # alternating: all see the same machine
        t_var.append(_timed(var))
        t_copy.append(_timed(copy))
        w_var.append(_wall(var))
        w_grouped.append(_wall(grouped))

    tempos, gains = [float(v) for v in rng.uniform(0.85, 1.15, B)], [float(v) for v in rng.uniform(-6, 8, B)]
    plain = RawAudioBatch.from_clips([PCMClip(p, t, g) for p, t, g in zip(clips, tempos, gains)]).to('cuda')
    fast = RawAudioBatch.from_clips([PCMClip(p, t, g, speed=d) for p, t, g, d in zip(clips, tempos, gains, draws)]).to('cuda')
    front = BatchSpectrogram(speed=sp)
    for _ in range(3):
        front(plain), front(fast)
    torch.cuda.synchronize()
    without, with_ = [], []
    for _ in range(args.reps):
        without.append(_timed(lambda: front(plain)))
        with_.append(_timed(lambda: front(fast)))
    med = lambda v: float(np.median(v))                              # noqa: E731
    print(json.dumps({'B': B, 'clip_samples': N, 'factors': list(FACTORS), 'reps': args.reps,
                      'tables': [[t[0], t[1], int(t[2].shape[1])] for t in tables], 'outputs': int(out_off[-1]),
                      'var_ms': round(med(t_var), 4), 'var_ms_min': round(min(t_var), 4),
                      'var_wall_ms': round(med(w_var), 4), 'grouped_wall_ms': round(med(w_grouped), 4),
                      'grouped_wall_ms_min': round(min(w_grouped), 4), 'var_wall_ms_min': round(min(w_var), 4),
                      'grouped_over_var': round(med(w_grouped) / med(w_var), 2), 'grouped_equal': equal,
                      'bytes': 4 * half, 'copy_ms': round(med(t_copy), 4), 'copy_share': round(med(t_copy) / med(t_var), 3),
                      'gmacs': round(sum((out_off[b + 1] - out_off[b]) * tables[ids[b]][2].shape[1] for b in range(B))
                                     / (med(t_var) * 1e-3) / 1e9, 1),
                      'frontend_ms': round(med(without), 3), 'frontend_speed_ms': round(med(with_), 3),
                      'frontend_ms_spread': [round(min(without), 3), round(max(without), 3)],
                      'speed_share_of_frontend': round((med(with_) - med(without)) / med(without), 4)}))


if __name__ == '__main__':
    main()
