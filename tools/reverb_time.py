#!/usr/bin/env python
"""Time one reverberation launch (ds2_reverb), its plain vector-ALU form, and the frontend with and without the stage: one
JSON line.

    python tools/reverb_time.py [--reps 20]

Input: B = 10 clips of 15 s (240 000 samples) of seeded white noise, EVERY clip drawn, each with its own synthetic RIR of
K = 8000 taps (0.5 s).  ``reverb_ms``: device events around one ``ops.reverb`` call with ``keep_level`` (its small upload and
the scale kernel included; the output buffer and the workspace are the caller's), median of --reps after warm-up.
``tflops`` = 2 sum(n K) / reverb_ms and ``share_of_fp32_matrix_peak`` = that over 157.3 TF.  ``valu_ms``: the same call on the
same input in a child process that runs with DS2_REVERB_FORM=valu (the vector-ALU form of the same sum).
``frontend_ms`` / ``frontend_reverb_ms``: ``BatchSpectrogram`` on the same clips as int16 with a drawn tempo and gain each
(decode, WSOLA, gain, spectrogram), without draws and with draws at the default ``prob``, alternating; the draws change from
one repetition to the next through ten seeded sets (``drawn_clips_of_100``: how many of their 100 clips got an RIR), so the
median is over batches with two, three, four ... convolved clips as training sees them.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

B, N, K, FILES, PEAK_TF = 10, 240000, 8000, 16, 157.3


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


def _bank(rng):
    t = np.arange(K) / 16000.0
    h = rng.standard_normal((FILES, K)) * np.exp(-6.907755278982137 * t / 0.5) * 0.3
    h[:, 0] = 1.0
    return h.astype(np.float32)


def _launch_ms(reps):
    import torch
    from ds2hip import lib, ops
    rng = np.random.RandomState(0)
    bank = torch.from_numpy(_bank(rng).reshape(-1)).cuda()
    wav = torch.from_numpy((rng.standard_normal(B * N) * 0.1).astype(np.float32)).cuda()
    offs = [N * b for b in range(B + 1)]
    lo, ln = [K * (b % FILES) for b in range(B)], [K] * B
    out = torch.empty_like(wav)
    ws = torch.empty(lib.query('ds2_reverb_ws_bytes', B, N), dtype=torch.uint8, device='cuda')
    run = lambda: ops.reverb(wav, offs, bank, lo, ln, True, out=out, ws=ws)      # noqa: E731
    _timed(run, 3)
    return _timed(run, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--launch-only', action='store_true', help='print the launch times as JSON and exit (the child run)')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'reverb_time.py measures on the GPU'
    if args.launch_only:
        print(json.dumps(_launch_ms(args.reps)))
        return
    ts = _launch_ms(args.reps)
    # the vector-ALU form: a fresh child (the library reads the switch at every call, but the parent stays as it was)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--launch-only', '--reps', str(max(args.reps // 4, 3))],
                           capture_output=True, text=True, env=dict(os.environ, DS2_REVERB_FORM='valu'), timeout=900)
    assert child.returncode == 0, child.stderr[-2000:]
    valu = json.loads(child.stdout.strip().splitlines()[-1])

    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, Reverb
    rng = np.random.RandomState(1)
    rv = Reverb.__new__(Reverb)              # a Reverb over a synthetic bank without files on disk
    rv.__setstate__(dict(path='<synthetic>', sample_rate=16000, prob=0.3, max_rir_seconds=0.5, max_bank_seconds=600,
                         device='cuda', max_taps=K, paths=['%02d.wav' % i for i in range(FILES)],
                         lengths=[K] * FILES, starts=[K * i for i in range(FILES)], _banks={}))
    rv._banks[torch.device('cuda', torch.cuda.current_device())] = torch.from_numpy(_bank(rng).reshape(-1)).cuda()
    pcm = [torch.from_numpy((rng.standard_normal(N) * 3277).clip(-32768, 32767).astype(np.int16)) for _ in range(B)]
    tempos, gains = [float(v) for v in rng.uniform(0.85, 1.15, B)], [float(v) for v in rng.uniform(-6, 8, B)]
    draw_sets = [[rv.draw(rng) for _ in range(B)] for _ in range(10)]
    plain = RawAudioBatch.from_clips([PCMClip(p, t, g) for p, t, g in zip(pcm, tempos, gains)]).to('cuda')
    wets = [RawAudioBatch.from_clips([PCMClip(p, t, g, None, None, d) for p, t, g, d in zip(pcm, tempos, gains, draws)]).to('cuda')
            for draws in draw_sets]
    front = BatchSpectrogram(reverb=rv)
    for wet in wets[:3]:
        front(plain), front(wet)
    torch.cuda.synchronize()
    without, with_ = [], []
    for i in range(max(args.reps // 10, 1) * 10):                 # alternating: both see the same machine
        without += _timed(lambda: front(plain), 1)
        with_ += _timed(lambda: front(wets[i % 10]), 1)
    flops = 2.0 * B * N * K
    ms, vms, f0, f1 = float(np.median(ts)), float(np.median(valu)), float(np.median(without)), float(np.median(with_))
    tf = flops / (ms * 1e-3) / 1e12
    print(json.dumps({'B': B, 'clip_samples': N, 'taps': K, 'reps': args.reps, 'reverb_ms': round(ms, 4),
                      'reverb_ms_min': round(min(ts), 4), 'flop': flops, 'tflops': round(tf, 2),
                      'share_of_fp32_matrix_peak': round(tf / PEAK_TF, 4), 'valu_ms': round(vms, 4),
                      'valu_ms_min': round(min(valu), 4), 'mfma_over_valu_speedup': round(vms / ms, 3),
                      'prob': rv.prob, 'drawn_clips_of_100': sum(d is not None for draws in draw_sets for d in draws),
                      'frontend_ms': round(f0, 3), 'frontend_reverb_ms': round(f1, 3),
                      'frontend_ms_spread': [round(min(without), 3), round(max(without), 3)],
                      'reverb_share_of_frontend': round((f1 - f0) / f0, 4)}))


if __name__ == '__main__':
    main()
