#!/usr/bin/env python
"""Time the segmentation of a one-hour recording (ds2_vad_segment), one JSON line.

    python tools/vad_time.py [--reps 20] [--seconds 3600]

Input: a seeded recording of 57.6 M int16 samples (one hour at 16 kHz): white noise at -55 dBFS with bursts at -20 dBFS of
0.5 .. 20 s (some longer than the 15 s a segment may have, so they are split) between gaps of 0.2 .. 3 s.
``vad_ms``: device events around one ``ops.vad_segment`` call with the Segmenter's default rule and a workspace allocated
once outside the timed region -- three launches and the one readback -- median of --reps after warm-up; ``vad_launches_ms``
the same around the bare ``ds2_vad_segment`` call, without the readback.  ``pcm_gbps``: the 2 bytes per sample over
``vad_launches_ms`` (the energy pass is the only one that reads them).  ``pcm16_to_float_ms``: ``ds2_pcm16_to_float`` over
the same buffer in the same run, alternating with the segmentation: it reads the same bytes (and writes twice as many).
``host_ms``: tests/vad_ref.py (numpy block energies, Python integers from there) on the host, once; ``host_energy_ms``:
its numpy energy pass alone.  ``equal_to_reference``: the device's segments and info against it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)


def recording(seconds, seed=0):
    rng = np.random.default_rng(seed)
    n = int(seconds * 16000)
    lens, amps, at, loud = [], [], 0, False
    while at < n:
        k = int(rng.uniform(0.5, 20.0) * 16000) if loud else int(rng.uniform(0.2, 3.0) * 16000)
        lens.append(min(k, n - at))
        amps.append(3276.7 if loud else 58.27)                       # -20 and -55 dBFS rms
        at += k
        loud = not loud
    x = rng.standard_normal(n, dtype=np.float32)
    x *= np.repeat(np.asarray(amps, np.float32), lens)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--seconds', type=float, default=3600.0)
    args = ap.parse_args()
    import torch
    from codes.segment import Segmenter
    from ds2hip import lib, ops
    from tests import vad_ref
    assert torch.cuda.is_available(), 'vad_time.py measures on the GPU'
    x = recording(args.seconds)
    n, nb = len(x), -(-len(x) // 160)
    s = Segmenter()
    rule = (s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    pcm = torch.from_numpy(x).to('cuda')
    ws = torch.empty(lib.query('ds2_vad_segment_ws_bytes', n), dtype=torch.uint8, device='cuda')
    cap = nb // min(s.min_speech, (s.max_len + 1) // 2) + 1
    out = torch.empty(8 + 2 * cap, dtype=torch.int32, device='cuda')
    wav = torch.empty(n, dtype=torch.float32, device='cuda')
    full = lambda: ops.vad_segment(pcm, *rule, ws=ws)                                                   # noqa: E731
    bare = lambda: lib.call('ds2_vad_segment', pcm, n, *rule, ws, ws.numel(), out[8:], cap, out[:8])    # noqa: E731
    conv = lambda: lib.call('ds2_pcm16_to_float', pcm, n, ops.UNIT_SCALE, wav)                          # noqa: E731
    for f in (full, bare, conv):
        _timed(f, 3)
    t_full, t_bare, t_conv = [], [], []
    for _ in range(args.reps):                                      # alternating: all three see the same machine
        t_full += _timed(full, 1)
        t_bare += _timed(bare, 1)
        t_conv += _timed(conv, 1)
    segs, info = full()

    t0 = time.perf_counter()
    vad_ref.block_energies(x)
    t_energy = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = vad_ref.vad_ref(x, *rule)
    t_host = time.perf_counter() - t0
    equal = bool(np.array_equal(segs.numpy(), want['segs'])) and \
        [info[k] for k in ('n_seg', 'floor_bin', 'thr', 'speech_blocks', 'nb')] == want['info'][:5]
    med = lambda v: float(np.median(v))                                                                 # noqa: E731
    lengths = (want['segs'][:, 1] - want['segs'][:, 0]) / 100.0
    print(json.dumps({'samples': n, 'blocks': nb, 'reps': args.reps, 'segments': int(info['n_seg']),
                      'longest_segment_s': float(lengths.max()) if len(lengths) else 0.0,
                      'speech_seconds': info['speech_blocks'] / 100.0, 'floor_bin': info['floor_bin'], 'thr': info['thr'],
                      'ws_bytes': int(ws.numel()),
                      'vad_ms': round(med(t_full), 4), 'vad_ms_min': round(min(t_full), 4),
                      'vad_launches_ms': round(med(t_bare), 4), 'vad_launches_ms_min': round(min(t_bare), 4),
                      'pcm_bytes': 2 * n, 'pcm_gbps': round(2 * n / (med(t_bare) * 1e-3) / 1e9, 1),
                      'pcm16_to_float_ms': round(med(t_conv), 4), 'pcm16_to_float_ms_min': round(min(t_conv), 4),
                      'pcm16_to_float_read_gbps': round(2 * n / (med(t_conv) * 1e-3) / 1e9, 1),
                      'host_ms': round(1e3 * t_host, 1), 'host_energy_ms': round(1e3 * t_energy, 1),
                      'equal_to_reference': equal}))


if __name__ == '__main__':
    main()
