#!/usr/bin/env python
"""Time one banded CTC alignment launch (ds2_ctc_align_banded) at an hour's size against the host reference, one JSON line.

    python tools/align_long_time.py [--reps 3] [--leg-timeout 900] [--skip-host]

Input: T = 180 000 frames (an hour of 20 ms steps) x A = 29 of seeded, peaked softmax output -- blank-dominated, label l of
L = 50 000 spelled at frame floor(3.6 l) + a jitter of 0..2 frames -- aligned to that transcript on the diagonal band.  Legs,
each a child process of its own under its own time limit (a leg that fails ends the run: nothing is started after it):
W = 4096, W = 1024 and the library's widest band on the device (device events around one ``ops.ctc_align_banded`` call, the
workspace allocation included; median of --reps after one warm-up launch), and tests/align_banded_ref.py's windowed float64
numpy reference at W = 4096 on the same input.  There is no pass / fail time: nothing exists to compare with."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

T, A, L = 180000, 29, 50000


def inputs():
    rng = np.random.default_rng(0)
    labels = rng.integers(1, A, size=L)
    x = (rng.standard_normal((T, A)) * 0.5).astype(np.float32)
    x[:, 0] += 5.0
    at = (np.arange(L) * 18) // 5 + rng.integers(0, 3, size=L)
    x[at, labels] += 9.0
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), labels


def digest(score, states):
    return hashlib.sha1(np.asarray(states, dtype=np.int32).tobytes()).hexdigest()[:16], float(score)


def device_leg(w, reps):
    import torch
    from codes.align import band_margin, diagonal_band
    from ds2hip import lib, ops
    assert torch.cuda.is_available(), 'align_long_time.py measures on the GPU'
    w = lib.ALIGN_BAND_MAX if w == 'max' else int(w)
    probs_h, labels = inputs()
    probs = torch.from_numpy(probs_h).cuda()[None]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')   # noqa: E731
    lo = diagonal_band(T, 2 * L + 1, w)
    lo_d = lo.to('cuda', torch.int32)[None]
    args = (probs, i32([T]), i32(labels.tolist()), i32([0]), i32([L]), L, lo_d, w)
    out = ops.ctc_align_banded(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.ctc_align_banded(*args)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    states, score = out[0][0].cpu().numpy(), float(out[3][0])
    sha, score = digest(score, states)
    return {'W': w, 'device_ms': round(float(np.median(ts)), 2), 'device_ms_min': round(min(ts), 2),
            'per_frame_us': round(float(np.median(ts)) * 1e3 / T, 3), 'score': score,
            'band_margin': band_margin(states, lo, w, 2 * L + 1) if np.isfinite(score) else None, 'states_sha1': sha}


def host_leg(w):
    from tests import align_banded_ref as bref
    from tests import align_ref
    probs_h, labels = inputs()
    t0 = time.perf_counter()
    score, states = bref.windowed(align_ref.frame_terms(probs_h, False), labels.tolist(), bref.diagonal(T, 2 * L + 1, w), w)
    ms = (time.perf_counter() - t0) * 1e3
    sha, score = digest(score, states if states is not None else np.full(T, -1))
    return {'W': w, 'host_ref_ms': round(ms, 1), 'score': score, 'states_sha1': sha}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--leg-timeout', type=int, default=900, help='seconds per leg')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg is not None:
        kind, w = args.leg.split(':')
        print(json.dumps(device_leg(w, args.reps) if kind == 'device' else host_leg(int(w))))
        return
    legs = ['device:4096', 'device:1024', 'device:max'] + ([] if args.skip_host else ['host:4096'])
    res = {'T': T, 'A': A, 'L': L, 'legs': {}}
    for leg in legs:
        cmd = ['timeout', '-k', '10', str(args.leg_timeout), sys.executable, os.path.abspath(__file__), '--leg', leg,
               '--reps', str(args.reps)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            res['legs'][leg] = {'failed': out.returncode, 'stderr': out.stderr[-400:]}
            break
        res['legs'][leg] = json.loads(out.stdout.strip().splitlines()[-1])
    dev, host = res['legs'].get('device:4096', {}), res['legs'].get('host:4096', {})
    if 'device_ms' in dev and 'host_ref_ms' in host:
        res['speedup_vs_host_ref'] = round(host['host_ref_ms'] / dev['device_ms'], 1)
        res['same_states_as_host_ref'] = dev['states_sha1'] == host['states_sha1']
        res['score_minus_host_ref'] = dev['score'] - host['score']
    print(json.dumps(res))
    if any('failed' in v for v in res['legs'].values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
