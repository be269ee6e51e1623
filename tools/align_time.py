#!/usr/bin/env python
"""Time one CTC forced-alignment launch (ds2_ctc_align) against the host reference, one JSON line.

    python tools/align_time.py [--reps 20] [--host-reps 1]

Input: B = 10 utterances x T = 746 frames x A = 29 of seeded, peaked softmax output, each aligned to a transcript of
L = 200 labels (the flagship minibatch's shape).  Device time: device events around one ``ops.ctc_align`` call (the
workspace allocation included), median of --reps after one warm-up.  Host time: tests/align_ref.py's float64 numpy
Viterbi over the same batch, the probabilities already on the host.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=1)
    args = ap.parse_args()
    import torch
    from ds2hip import ops
    from tests import align_ref
    assert torch.cuda.is_available(), 'align_time.py measures on the GPU'
    rng = np.random.default_rng(0)
    B, T, A, L = 10, 746, 29, 200
    labels = [[int(v) for v in rng.integers(1, A, size=L)] for _ in range(B)]
    x = rng.standard_normal((B, T, A)) * 0.5
    x[:, :, 0] += 5.0
    for b in range(B):                       # the transcript spelled out at sorted random frames
        for f, k in zip(np.sort(rng.choice(T, size=L, replace=False)), labels[b]):
            x[b, f, k] += 9.0
    e = np.exp(x - x.max(-1, keepdims=True))
    probs_h = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    probs = torch.from_numpy(probs_h).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')   # noqa: E731
    sizes, flat = i32([T] * B), i32([v for lab in labels for v in lab])
    offs, lens = i32([L * b for b in range(B)]), i32([L] * B)
    run = lambda: ops.ctc_align(probs, sizes, flat, offs, lens, L)      # noqa: E731
    out = run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    hs = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        ref = align_ref.align_batch(probs_h, [T] * B, labels)
        hs.append((time.perf_counter() - t0) * 1e3)
    dev_ms, host_ms = float(np.median(ts)), float(np.median(hs))
    print(json.dumps({'B': B, 'T': T, 'A': A, 'L': L, 'device_ms': round(dev_ms, 3), 'device_ms_min': round(min(ts), 3),
                      'per_frame_us': round(dev_ms * 1e3 / T, 3), 'host_ref_ms': round(host_ms, 1),
                      'speedup_vs_host_ref': round(host_ms / dev_ms, 1),
                      'same_states_as_host_ref': bool(np.array_equal(out[0].cpu().numpy(), ref[0]))}))


if __name__ == '__main__':
    main()
