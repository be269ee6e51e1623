#!/usr/bin/env python
"""Time one keyword-search call (ds2_ctc_keyword_search) beside the host reference, one JSON line.

    python tools/kws_time.py [--reps 20]

Input: B = 32 segments x T = 746 frames x A = 29 of seeded log-softmax output and K = 100 keywords of 8 labels, thresholds
at -4 per label, max_hits = 4.  Device time: device events around one ``ops.keyword_search`` call (both launches and the
allocation of workspace and outputs included), median of --reps after one warm-up.  Host time: tests/kws_ref.py on a SUBSET
of the pairs -- the 32 pairs (b, (3 b) mod K), one per segment -- scaled to all B K pairs; the device result is compared
with the reference on that subset."""
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
    args = ap.parse_args()
    import torch
    from ds2hip import ops
    from tests import kws_ref
    assert torch.cuda.is_available(), 'kws_time.py measures on the GPU'
    rng = np.random.default_rng(0)
    B, T, A, K, L, max_hits = 32, 746, 29, 100, 8, 4
    x = torch.from_numpy((rng.standard_normal((B, T, A)) * 3.0).astype(np.float32))
    logp_h = torch.log_softmax(x, dim=-1).numpy()
    keywords = [[int(v) for v in rng.integers(1, A, size=L)] for _ in range(K)]
    min_score = [-4.0 * L] * K
    logp = torch.from_numpy(logp_h).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')   # noqa: E731
    sizes, flat = i32([T] * B), i32([v for kw in keywords for v in kw])
    offs, lens = i32([L * k for k in range(K)]), i32([L] * K)
    thr = torch.tensor(min_score, dtype=torch.float64, device='cuda')
    run = lambda: ops.keyword_search(logp, sizes, flat, offs, lens, thr, max_hits=max_hits)      # noqa: E731
    out = [o.cpu().numpy() for o in run()]
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    pairs = [(b, (3 * b) % K) for b in range(B)]
    t0 = time.perf_counter()
    ref = kws_ref.search_batch(logp_h, [T] * B, keywords, min_score, max_hits=max_hits, pairs=pairs)
    host_ms = (time.perf_counter() - t0) * 1e3 * (B * K) / len(pairs)
    sel = tuple(np.asarray(pairs).T)
    same = all(np.array_equal(o[sel], r[sel]) for o, r in zip(out, ref))
    dev_ms = float(np.median(ts))
    print(json.dumps({'B': B, 'T': T, 'A': A, 'K': K, 'L': L, 'max_hits': max_hits, 'device_ms': round(dev_ms, 3),
                      'device_ms_min': round(min(ts), 3), 'per_frame_us': round(dev_ms * 1e3 / T, 3),
                      'hits_found': int(np.minimum(out[2], max_hits).sum()), 'host_ref_pairs': len(pairs),
                      'host_ref_ms_all_pairs': round(host_ms, 1), 'speedup_vs_host_ref': round(host_ms / dev_ms, 1),
                      'same_as_host_ref_on_subset': bool(same)}))


if __name__ == '__main__':
    main()
