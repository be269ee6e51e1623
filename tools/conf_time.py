#!/usr/bin/env python
"""Time the word-confidence call (ds2_ctc_unit_posterior) beside the search that feeds it, one JSON line.

    python tools/conf_time.py [--reps 5]

Input: B = 32 segments x T = 746 frames x A = 29 of seeded softmax output that spells about 100 labels per row (a peak
every 7 frames, a space every sixth peak or so), decoded by the device beam search at width 16.  Device times: device
events around one call (its launches and the allocation of workspace and outputs included), median of --reps after one
warm-up, for
  * ``ops.ctc_unit_posterior`` on the 32 one-best rows, words;
  * ``ops.ctc_unit_posterior`` on the 512 rows of the 16-best list (utt = row // 16), words;
  * the ``ds2_ctc_beam_search_batch`` call that produced the one-best rows, and the N-best call, for scale.
Host time: tests/conf_ref.py on the first 4 one-best rows, per row; the device values are compared with it there."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)


def spelled(rng, B, T, A, space_id, period=7):
    x = rng.standard_normal((B, T, A)).astype(np.float32)
    x[:, :, 0] += 4.0
    for b in range(B):
        for t in range(int(rng.integers(0, period)), T, period):
            c = space_id if rng.random() < 1.0 / 6.0 else int(rng.integers(2, A))
            x[b, t, c] += 7.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    from ds2hip import ops
    from tests import conf_ref
    assert torch.cuda.is_available(), 'conf_time.py measures on the GPU'
    rng = np.random.default_rng(0)
    B, T, A, W, N, space_id = 32, 746, 29, 16, 16, 1
    probs = torch.softmax(torch.from_numpy(spelled(rng, B, T, A, space_id)), dim=-1).contiguous()
    probs_d = probs.cuda()
    sizes = torch.full((B,), T, dtype=torch.int32, device='cuda')

    spread = {}                                            # [min, max] of every timed call, in the order of the *_ms keys

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        spread[len(spread)] = [round(min(ts), 3), round(max(ts), 3)]
        return round(float(np.median(ts)), 3)

    one = ops.ctc_beam_search(probs_d, sizes, W, space_id=space_id)
    many = ops.ctc_beam_search_nbest(probs_d, sizes, W, N, space_id=space_id)
    rows = [x.view(B * N, -1) if x.dim() == 3 else x.view(B * N) for x in many[:3]]
    utt = (torch.arange(B * N, dtype=torch.int32, device='cuda') // N).int()
    res = {'B': B, 'T': T, 'A': A, 'beam_width': W, 'nbest': N,
           'labels_per_row': round(float(one[2].float().mean()), 1)}
    out1 = ops.ctc_unit_posterior(probs_d, sizes, one[0], one[1], one[2], space_id=space_id)
    outn = ops.ctc_unit_posterior(probs_d, sizes, rows[0], rows[1], rows[2], utt, space_id=space_id)
    res['words_one_best'] = int(out1[3].clamp(min=0).sum())
    res['words_nbest_rows'] = int(outn[3].clamp(min=0).sum())
    res['unit_posterior_32_rows_ms'] = timed(lambda: ops.ctc_unit_posterior(probs_d, sizes, one[0], one[1], one[2],
                                                                            space_id=space_id))
    res['unit_posterior_512_rows_ms'] = timed(lambda: ops.ctc_unit_posterior(probs_d, sizes, rows[0], rows[1], rows[2], utt,
                                                                             space_id=space_id))
    res['beam_search_batch_ms'] = timed(lambda: ops.ctc_beam_search(probs_d, sizes, W, space_id=space_id))
    res['beam_search_nbest_ms'] = timed(lambda: ops.ctc_beam_search_nbest(probs_d, sizes, W, N, space_id=space_id))
    res['min_max_ms'] = [spread[i] for i in range(len(spread))]
    k = 4
    lab, off, ln = (x[:k].cpu().numpy() for x in one[:3])
    t0 = time.perf_counter()
    ref = conf_ref.unit_posterior(probs.numpy()[:k], [T] * k, lab, off, ln, None, space_id, 0)
    res['host_ref_ms_per_row'] = round((time.perf_counter() - t0) * 1e3 / k, 1)
    got = out1[2][:k].cpu().numpy()
    fin = np.isfinite(ref[2])
    res['same_units_as_host_ref'] = bool(np.array_equal(ref[3], out1[3][:k].cpu().numpy()))
    res['max_abs_dlogp_vs_host_ref'] = float(np.abs(got[fin] - ref[2][fin]).max()) if fin.any() else 0.0
    print(json.dumps(res))


if __name__ == '__main__':
    main()
