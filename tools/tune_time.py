#!/usr/bin/env python
"""Time a 64-point LM weight sweep: the per-point path against codes.tune.LMTuner, one JSON line.

    python tools/tune_time.py [--reps 5] [--widths 16,64] [--rows 32,256,1024,2048] [--out DIR]

Input: tools/beam_time.py's -- B = 32 utterances x T = 746 frames x A = 29 of seeded, peaked softmax output spelling
generated text, a word 3-gram and a char 6-gram built by tools/make_lm.py -- with the spelled sentences as targets, and an
8 x 8 grid of (alpha, beta).  Device events around each whole sweep, median of --reps after one warm-up:
  (a) per_point_ms   what there was before LMTuner: 64 DeviceBeamCTCDecoder.decode calls, each followed by the host loop of
                     test.py (labels to strings, Decoder.wer / Decoder.cer per utterance)
  (b) tuner_ms       LMTuner.add_batch + result() at each --rows value of rows_per_launch; beam_ms / edit_ms are the sums of
                     the sweep's ctc_beam_search_rows and edit_stats launches, timed by their own events in a separate run
Needs no corpus.  The numbers in DESIGN.md "LM weight tuning" are this tool's.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)
from tools.beam_time import B, LABELS, T, seeded_input, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--widths', default='16,64')
    ap.add_argument('--rows', default='32,256,1024,2048')
    ap.add_argument('--lms', default='word3,char6')
    ap.add_argument('--out', default=None, help='directory for the generated LMs (default: a temporary one)')
    args = ap.parse_args()
    import torch
    from codes import tune
    from codes.decoder import DeviceBeamCTCDecoder
    from ds2hip import ops
    assert torch.cuda.is_available(), 'tune_time.py measures on the GPU'
    probs, refs, _, lms = seeded_input(args.out, args.lms.split(','))
    probs = torch.from_numpy(probs).cuda()
    A = len(LABELS)
    sizes = torch.full((B,), T, dtype=torch.int32, device='cuda')
    targets = torch.tensor([LABELS.index(c) for r in refs for c in r], dtype=torch.int32, device='cuda')
    target_sizes = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    alphas = [round(0.25 * k, 2) for k in range(8)]
    betas = [round(0.5 * k, 2) for k in range(8)]

    res = {'B': B, 'T': T, 'A': A, 'grid_points': len(alphas) * len(betas), 'reps': args.reps, 'per_point_ms': {},
           'tuner_ms': {}, 'beam_ms': {}, 'edit_ms': {}, 'launches': {}, 'agree': True}
    for w in [int(v) for v in args.widths.split(',')]:
        for name, lm in lms.items():
            key = 'W%d_%s' % (w, name)

            def per_point():
                table = []
                for a in alphas:
                    for b in betas:
                        dec = DeviceBeamCTCDecoder(LABELS, beam_width=w, lm=lm, alpha=a, beta=b)
                        decoded, _ = dec.decode(probs, sizes)
                        table.append((sum(dec.wer(h[0], r) for h, r in zip(decoded, refs)),
                                      sum(dec.cer(h[0], r) for h, r in zip(decoded, refs))))
                return table

            ms, _, want = timed(per_point, args.reps)
            res['per_point_ms'][key] = round(ms, 2)
            for rows in [int(v) for v in args.rows.split(',')]:
                def sweep():
                    t = tune.LMTuner(LABELS, lm, w, alphas, betas, rows_per_launch=rows)
                    t.add_batch(probs, sizes, targets, target_sizes)
                    return t.result(), t.launches

                rkey = '%s_rows%d' % (key, rows)
                ms, _, (table, launches) = timed(sweep, args.reps)
                res['tuner_ms'][rkey] = round(ms, 2)
                res['launches'][rkey] = launches
                res['agree'] = res['agree'] and [(g['word_dist'], g['char_dist']) for g in table['grid']] == want
                # the two launches on their own: the same sweep with an event pair around every call
                pairs = {'beam': [], 'edit': []}

                def wrap(fn, kind):
                    def inner(*a, **k):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        val = fn(*a, **k)
                        e1.record()
                        pairs[kind].append((e0, e1))
                        return val
                    return inner

                saved = ops.ctc_beam_search_rows, ops.edit_stats
                ops.ctc_beam_search_rows, ops.edit_stats = wrap(saved[0], 'beam'), wrap(saved[1], 'edit')
                try:
                    sums = {'beam': [], 'edit': []}
                    for _ in range(args.reps):
                        pairs['beam'], pairs['edit'] = [], []
                        sweep()
                        torch.cuda.synchronize()
                        for kind in sums:
                            sums[kind].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs[kind]))
                finally:
                    ops.ctc_beam_search_rows, ops.edit_stats = saved
                res['beam_ms'][rkey] = round(float(np.median(sums['beam'])), 2)
                res['edit_ms'][rkey] = round(float(np.median(sums['edit'])), 3)
            print('measured %s' % key, file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
