#!/usr/bin/env python
"""Time the device CTC beam search that returns N-best lists (ds2_ctc_beam_search_nbest) beside the 1-best entry
(ds2_ctc_beam_search_batch) on the same input, one JSON line.

    python tools/nbest_time.py [--reps 5] [--out DIR]

Input: tools/beam_time.py's -- B = 32 utterances x T = 746 frames x A = 29 of seeded, peaked softmax output spelling
generated text.  (W, N) in (16,1), (16,4), (16,16), (64,16), (64,64); without an LM and with a word 3-gram built by
tools/make_lm.py.  Device events, median of --reps after one warm-up; ``spread_ms`` is max - min of the repeats.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--points', default='16:1,16:4,16:16,64:16,64:64', help='W:N pairs')
    ap.add_argument('--out', default=None, help='directory for the generated LM (default: a temporary one)')
    args = ap.parse_args()
    import torch
    from beam_time import B, LABELS, T, seeded_input, timed
    from ds2hip import ops
    assert torch.cuda.is_available(), 'nbest_time.py measures on the GPU'
    probs, _, _, lms = seeded_input(args.out, ('word3',))
    probs = torch.from_numpy(probs).cuda()
    lms = {'none': None, 'word3': lms['word3']}
    A = len(LABELS)
    sizes = torch.full((B,), T, dtype=torch.int32, device='cuda')
    res = {'B': B, 'T': T, 'A': A, 'batch_ms': {}, 'batch_spread_ms': {}, 'nbest_ms': {}, 'nbest_spread_ms': {},
           'ratio': {}, 'mean_count': {}}
    for w, n in [tuple(int(v) for v in p.split(':')) for p in args.points.split(',')]:
        for name, lm in lms.items():
            key = 'W%d_N%d_%s' % (w, n, name)
            plain, plain_sp, _ = timed(lambda: ops.ctc_beam_search(probs, sizes, w, 0, False, lm, 0.5, 1.0, 1), args.reps)
            many, many_sp, _ = timed(lambda: ops.ctc_beam_search_nbest(probs, sizes, w, n, 0, False, lm, 0.5, 1.0, 1),
                                       args.reps)
            res['batch_ms'][key], res['batch_spread_ms'][key] = round(plain, 3), round(plain_sp, 3)
            res['nbest_ms'][key], res['nbest_spread_ms'][key] = round(many, 3), round(many_sp, 3)
            res['ratio'][key] = round(many / plain, 3)
            res['mean_count'][key] = round(float(ops.ctc_beam_search_nbest(probs, sizes, w, n, 0, False, lm, 0.5, 1.0,
                                                                           1)[6].float().mean()), 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
