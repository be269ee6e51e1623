#!/usr/bin/env python
"""Time the device CTC beam search with phrase boosting (ds2_ctc_beam_search_bias) beside the unbiased entry
(ds2_ctc_beam_search_batch) on the same input, one JSON line.

    python tools/bias_time.py [--reps 5] [--out DIR]

Input: tools/beam_time.py's -- B = 32 utterances x T = 746 frames x A = 29 of seeded, peaked softmax output spelling
generated text.  W in {16, 64}; without an LM and with a word 3-gram built by tools/make_lm.py; 100 boosted phrases of 8
labels cut from the generated text (so that they do occur).  Device events, median of --reps after one warm-up.
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
    ap.add_argument('--widths', default='16,64')
    ap.add_argument('--weight', type=float, default=2.0)
    ap.add_argument('--out', default=None, help='directory for the generated LM (default: a temporary one)')
    args = ap.parse_args()
    import torch
    from beam_time import B, LABELS, T, seeded_input, timed
    from codes.bias import PhraseBooster
    from ds2hip import ops
    assert torch.cuda.is_available(), 'bias_time.py measures on the GPU'
    probs, spoken, sents, lms = seeded_input(args.out, ('word3',))
    probs = torch.from_numpy(probs).cuda()
    lms = {'none': None, 'word3': lms['word3']}
    A = len(LABELS)
    sizes = torch.full((B,), T, dtype=torch.int32, device='cuda')
    phrases, k = [], 0
    while len(phrases) < 100:                # 8-label cuts of what is spoken, then of the rest of the text
        s = (spoken + sents)[k % (B + len(sents))]
        cut = s[(7 * k) % max(1, len(s) - 8):][:8]
        if len(cut) == 8 and cut not in phrases:
            phrases.append(cut)
        k += 1
    booster = PhraseBooster(LABELS, phrases, weight=args.weight)
    trans, final = booster.tables(probs.device)
    res = {'B': B, 'T': T, 'A': A, 'phrases': len(phrases), 'phrase_labels': 8, 'states': booster.graph.n_states,
           'weight': args.weight, 'batch_ms': {}, 'bias_ms': {}, 'ratio': {}, 'boosted_labels': {}}
    for w in [int(v) for v in args.widths.split(',')]:
        for name, lm in lms.items():
            key = 'W%d_%s' % (w, name)
            plain = timed(lambda: ops.ctc_beam_search(probs, sizes, w, 0, False, lm, 0.5, 1.0, 1), args.reps)[0]
            bias = timed(lambda: ops.ctc_beam_search_bias(probs, sizes, w, trans, final, args.weight, 0, False, lm, 0.5,
                                                          1.0, 1), args.reps)[0]
            res['batch_ms'][key], res['bias_ms'][key] = round(plain, 3), round(bias, 3)
            res['ratio'][key] = round(bias / plain, 3)
            res['boosted_labels'][key] = int(ops.ctc_beam_search_bias(probs, sizes, w, trans, final, args.weight, 0, False,
                                                                      lm, 0.5, 1.0, 1)[5].sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
