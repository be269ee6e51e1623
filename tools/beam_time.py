#!/usr/bin/env python
"""Time the device CTC beam search (ds2_ctc_beam_search_batch) against the host search, one JSON line.

    python tools/beam_time.py [--reps 5] [--host-reps 1] [--out DIR]

Input: B = 32 utterances x T = 746 frames x A = 29 of seeded, peaked softmax output spelling generated text.  Device
times (device events, median of --reps after one warm-up) at W in {16, 64, 128}: without an LM, with a char 6-gram and
with a word 3-gram, both built by tools/make_lm.py from generated text.  The host BeamCTCDecoder (the probabilities
copied to the host, one ds2_ctc_beam_search call per utterance) is timed on the same no-LM input.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
LABELS = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]
WORDS = ('THE OF AND A TO IN IS YOU THAT IT HE WAS FOR ON ARE AS WITH HIS THEY I AT BE THIS HAVE FROM OR ONE HAD BY '
         'WORD BUT NOT WHAT ALL WERE WE WHEN YOUR CAN SAID THERE USE AN EACH WHICH SHE DO HOW THEIR IF WILL UP OTHER '
         'ABOUT OUT MANY THEN THEM THESE SO SOME HER WOULD MAKE LIKE HIM INTO TIME HAS LOOK TWO MORE WRITE GO SEE').split()


B, T = 32, 746
LM_SPECS = (('char6', 6, 'char'), ('word3', 3, 'word'))


def seeded_input(out=None, lm_names=('char6', 'word3')):
    """The input of this tool and of nbest_time.py, bias_time.py and tune_time.py; needs no GPU.  Returns probs (B,T,A)
    float32 numpy, seeded, peaked softmax output in which utterance b spells spoken[b] (letter, then blank); spoken; sents,
    the 2000 generated sentences they are cut from; and {name: NGramLM} for the ``lm_names`` among LM_SPECS, built by
    tools/make_lm.py from sents under ``out`` (default: a temporary directory)."""
    from codes.lm import NGramLM
    rng = np.random.default_rng(0)
    out = out or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    text = os.path.join(out, 'text.txt')
    sents = [' '.join(rng.choice(WORDS, size=rng.integers(4, 20))) for _ in range(2000)]
    with open(text, 'w') as f:
        f.write('\n'.join(sents) + '\n')
    lms = {}
    for name, order, unit in LM_SPECS:
        if name not in lm_names:
            continue
        path = os.path.join(out, name + '.arpa')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_lm.py'), '--order', str(order), '--unit', unit,
                        '--text', text, '-o', path], check=True, capture_output=True)
        lms[name] = NGramLM.from_arpa(path, LABELS, unit=unit)
    x = rng.standard_normal((B, T, len(LABELS))) * 1.5
    spoken = []
    for b in range(B):                       # frames spelling a sentence: letter, then blank
        s = ' '.join(sents[1000 + b * 3:1000 + b * 3 + 6])[:T // 2]
        spoken.append(s)
        for i, ch in enumerate(s):
            x[b, 2 * i, LABELS.index(ch)] += 4.0
            x[b, 2 * i + 1, 0] += 3.0
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), spoken, sents, lms


def timed(run, reps):
    """One warm-up, then ``reps`` runs between device events: (median ms, max - min ms, the last run's value)."""
    import torch
    run()
    torch.cuda.synchronize()
    ts, val = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        val = run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(max(ts) - min(ts)), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--widths', default='16,64,128')
    ap.add_argument('--out', default=None, help='directory for the generated LMs (default: a temporary one)')
    args = ap.parse_args()
    import torch
    from codes.decoder import BeamCTCDecoder
    from ds2hip import ops
    assert torch.cuda.is_available(), 'beam_time.py measures on the GPU'
    probs, _, _, lms = seeded_input(args.out)
    probs = torch.from_numpy(probs).cuda()
    A = len(LABELS)
    sizes = torch.full((B,), T, dtype=torch.int32, device='cuda')
    res = {'B': B, 'T': T, 'A': A, 'device_ms': {}, 'host_ms': {}, 'per_frame_us': {}}
    for w in [int(v) for v in args.widths.split(',')]:
        for name, lm in (('none', None), ('char6', lms['char6']), ('word3', lms['word3'])):
            ms = timed(lambda: ops.ctc_beam_search(probs, sizes, w, 0, False, lm, 0.5, 1.0, 1), args.reps)[0]
            key = 'W%d_%s' % (w, name)
            res['device_ms'][key] = round(ms, 3)
            res['per_frame_us'][key] = round(ms * 1e3 / T, 2)
        dec = BeamCTCDecoder(LABELS, beam_width=w)
        ts = []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode(probs, sizes.cpu())
            ts.append((time.perf_counter() - t0) * 1e3)
        res['host_ms']['W%d_none' % w] = round(float(np.median(ts)), 1)
        res['speedup_vs_host'] = res.get('speedup_vs_host', {})
        res['speedup_vs_host']['W%d' % w] = round(res['host_ms']['W%d_none' % w] / res['device_ms']['W%d_none' % w], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
