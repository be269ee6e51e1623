#!/usr/bin/env python
"""Time banded CTC alignment with gaps (ds2_ctc_align_banded_gap) beside the plain entry (ds2_ctc_align_banded) on the same
input in the same process, one JSON line.

    python tools/align_gap_time.py [--reps 3] [--leg-timeout 600] [--bands 1024,4096,8192]

Input: tools/align_long_time.py's -- T = 180 000 frames x A = 29 of seeded, peaked softmax output aligned to its L = 50 000
labels on the diagonal band; label 1 stands for the space (one label in 28, so the blanks beside one label in 14 are
eligible).  One child process per band width under its own time limit (a leg that fails ends the run).  In each, after one
warm-up launch of every form, --reps rounds of plain, gap at g = inf, gap at g = 4 in turn -- alternating, so that a drift of
the machine falls on all three -- each launch between device events, workspace allocation included as in
tools/align_long_time.py; the medians are reported, with min and max as the spread.  Reported beside the times: whether the
states at g = inf equal the plain entry's (they must), and how many frames g = 4 absorbs.  There is no pass / fail time."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from align_long_time import A, L, T, inputs  # noqa: E402

SPACE, G = 1, 4.0


def leg(w, reps):
    import torch
    from codes.align import diagonal_band
    from ds2hip import ops
    assert torch.cuda.is_available(), 'align_gap_time.py measures on the GPU'
    probs_h, labels = inputs()
    probs = torch.from_numpy(probs_h).cuda()[None]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')   # noqa: E731
    lo_d = diagonal_band(T, 2 * L + 1, w).to('cuda', torch.int32)[None]
    args = (probs, i32([T]), i32(labels.tolist()), i32([0]), i32([L]), L, lo_d, w)
    forms = {'plain': lambda: ops.ctc_align_banded(*args),
             'gap_inf': lambda: ops.ctc_align_banded_gap(*args, SPACE, float('inf')),
             'gap': lambda: ops.ctc_align_banded_gap(*args, SPACE, G)}
    out = {k: f() for k, f in forms.items()}                        # the warm-up launches; their results are the ones compared
    torch.cuda.synchronize()
    ts = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    res = {'W': w}
    for k, v in ts.items():
        res[k + '_ms'] = round(float(np.median(v)), 2)
        res[k + '_ms_min_max'] = [round(min(v), 2), round(max(v), 2)]
    res['gap_inf_over_plain'] = round(res['gap_inf_ms'] / res['plain_ms'], 4)
    res['gap_over_plain'] = round(res['gap_ms'] / res['plain_ms'], 4)
    res['equal_states_at_inf'] = bool(torch.equal(out['plain'][0], out['gap_inf'][0]) and
                                      torch.equal(out['plain'][1], out['gap_inf'][1]) and
                                      torch.equal(out['plain'][2], out['gap_inf'][2]) and
                                      torch.equal(out['plain'][3], out['gap_inf'][4]) and not bool(out['gap_inf'][3].any()))
    res['plain_score'], res['gap_score'] = float(out['plain'][3][0]), float(out['gap'][4][0])
    res['gap_frames'] = int(out['gap'][3].sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--leg-timeout', type=int, default=600, help='seconds per band width')
    ap.add_argument('--bands', default='1024,4096,8192')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg is not None:
        print(json.dumps(leg(int(args.leg), args.reps)))
        return
    res = {'T': T, 'A': A, 'L': L, 'space': SPACE, 'gap_penalty': G, 'reps': args.reps, 'legs': {}}
    for w in args.bands.split(','):
        cmd = ['timeout', '-k', '10', str(args.leg_timeout), sys.executable, os.path.abspath(__file__), '--leg', w, '--reps',
               str(args.reps)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            res['legs'][w] = {'failed': out.returncode, 'stderr': out.stderr[-400:]}
            break
        res['legs'][w] = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if any('failed' in v for v in res['legs'].values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
