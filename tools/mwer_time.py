#!/usr/bin/env python
"""Time the MWER loss (ds2_ctc_mwer_grad, codes.ctc.mwer_costs_and_grad) beside what it replaces, one JSON line.

    python tools/mwer_time.py [--reps 5]

Input: one training-size minibatch -- B = 10 utterances x T = 746 frames x A = 29 of seeded activations that spell generated
text of about 100 labels per utterance (blank-dominated elsewhere, margins of an unsure model), N = 4 hypotheses from a beam of W = 8.
  kernel_ms        ds2_ctc_mwer_grad alone, on the hypotheses the device search returned for this input
  composition_ms   the same result from existing ops: acts replicated to (T, B (N+1), A), ONE ds2_ctc_loss_grad call over
                   all rows, the posteriors and the weighted sum of the rows' gradients in torch
  mwer_ms          the whole codes.ctc.mwer_costs_and_grad (softmax, transpose, search, edit_stats, its one readback, kernel)
  ctc_ms           codes.ctc.ctc_costs_and_grad on the same input
  search_ms        softmax + transpose + ds2_ctc_beam_search_nbest alone
Device events, median of --reps after one warm-up; ``*_spread_ms`` is max - min of the repeats.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    import beam_time
    from beam_time import LABELS, WORDS
    from codes.ctc import ctc_costs_and_grad, mwer_costs_and_grad
    from ds2hip import ops
    assert torch.cuda.is_available(), 'mwer_time.py measures on the GPU'
    rng = np.random.default_rng(0)
    B, T, A, N, W = 10, 746, len(LABELS), 4, 8
    space = LABELS.index(' ')
    x = rng.standard_normal((T, B, A))
    x[:, :, 0] += 5.0                        # a trained model's output: blank wherever nothing is said
    refs = []
    for b in range(B):                       # frames spelling a sentence: one letter every third frame
        s = ' '.join(rng.choice(WORDS, size=30))[:int(rng.integers(90, 111))]
        refs.append([LABELS.index(ch) for ch in s])
        for i, ch in enumerate(s):
            x[3 * i, b, LABELS.index(ch)] += 7.0
    acts = torch.from_numpy(x.astype(np.float32)).cuda()
    targets = torch.tensor([v for r in refs for v in r], dtype=torch.int32)
    sizes = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    act_lens = torch.full((B,), T, dtype=torch.int32)

    def timed(run):
        return tuple(round(v, 3) for v in beam_time.timed(run, args.reps)[:2])

    res = {'B': B, 'T': T, 'A': A, 'N': N, 'W': W, 'mean_ref_len': round(float(sizes.float().mean()), 1)}
    _, _, info = mwer_costs_and_grad(acts, targets, act_lens, sizes, space, nbest=N, beam_width=W)
    hyp, hyp_len, count, risk = info['hyp'], info['hyp_len'], info['count'], info['risk']
    res['mean_count'] = round(float(count.float().mean()), 2)
    res['mean_hyp_len'] = round(float(hyp_len.float().mean()), 1)
    res['mean_exp_risk'] = round(float(info['exp_risk'].mean()), 3)
    max_len = min(max(int(hyp_len.max()), int(sizes.max())), 511)
    res['max_label_len'] = max_len
    res['workspace_mb'] = round(ops.ctc_mwer_ws_bytes(T, B, A, N, max_len) / 2.0 ** 20, 1)
    dev = acts.device
    ref_d, lens_d, alen_d = targets.to(dev), sizes.to(dev), act_lens.to(dev)
    offs_d = (torch.cumsum(lens_d, 0) - lens_d).int()
    ws = torch.empty(ops.ctc_mwer_ws_bytes(T, B, A, N, max_len), dtype=torch.uint8, device=dev)

    def kernel():
        return ops.ctc_mwer_grad(acts, alen_d, hyp, hyp_len, count, risk, ref_d, offs_d, lens_d, max_len, 0.01, 0.1, True, ws=ws)

    # the composition: every row of every utterance as an utterance of its own
    rows_lab = torch.cat([hyp[:, :, :max_len], torch.zeros((B, 1, max_len), dtype=torch.int32, device=dev)], 1)
    for b in range(B):
        rows_lab[b, N, :len(refs[b])] = torch.tensor(refs[b], dtype=torch.int32, device=dev)
    rows_lab = rows_lab.reshape(B * (N + 1), max_len).contiguous()
    rows_len = torch.cat([hyp_len, lens_d.view(B, 1)], 1).reshape(-1).contiguous()
    rows_off = (torch.arange(B * (N + 1), device=dev, dtype=torch.int32) * max_len).contiguous()
    rows_alen = alen_d.repeat_interleave(N + 1).contiguous()

    def composition():
        rep = acts.repeat_interleave(N + 1, dim=1).contiguous()
        costs, grads = ops.ctc_loss_grad(rep, rows_lab.view(-1), rows_off, rows_len, rows_alen, max_len)
        c = costs.double().view(B, N + 1)
        post = torch.softmax(-c[:, :N], 1)
        exp_risk = (post * risk.double()).sum(1, keepdim=True)
        w = torch.cat([-post * (risk.double() - exp_risk), torch.full((B, 1), 0.01, dtype=torch.float64, device=dev)], 1)
        return 0.1 * (grads.view(T, B, N + 1, A) * w.float().view(1, B, N + 1, 1)).sum(2)

    diff = float((kernel()[5] - composition()).abs().max())
    res['kernel_minus_composition'] = diff
    res['kernel_ms'], res['kernel_spread_ms'] = timed(kernel)
    res['composition_ms'], res['composition_spread_ms'] = timed(composition)
    res['mwer_ms'], res['mwer_spread_ms'] = timed(
        lambda: mwer_costs_and_grad(acts, targets, act_lens, sizes, space, nbest=N, beam_width=W, grad_scale=0.1,
                                    zero_batch_if_inf=True))
    res['ctc_ms'], res['ctc_spread_ms'] = timed(
        lambda: ctc_costs_and_grad(acts, targets, act_lens, sizes, grad_scale=0.1, zero_batch_if_inf=True))
    res['search_ms'], res['search_spread_ms'] = timed(
        lambda: ops.ctc_beam_search_nbest(ops.softmax_rows(acts, T * B, A).transpose(0, 1).contiguous(), alen_d, W, N))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
