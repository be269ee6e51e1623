#!/usr/bin/env python
"""Generate the multi-task golden fixtures by running the REFERENCE's own multi-task model and sampler.

Run once where a checkout of the reference project exists
(``DS2_REFERENCE_TREE=<its root> python tests/golden/make_golden_multitask.py``).  It imports the reference's
``codes/model.py`` and ``codes/sampler.py`` by file path and the seeded-input helpers of ``make_golden.py``; only the outputs
under ``multitask/`` next to this file are committed (a directory of their own: the single-task generator's test pins the
set of ``*.npz`` files in this one):

  ref_mt_tiny.npz   hidden 32, 2 layers, en (A = 29, B = 3) + pt_BR (A = 43, B = 2), ragged, one batch-wide T_in:
                    the same-seed initial parameters (per-key sum and strided sample), per-head train logits and eval
                    probabilities, per-task and total loss (task_weights [1, 0.5]), the gradient of every parameter
                    (whole, or norm + strided sample above 20 k elements) and the BatchNorm buffers after the step.
  ref_mt_full_b16.npz  the default 5 x BiGRU-800 base, 8 en + 8 pt_BR utterances, T_in = 501, ragged: per task every
                    ``tstride``-th frame of the train logits and eval probabilities, the eval argmax (+ runner-up, + near-tie
                    mask) of EVERY frame, the CTC cost sum and output sizes (keys ``<name>_<task>``); per parameter the
                    gradient norm and a strided sample, and the BatchNorm buffers after the step -- the format of
                    tests/golden_cases.py ``check_against_golden``, one task at a time.
  ref_mt_traj.npz   4 Nesterov-SGD steps of the same model (task_weights [1, 0.5], max_norm 400, lr 1e-2, momentum 0.9):
                    step 2 has only pt_BR present (gradients zeroed in place, the absent head keeps moving on momentum),
                    step 3 has an en transcript that cannot be aligned: that task contributes loss 0 and no gradient
                    (the per-task infinite-loss rule), pt_BR trains as usual.
  ref_mt_sampler.json  WeightedBucketingRandomSampler bins (equal / unbalanced / schedule) on a toy two-dataset source.
  ref_multitask_configs.json  the reference's three multi-task scripts/*.json, verbatim (text).

The CTC loss is torch's F.ctc_loss on log_softmax with reduction 'sum' (the reference's warp-ctc, as in make_golden.py).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'multitask')
sys.path.insert(0, ROOT)

from oracle.model import seeded_state_dict  # noqa: E402
from tests.golden.make_golden import (label_lengths_for, load_reference_model_module, ragged_lengths,  # noqa: E402
                                      reference_root, seeded_inputs, seeded_labels)

MT_KW = dict(rnn_hidden_size=32, num_rnn_layers=2)
MT_SIZES = (3, 2)                       # en, pt_BR
MT_ALPHA = (29, 43)
MT_TIN = 101
MT_WEIGHTS = (1.0, 0.5)
TRAJ_OPT = dict(lr=1e-2, momentum=0.9, nesterov=True)
TRAJ_MAX_NORM = 400.0
MULTITASK_CONFIGS = ('example-multi-task.json', 'multi-task.json', 'multi-task-schedule-sampling.json')
SAMPLER_COUNTS = (7, 12)
SAMPLER_BATCH = 4
SAMPLER_EPOCHS = 5


def mt_batch(seed, lengths=None, label_lens=None):
    """Per-task (x (B_i,T_in,161), labels, label_lens, lengths): one batch-wide T_in, ragged lengths, seeded values."""
    n = sum(MT_SIZES)
    lengths = lengths or ragged_lengths(seed, n, MT_TIN)
    label_lens = label_lens or label_lengths_for(lengths)
    x = seeded_inputs(seed + 1, n, MT_TIN, lengths=lengths)
    out, b0 = [], 0
    for task, (bsz, nalpha) in enumerate(zip(MT_SIZES, MT_ALPHA)):
        ll = label_lens[b0:b0 + bsz]
        out.append((x[b0:b0 + bsz], seeded_labels(seed + 2 + task, ll, nalpha), list(ll), lengths[b0:b0 + bsz]))
        b0 += bsz
    return out


def traj_batches():
    """The four steps' batches: A, B, B without en, A with en's first transcript too long for its output frames."""
    a, b = mt_batch(301), mt_batch(311)
    c = [None, b[1]]
    x, _, ll, lens = a[0]
    ll = list(ll)
    ll[0] = 200                                          # > the 46 output frames: infeasible for CTC
    d = [(x, seeded_labels(399, ll, MT_ALPHA[0]), ll, lens), a[1]]
    return [a, b, c, d]


def build_reference(ref):
    torch.manual_seed(0)
    base = ref.DeepSpeech(include_classifier=False, **MT_KW)
    heads = [ref.SequenceWiseClassifier(base._rnn_hidden_size, a) for a in MT_ALPHA]
    return ref.MultiTaskModel(base, heads)


def task_losses(outs, batch):
    """[(loss_i = sum of costs / B_i, finite)] per present task, F.ctc_loss in warp-ctc's place."""
    res = []
    for o, item in zip(outs, batch):
        if item is None:
            res.append(None)
            continue
        x, labels, ll, lens = item
        pct = torch.tensor([n / float(MT_TIN) for n in lens], dtype=torch.float32)
        out_sizes = (pct * o.shape[1]).int()
        loss = F.ctc_loss(o.transpose(0, 1).log_softmax(-1), torch.from_numpy(labels).long(), out_sizes.long(),
                          torch.tensor(ll, dtype=torch.long), blank=0, reduction='sum') / x.shape[0]
        res.append(loss)
    return res


def sample(a, n=1024):
    flat = np.asarray(a).reshape(-1)
    stride = max(1, flat.shape[0] // n)
    return flat[::stride][:n].copy()


def run_tiny(ref):
    model = build_reference(ref)
    out = {}
    for k, v in model.state_dict().items():                 # same-seed initialisation (get_model under manual_seed(0))
        if v.is_floating_point():
            out['init_sum_' + k] = np.float64(v.double().sum().item())
            out['init_sample_' + k] = sample(v.numpy(), 256)
    model.load_state_dict(seeded_state_dict(model, seed=1234))
    batch = mt_batch(201)
    xs = [torch.from_numpy(b[0]) for b in batch]
    model.train()
    outs = model(xs)
    losses = task_losses(outs, batch)
    total = sum(w * l for w, l in zip(MT_WEIGHTS, losses))
    model.zero_grad()
    total.backward()
    for i, (o, l) in enumerate(zip(outs, losses)):
        out['logits_%d' % i] = o.detach().numpy()
        out['loss_%d' % i] = np.float64(l.item())
        out['pct_%d' % i] = np.array([n / float(MT_TIN) for n in batch[i][3]], np.float32)
    out['loss_total'] = np.float64(total.item())
    for k, p in model.named_parameters():
        g = p.grad.detach().numpy()
        out['gnorm_' + k] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        if g.size <= 20000:
            out['grad_' + k] = g
        else:
            out['gsample_' + k] = sample(g)
    for k, v in model.state_dict().items():
        if 'running' in k or 'num_batches' in k:
            out['buf_' + k] = v.numpy().copy()
    model.eval()
    with torch.no_grad():
        probs = model(xs)
        solo = model([None, xs[1]])                        # an absent task: None out, the other head as before
    for i, p in enumerate(probs):
        out['probs_%d' % i] = p.numpy()
    out['probs_solo_1'] = solo[1].numpy()
    np.savez_compressed(os.path.join(OUT, 'ref_mt_tiny.npz'), **out)
    print('ref_mt_tiny.npz', 'losses', [l.item() for l in losses], 'total', total.item())


FULL_SIZES = (8, 8)
FULL_TIN = 501
FULL_TSTRIDE = 4


def full_b16_batch():
    """Per-task (x, labels, label_lens, lengths) of the full-size case: one batch-wide T_in, ragged."""
    n = sum(FULL_SIZES)
    lengths = ragged_lengths(501, n, FULL_TIN)
    label_lens = label_lengths_for(lengths)
    x = seeded_inputs(502, n, FULL_TIN, lengths=lengths)
    out, b0 = [], 0
    for task, (bsz, nalpha) in enumerate(zip(FULL_SIZES, MT_ALPHA)):
        ll = label_lens[b0:b0 + bsz]
        out.append((x[b0:b0 + bsz], seeded_labels(503 + task, ll, nalpha), list(ll), lengths[b0:b0 + bsz]))
        b0 += bsz
    return out


def run_full_b16(ref):
    torch.manual_seed(0)
    base = ref.DeepSpeech(include_classifier=False)
    model = ref.MultiTaskModel(base, [ref.SequenceWiseClassifier(base._rnn_hidden_size, a) for a in MT_ALPHA])
    model.load_state_dict(seeded_state_dict(model, seed=1234))
    batch = full_b16_batch()
    xs = [torch.from_numpy(b[0]) for b in batch]
    model.train()
    outs = model(xs)
    out = {'tstride': np.int32(FULL_TSTRIDE)}
    total = 0
    for i, (o, item) in enumerate(zip(outs, batch)):
        x, labels, ll, lens = item
        pct = torch.tensor([n / float(FULL_TIN) for n in lens], dtype=torch.float32)
        out_sizes = (pct * o.shape[1]).int()
        cost = F.ctc_loss(o.transpose(0, 1).log_softmax(-1), torch.from_numpy(labels).long(), out_sizes.long(),
                          torch.tensor(ll, dtype=torch.long), blank=0, reduction='sum')
        total = total + MT_WEIGHTS[i] * cost / x.shape[0]
        out['logits_%d' % i] = o.detach().numpy()[:, ::FULL_TSTRIDE].copy()
        out['loss_sum_%d' % i] = np.float32(cost.item())
        out['out_sizes_%d' % i] = out_sizes.numpy().astype(np.int32)
        out['pct_%d' % i] = pct.numpy()
    model.zero_grad()
    total.backward()
    out['loss_total'] = np.float64(total.item())
    for k, p in model.named_parameters():
        g = p.grad.detach().numpy()
        out['gnorm_' + k] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        out['gsample_' + k] = sample(g)
    for k, v in model.state_dict().items():
        if 'running' in k:
            out['buf_' + k] = v.numpy().copy()
    model.eval()
    with torch.no_grad():
        probs = model(xs)
    for i, p in enumerate(probs):
        p = p.numpy()
        out['probs_%d' % i] = p[:, ::FULL_TSTRIDE].copy()
        order = np.argsort(-p, axis=-1, kind='stable')
        top = np.take_along_axis(p, order[..., :2], -1)
        out['argmax_%d' % i] = order[..., 0].astype(np.uint8)
        out['argmax2_%d' % i] = order[..., 1].astype(np.uint8)
        out['near_tie_%d' % i] = (top[..., 0] - top[..., 1]) < 1e-4
    np.savez_compressed(os.path.join(OUT, 'ref_mt_full_b16.npz'), **out)
    print('ref_mt_full_b16.npz total', total.item(), 'size %.1f KB' % (os.path.getsize(os.path.join(OUT, 'ref_mt_full_b16.npz')) / 1024.0))


def run_traj(ref):
    model = build_reference(ref)
    model.load_state_dict(seeded_state_dict(model, seed=1234))
    opt = torch.optim.SGD(model.parameters(), **TRAJ_OPT)
    out = {'losses': [], 'gnorms': [], 'task_losses': []}
    for step, batch in enumerate(traj_batches()):
        model.train()
        xs = [None if b is None else torch.from_numpy(b[0]) for b in batch]
        outs = model(xs)
        losses = task_losses(outs, batch)
        total, value, per = None, 0.0, []
        for w, l in zip(MT_WEIGHTS, losses):
            if l is None:
                per.append(np.nan)
                continue
            if not np.isfinite(l.item()):                   # the per-task infinite-loss rule: 0, and no gradient
                per.append(0.0)
                continue
            per.append(l.item())
            value += w * l.item()
            total = w * l if total is None else total + w * l
        opt.zero_grad(set_to_none=False)                    # zero-then-step: an absent head moves on momentum
        total.backward()
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), TRAJ_MAX_NORM)
        opt.step()
        out['losses'].append(value)
        out['gnorms'].append(float(gn))
        out['task_losses'].append(per)
        print('  step', step, 'loss', value, per, 'gnorm', float(gn))
    for k in ('losses', 'gnorms', 'task_losses'):
        out[k] = np.asarray(out[k], np.float64)
    for k, p in model.named_parameters():
        flat = p.detach().numpy().reshape(-1)
        out['wsample_' + k] = sample(flat)
        out['wnorm_' + k] = np.float64(np.sqrt((flat.astype(np.float64) ** 2).sum()))
        out['msample_' + k] = sample(opt.state[p]['momentum_buffer'].numpy())
    for k, v in model.state_dict().items():
        if 'running' in k or 'num_batches' in k:
            out['buf_' + k] = v.numpy().copy()
    np.savez_compressed(os.path.join(OUT, 'ref_mt_traj.npz'), **out)
    print('ref_mt_traj.npz', out['losses'])


class ToySource(object):
    """Two manifests' durations end to end, as ConcatAudioDataset exposes them."""

    def __init__(self, counts=SAMPLER_COUNTS, seed=5):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.durations = []
        self.cumulative_sizes = []
        for c in counts:
            self.durations += sorted(float(v) for v in np.round(rng.uniform(1.0, 15.0, size=c), 3))
            self.cumulative_sizes.append(len(self.durations))

    def __len__(self):
        return len(self.durations)


def run_sampler(root):
    spec = importlib.util.spec_from_file_location('reference_codes_sampler', os.path.join(root, 'codes', 'sampler.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    src = ToySource()
    out = {'counts': list(SAMPLER_COUNTS), 'batch_size': SAMPLER_BATCH, 'num_epochs': SAMPLER_EPOCHS,
           'durations': src.durations, 'bins': {}}
    for sampling in ('equal', 'unbalanced', 'schedule'):
        s = mod.WeightedBucketingRandomSampler(src, batch_size=SAMPLER_BATCH, sampling=sampling, num_epochs=SAMPLER_EPOCHS)
        per = {}
        for epoch in (0, 1, 3):
            if epoch:
                s.shuffle(epoch)
            per[str(epoch)] = [[int(i) for i in b] for b in s.bins]
        out['bins'][sampling] = per
    with open(os.path.join(OUT, 'ref_mt_sampler.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


def write_configs(root):
    cfg = {}
    for name in MULTITASK_CONFIGS:
        with open(os.path.join(root, 'scripts', name)) as f:
            cfg[name] = f.read()
    with open(os.path.join(OUT, 'ref_multitask_configs.json'), 'w') as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write('\n')


def main():
    root = reference_root()
    ref = load_reference_model_module()
    run_tiny(ref)
    run_traj(ref)
    run_full_b16(ref)
    run_sampler(root)
    write_configs(root)


if __name__ == '__main__':
    main()
