"""Multi-task path on the GPU: the segmented sequence-BatchNorm kernels against fp64 torch, the MultiTaskModel against the
reference's (ref_mt_tiny.npz), and the fused and autograd trainers against the reference's optimisation trajectory
(ref_mt_traj.npz: an absent task, an infeasible task)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.model import seeded_state_dict  # noqa: E402
from tests.golden.make_golden_multitask import MT_KW, MT_TIN, MT_WEIGHTS, TRAJ_MAX_NORM, TRAJ_OPT, mt_batch, traj_batches  # noqa: E402,E501


# ------------------------------------------------------------------------------------------------ segmented BatchNorm
def _bn_truth(x, bounds, gammas, betas, rms, rvs, dxf, training):
    """fp64 per-task BatchNorm over the strided rows of x (T,B,H): packed y, interleaved dx, dgamma, dbeta, new buffers."""
    t, b, h = x.shape
    ys, dx = [], torch.empty_like(x)
    dg, db, nrm, nrv = [], [], [], []
    for g in range(len(bounds) - 1):
        xs = x[:, bounds[g]:bounds[g + 1]].reshape(-1, h)
        n = xs.shape[0]
        if training:
            mu, var = xs.mean(0), xs.var(0, unbiased=False)
            nrm.append(0.9 * rms[g] + 0.1 * mu)
            nrv.append(0.9 * rvs[g] + 0.1 * (var * n / (n - 1) if n > 1 else var))
        else:
            mu, var = rms[g], rvs[g]
        inv = 1.0 / torch.sqrt(var + 1e-5)
        xh = (xs - mu) * inv
        ys.append(xh * gammas[g] + betas[g])
        d = dxf[t * bounds[g]:t * bounds[g + 1]]
        dg.append((d * xh).sum(0))
        db.append(d.sum(0))
        dxs = gammas[g] * inv * (d - d.mean(0) - xh * (d * xh).mean(0))
        dx[:, bounds[g]:bounds[g + 1]] = dxs.view(t, bounds[g + 1] - bounds[g], h)
    return torch.cat(ys), dx.reshape(-1, h), dg, db, nrm, nrv


@pytest.mark.parametrize('t,bounds,h', [(746, [0, 16], 800), (746, [0, 8, 16], 800), (1, [0, 3, 5], 32),
                                        (37, [0, 1, 4, 5, 9, 10], 32), (1, [0, 2, 3, 7, 8, 10], 800),
                                        (19, [0, 3, 5], 36), (11, [0, 2, 5], 30)])
def test_segmented_batchnorm_against_fp64(t, bounds, h):
    from ds2hip import ops
    torch.manual_seed(t * 131 + h + len(bounds))
    b, nseg = bounds[-1], len(bounds) - 1
    dev = 'cuda'
    xa = (torch.randn(t, b, h) * 2 + 0.5).to(dev)
    xb = torch.randn(t, b, h).to(dev)
    gam = [(torch.rand(h) + 0.5).to(dev) for _ in range(nseg)]
    bet = [(torch.rand(h) - 0.5).to(dev) for _ in range(nseg)]
    rms = [(torch.rand(h) - 0.5).to(dev) for _ in range(nseg)]
    rvs = [(torch.rand(h) + 0.5).to(dev) for _ in range(nseg)]
    dxf = torch.randn(t * b, h).to(dev)
    x64 = (xa.double() + xb.double()).cpu()
    d64 = [v.double().cpu() for v in gam], [v.double().cpu() for v in bet]
    for training in (True, False):
        rm = [v.clone() for v in rms]
        rv = [v.clone() for v in rvs]
        y_t, dx_t, dg_t, db_t, nrm, nrv = _bn_truth(x64, bounds, d64[0], d64[1], [v.double().cpu() for v in rms],
                                                    [v.double().cpu() for v in rvs], dxf.double().cpu(), training)
        mi = ops.bn1d_seg_stats(xa, xb, t, b, h, bounds, rm, rv, training)
        y = ops.bn1d_seg_apply(xa, xb, mi, t, b, h, bounds, gam, bet)
        for g in range(nseg):
            # (the batch variance is E[x^2] - mean^2 from fp32 partials, as in the single-task kernels: over the 2 rows of a
            # T = 1 segment that difference loses digits, so few-row segments get a wider band)
            rows = slice(t * bounds[g], t * bounds[g + 1])
            few = training and t * (bounds[g + 1] - bounds[g]) < 8
            torch.testing.assert_close(y[rows].double().cpu(), y_t[rows], atol=5e-3 if few else 2e-4, rtol=1e-4)
        if training:
            for g in range(nseg):
                torch.testing.assert_close(rm[g].double().cpu(), nrm[g], atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(rv[g].double().cpu(), nrv[g], atol=1e-5, rtol=1e-4)
            dgs = [torch.full((h,), float('nan'), device=dev) for _ in range(nseg)]
            dbs = [torch.full((h,), float('nan'), device=dev) for _ in range(nseg)]
            dx = ops.bn1d_seg_bwd(xa, xb, dxf, mi, t, b, h, bounds, gam, dgs, dbs)
            got = dx.double().cpu().view(t, b, h)
            want = dx_t.view(t, b, h)
            for g in range(nseg):
                cols = slice(bounds[g], bounds[g + 1])
                few = t * (bounds[g + 1] - bounds[g]) < 8
                scale = float(want[:, cols].abs().max())
                torch.testing.assert_close(got[:, cols], want[:, cols], atol=(2e-2 if few else 2e-4) * scale + 1e-6,
                                           rtol=1e-4)
                torch.testing.assert_close(dgs[g].double().cpu(), dg_t[g],
                                           atol=(2e-2 if few else 2e-3) * float(dg_t[g].abs().max()) + 1e-4, rtol=1e-4)
                torch.testing.assert_close(dbs[g].double().cpu(), db_t[g], atol=2e-3 * float(db_t[g].abs().max()) + 1e-4,
                                           rtol=1e-4)
        else:
            for g in range(nseg):                       # eval: the running buffers are read, not written
                assert torch.equal(rm[g], rms[g]) and torch.equal(rv[g], rvs[g])


def test_segmented_batchnorm_rejects_bad_segments():
    from ds2hip import lib, ops
    x = torch.zeros(2, 4, 8, device='cuda')
    one = torch.ones(8, device='cuda')
    # an empty segment, segments that stop short of B or start past 0, more than 8 segments
    for bounds in ([0, 2, 2, 4], [0, 3], [1, 4], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]):
        nseg = len(bounds) - 1
        xx = x if bounds[-1] <= 4 else torch.zeros(2, bounds[-1], 8, device='cuda')
        with pytest.raises(lib.Ds2Error):
            ops.bn1d_seg_apply(xx, None, torch.zeros(nseg, 16, device='cuda'), 2, xx.shape[1], 8, bounds, [one] * nseg,
                               [one] * nseg)


# ------------------------------------------------------------------------------------------------ model vs reference
def _mt_model():
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': dict(MT_KW)}))
    model.load_state_dict(seeded_state_dict(model, 1234))
    return model.to('cuda')


def _batch_lists(batch):
    """mt_batch/traj_batches items -> the trainer's per-task lists."""
    xs, tg, pct, sz = [], [], [], []
    for item in batch:
        if item is None:
            for lst in (xs, tg, pct, sz):
                lst.append(None)
            continue
        x, labels, ll, lens = item
        xs.append(torch.from_numpy(x))
        tg.append(torch.from_numpy(labels).int())
        pct.append(torch.tensor([n / float(MT_TIN) for n in lens], dtype=torch.float32))
        sz.append(torch.tensor(ll, dtype=torch.int32))
    return xs, tg, pct, sz


def test_multitask_model_against_reference_golden(golden_dir):
    from codes.ctc import CTCLoss
    g = np.load(os.path.join(golden_dir, 'multitask', 'ref_mt_tiny.npz'))
    model = _mt_model()
    xs, tg, pct, sz = _batch_lists(mt_batch(201))
    model.train()
    outs = model([x.cuda() for x in xs])
    total = 0
    for i, o in enumerate(outs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), g['logits_%d' % i], rtol=0, atol=1e-3)
        out_sizes = (pct[i] * o.shape[1]).int()
        loss = CTCLoss()(o.transpose(0, 1), tg[i], out_sizes, sz[i]) / o.shape[0]
        assert abs(float(loss.item()) - float(g['loss_%d' % i])) <= 1e-4 * abs(float(g['loss_%d' % i])), i
        total = total + MT_WEIGHTS[i] * loss.sum()
    assert abs(float(total.item()) - float(g['loss_total'])) <= 1e-4 * float(g['loss_total'])
    total.backward()
    for k, p in model.named_parameters():
        gn = float(np.sqrt((p.grad.cpu().numpy().astype(np.float64) ** 2).sum()))
        if k in ('base_model.conv.0.bias', 'base_model.conv.3.bias'):
            assert gn < 1e-3 and float(g['gnorm_' + k]) < 1e-3, k
            continue
        assert abs(gn - float(g['gnorm_' + k])) <= 2e-3 * float(g['gnorm_' + k]) + 1e-6, k
        if 'grad_' + k in g.files:
            ref = g['grad_' + k]
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-3 * np.abs(ref).max() + 1e-7, err_msg=k)
        else:
            flat = p.grad.cpu().numpy().reshape(-1)
            ref = g['gsample_' + k]
            np.testing.assert_allclose(flat[::max(1, flat.size // 1024)][:1024], ref, rtol=2e-3,
                                       atol=2e-3 * np.abs(ref).max() + 1e-7, err_msg=k)
    for k, v in model.state_dict().items():
        if 'running' in k:
            np.testing.assert_allclose(v.cpu().numpy(), g['buf_' + k], rtol=1e-4, atol=1e-5, err_msg=k)
        elif 'num_batches' in k:
            assert int(v) == int(g['buf_' + k]), k
    model.eval()
    with torch.no_grad():
        probs = model([x.cuda() for x in xs])
        solo = model([None, xs[1].cuda()])
    for i, p in enumerate(probs):
        np.testing.assert_allclose(p.cpu().numpy(), g['probs_%d' % i], rtol=0, atol=1e-3)
    assert solo[0] is None
    np.testing.assert_allclose(solo[1].cpu().numpy(), g['probs_solo_1'], rtol=0, atol=1e-3)


class _TaskView(object):
    """One task's keys of ref_mt_full_b16.npz under the names tests/golden_cases.py ``check_against_golden`` reads."""

    def __init__(self, g, task, with_grads):
        self.g, self.task = g, task
        per = ('logits', 'probs', 'argmax', 'argmax2', 'near_tie', 'out_sizes')
        self.map = {k: '%s_%d' % (k, task) for k in per}
        self.map['loss_sum'] = 'loss_sum_%d' % task
        self.files = list(self.map) + ['tstride'] + [k for k in g.files if with_grads and k.startswith(('gnorm_', 'gsample_',
                                                                                                        'buf_'))]

    def __getitem__(self, k):
        key = self.map.get(k, k)
        if key not in self.g.files:                         # base parameters go by their single-task names there
            pre = key.split('_', 1)[0] + '_'
            key = pre + 'base_model.' + key[len(pre):]
        return self.g[key]


def test_full_size_multitask_model_against_reference_golden(golden_dir):
    """The default 5 x BiGRU-800 base with the en (29) and pt_BR (43) heads, 8 + 8 utterances (ref_mt_full_b16.npz), at
    the tolerances of the single-task full-size goldens (tests/test_configs_gpu.py)."""
    from codes.ctc import ctc_costs_and_grad
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    from tests.golden.make_golden_multitask import FULL_TIN, full_b16_batch
    from tests.golden_cases import check_against_golden
    g = np.load(os.path.join(golden_dir, 'multitask', 'ref_mt_full_b16.npz'))
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': {}}))
    model.load_state_dict(seeded_state_dict(model, 1234))
    model = model.to('cuda').train()
    batch = full_b16_batch()
    x = torch.from_numpy(np.concatenate([b[0] for b in batch])).cuda()
    present = tuple((i, b[0].shape[0]) for i, b in enumerate(batch))
    costs = []

    def loss_fn(acts):
        grads = []
        for (i, n), a in zip(present, acts):
            pct = torch.tensor([v / float(FULL_TIN) for v in batch[i][3]], dtype=torch.float32)
            out_sizes = (pct * a.shape[0]).int()
            assert np.array_equal(out_sizes.numpy(), g['out_sizes_%d' % i])
            c, d = ctc_costs_and_grad(a, torch.from_numpy(batch[i][1]), out_sizes, torch.tensor(batch[i][2]),
                                      grad_scale=MT_WEIGHTS[i] / n)
            costs.append(float(c.sum().item()))
            grads.append(d)
        return None, grads

    _, acts = model.forward_backward(x, present, loss_fn)
    gflat = model.flat_grad()
    torch.cuda.synchronize()
    # (base parameters under their single-task names: check_against_golden knows conv.{0,3}.bias in front of a BatchNorm)
    names = dict((id(p), k.replace('base_model.', '', 1)) for k, p in model.named_parameters())
    grads = {names[id(p)]: model.base_model._gview(gflat, p).cpu().numpy() for p in model._plist}
    bufs = {k.replace('base_model.', '', 1): v.cpu().numpy() for k, v in model.state_dict().items() if 'running' in k}
    model.eval()
    with torch.no_grad():
        probs = model([x[:8], x[8:]])
    for i, a in enumerate(acts):
        check_against_golden(_TaskView(g, i, i == 0), a.transpose(0, 1).cpu().numpy(), costs[i], grads if i == 0 else {},
                             bufs if i == 0 else {}, probs[i].cpu().numpy(), logit_tol=1e-3, prob_tol=1e-3, gnorm_rtol=2e-3,
                             gsample_rtol=2e-3)


def test_base_without_classifier_returns_the_summed_directions():
    from codes.model import DeepSpeech
    torch.manual_seed(3)
    base = DeepSpeech(include_classifier=False, **MT_KW)
    assert not hasattr(base, 'fc') and not any(k.startswith('fc') for k in base.state_dict())
    base = base.cuda().train()
    x = torch.randn(3, 61, 161, device='cuda')
    h = base(x)
    assert tuple(h.shape) == (26, 3, 32)
    with torch.no_grad():
        acts, _ = base._forward_impl(x, training=True, need_grad=False)
    torch.testing.assert_close(h.detach(), acts[0] + acts[1])
    h.pow(2).sum().backward()                           # autograd from d(h) of the top layer
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in base.parameters())
    assert float(base.rnns[0].rnn.weight_ih_l0.grad.abs().sum()) > 0


@pytest.mark.parametrize('fused', [True, False])
def test_trajectory_matches_reference(golden_dir, fused, caplog):
    """Four steps as the reference's multi-task trainer runs them; step 2 has no en utterance (its head moves on momentum
    alone), step 3 an en transcript that cannot be aligned (en contributes 0 and no gradient, pt_BR trains)."""
    from codes.ctc import CTCLoss
    from codes.engine import create_trainer
    g = np.load(os.path.join(golden_dir, 'multitask', 'ref_mt_traj.npz'))
    model = _mt_model()
    if fused:
        opt = torch.optim.SGD(model.parameters(), **TRAJ_OPT)
    else:            # a (negligible) weight decay is not the fused kernel's form -> the reference-shaped autograd step
        opt = torch.optim.SGD(model.parameters(), weight_decay=1e-30, **TRAJ_OPT)
    trainer = create_trainer(model, opt, [CTCLoss(), CTCLoss()], 'cuda', max_norm=TRAJ_MAX_NORM,
                             task_weights=list(MT_WEIGHTS))
    assert trainer._fused == fused
    en_tracked = []
    losses, norms = [], []
    for step, batch in enumerate(traj_batches()):
        loss = trainer.update(_batch_lists(batch), defer=(fused and step % 2 == 1))
        losses.append(loss.result() if hasattr(loss, 'result') else loss)     # (a deferred step: resolved here)
        norms.append(trainer.last_grad_norm)
        en_tracked.append(int(model.heads[0].fc[0].module[0].num_batches_tracked))
    trainer.flush()
    losses = [float(v.result()) if hasattr(v, 'result') else float(v) for v in losses]
    np.testing.assert_allclose(losses, g['losses'], rtol=2e-4)
    if fused:
        np.testing.assert_allclose(norms, g['gnorms'], rtol=2e-3)
    assert en_tracked == [1, 2, 2, 3]                   # the absent step leaves the en head's BatchNorm alone
    assert any('inf loss for task 0' in r.message for r in caplog.records)
    for k, p in model.named_parameters():
        flat = p.detach().cpu().numpy().reshape(-1)
        ref = g['wsample_' + k]
        # (4 steps at lr 1e-2 from clipped gradients: the reference's own fp32 conv-gradient noise, ~2e-3 of the largest
        # element, moves with them -- the single-task trajectory goldens see the same)
        np.testing.assert_allclose(flat[::max(1, flat.size // 1024)][:1024], ref, rtol=1e-3,
                                   atol=5e-3 * np.abs(ref).max() + 1e-6, err_msg=k)
        if k in ('base_model.conv.0.bias', 'base_model.conv.3.bias'):
            continue       # a bias in front of a BatchNorm: exactly-zero gradients, both momentum buffers hold round-off only
        mom = opt.state[p]['momentum_buffer'].detach().cpu().numpy().reshape(-1)
        ref = g['msample_' + k]
        np.testing.assert_allclose(mom[::max(1, mom.size // 1024)][:1024], ref, rtol=2e-3,
                                   atol=5e-3 * np.abs(ref).max() + 1e-6, err_msg='momentum ' + k)
    for k, v in model.state_dict().items():
        if 'running' in k:
            ref = g['buf_' + k]         # (statistics of activations of the weights above: the same band)
            np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=5e-3, atol=1e-3 * np.abs(ref).max() + 1e-5, err_msg=k)


def test_multitask_evaluator_reports_per_task_lists():
    from codes.decoder import GreedyDecoder
    from codes.engine import create_evaluator
    model = _mt_model()
    xs, tg, pct, sz = _batch_lists(mt_batch(201))
    labels_en = ['_', ' ', "'"] + [chr(65 + i) for i in range(26)]
    labels_pt = labels_en + [chr(0xC0 + i) for i in range(14)]
    ev = create_evaluator(model, None, 'cuda', decoder=[GreedyDecoder(labels_en), GreedyDecoder(labels_pt)])
    res = ev.run([(xs, tg, pct, sz), ([None, xs[1]], [None, tg[1]], [None, pct[1]], [None, sz[1]])])
    assert set(res) == {'ctcloss', 'wer', 'cer'}
    assert all(isinstance(v, list) and len(v) == 2 for v in res.values())
    assert all(np.isfinite(v).all() and min(v) > 0 for v in res.values())


def _cli_loss(log, epoch, step):
    import re
    m = re.search(r'Epoch: \[%d\]\[%d/\d+\]\tTime [\d.]+\tData [\d.]+\tLoss ([-\d.]+)' % (epoch, step), log)
    assert m, 'no loss line for epoch %d step %d' % (epoch, step)
    return float(m.group(1))


def test_train_cli_multitask_trains_validates_and_resumes(tmp_path):
    """train.py on a two-language config, raw clips through the device frontend (one BatchSpectrogram launch sequence per
    multi-task batch, staged one bin ahead): two epochs with validation (per-task metric lists) and checkpoints; then a
    --continue-from resume of the epoch-1 checkpoint whose first step reproduces the uninterrupted run's loss (weights,
    momentum and BatchNorm buffers all come back); then the shipped augmentation (tempo + gain on the device)."""
    import json
    import subprocess
    import sys
    from tests.test_cli_gpu import ROOT, _corpus
    _corpus(tmp_path)
    cfg = json.loads(json.load(open(os.path.join(ROOT, 'tests', 'golden', 'multitask', 'ref_multitask_configs.json')))
                     ['multi-task.json'])
    cfg['model']['name'] = 'tiny_mt'
    cfg['model']['params'] = dict(MT_KW)
    cfg['training'].update(num_epochs=2, batch_size=3, augment=False, task_weights=[1, 0.5])
    (tmp_path / 'mt.json').write_text(json.dumps(cfg))

    def run(folder, *extra):
        cmd = [sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / 'mt.json'), '--data-dir', str(tmp_path),
               '--train-manifest', str(tmp_path / 'train.csv'), str(tmp_path / 'train.csv'), '--val-manifest',
               str(tmp_path / 'val.csv'), str(tmp_path / 'val.csv'), '--local', '--checkpoint', '--num-workers', '2',
               '--save-folder', str(tmp_path / folder)] + list(extra)
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return out.stderr + out.stdout

    log = run('results')
    assert 'Validation Summary Epoch: [2]' in log and 'Epoch: [1][1/4]' in log
    ckpt = tmp_path / 'results' / 'tiny_mt' / 'model_ckpt_1.pth'
    payload = torch.load(str(ckpt), map_location='cpu', weights_only=False)
    assert 'heads.1.fc.0.module.1.weight' in payload['state_dict'] and 'base_model.conv.0.weight' in payload['state_dict']
    assert payload['state_dict']['heads.1.fc.0.module.1.weight'].shape == (43, 32)
    assert all(len(v[-1]) == 2 for v in payload['val_metrics'].values())       # per-task lists
    assert any('momentum_buffer' in s for s in payload['optimizer']['state'].values())
    assert (tmp_path / 'results' / 'tiny_mt' / 'model_best-ckpt_1.pth').exists()
    resumed = run('resumed', '--continue-from', str(ckpt))
    assert 'Start epoch: 1' in resumed and 'Validation Summary Epoch: [2]' in resumed
    for step in (1, 2):
        want = _cli_loss(log, 2, step)
        assert abs(_cli_loss(resumed, 2, step) - want) <= 1e-3 * abs(want) + 1e-4, step
    cfg['training'].update(num_epochs=1, augment=True)
    (tmp_path / 'mt.json').write_text(json.dumps(cfg))
    aug = run('augmented')
    assert 'Validation Summary Epoch: [1]' in aug
