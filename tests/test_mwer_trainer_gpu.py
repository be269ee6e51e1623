"""The ``training.mwer`` block through the Trainer and train.py: steps run and report finite values, the fused path and the
autograd path (``MWERLoss`` through ``loss.backward()``) give the same gradient, and without the block nothing changes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.model import OracleDeepSpeech, seeded_state_dict  # noqa: E402
from tests import ctc_cases as cc  # noqa: E402
from tests.golden.make_golden import seeded_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KWARGS = dict(rnn_hidden_size=32, num_rnn_layers=2, num_classes=29)       # the small model of tests/test_model_gpu.py
SPACE = 1                                                                 # ' ' in ['_', ' ', "'", 'A', ...]
MWER = {'nbest': 4, 'beam_width': 8, 'ctc_weight': 0.01, 'risk': 'word'}


def _build(seed=1234):
    from codes.model import DeepSpeech
    shapes = OracleDeepSpeech(**KWARGS)
    model = DeepSpeech(**KWARGS)
    model.load_state_dict(seeded_state_dict(shapes, seed))
    return model.to('cuda')


def _sgd(model, fused=True):
    if fused:
        return torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    # a (negligible) weight decay is not the fused kernel's form -> the reference-shaped autograd step
    return torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-30)


def _batch():
    x = torch.from_numpy(seeded_inputs(5, 3, 80))
    labels = torch.tensor([3, 4, 1, 5, 6, 7, 1, 8, 9, 10, 11, 1, 12], dtype=torch.int32)
    return x, labels, torch.tensor([1.0, 0.9, 0.8]), torch.tensor([5, 3, 5], dtype=torch.int32)


@pytest.mark.parametrize('fused', [True, False])
def test_three_steps_with_the_block_report_finite_values(fused):
    from codes.ctc import CTCLoss
    from codes.engine import Trainer
    model = _build()
    trainer = Trainer(model, _sgd(model, fused), CTCLoss(), device='cuda', max_norm=5.0, mwer=dict(MWER), space_id=SPACE)
    assert trainer._fused == fused and trainer.last_expected_risk is None
    for _ in range(3):
        loss = trainer.update(_batch())
        risk = trainer.last_expected_risk
        print('loss %.4f expected risk %.4f' % (loss, risk))
        assert np.isfinite(loss) and np.isfinite(risk) and 0.0 <= risk <= 13.0 and loss >= risk
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_fused_and_autograd_paths_give_the_same_gradient():
    """Both paths run the same device chain on the same activations; d loss / d acts may differ by the kernel's own
    error on each side, i.e. by at most twice the derived condition of tests/test_mwer_gpu.py (x grad_scale = 1/B).  The
    backward pass is the same code on both paths and linear in d_acts: the flat gradients are held to 1e-4 of the flat
    gradient's largest entry (the relative tolerance tests/test_model_gpu.py holds a trainer step to; relative to the
    whole gradient, not to each parameter: a bias in front of a BatchNorm has a gradient that cancels to ~1e-8, and what
    is left of it is the rounding of the terms that cancelled).  Character risk: an untrained model's hypotheses hold no
    space, so their word distances are all equal and the MWER part would vanish."""
    from codes.ctc import MWERLoss
    from codes.engine import Trainer, sanitize_inputs
    x, labels, pct, sizes = _batch()
    bsz = x.shape[0]
    fused = _build()
    block = dict(MWER, risk='char')
    trainer = Trainer(fused, _sgd(fused), device='cuda', mwer=block, space_id=SPACE)
    seen = {}
    inner = trainer._mwer_loss_fn(labels, pct, sizes, bsz)

    def loss_fn(acts):
        loss, d_acts = inner(acts)
        seen['d_acts'], seen['acts'] = d_acts.clone(), acts.clone()
        return loss, d_acts
    fused.train()
    costs, _ = trainer._forward_backward(x.to('cuda'), loss_fn, None)
    torch.cuda.synchronize()
    g_fused = [fused._gview(fused.flat_grad(), p).clone() for p in fused._plist]

    auto = _build()
    auto.train()
    crit = MWERLoss(SPACE, **block)
    out = auto(x.to('cuda'))                                              # (B,T,A)
    out.register_hook(lambda g: seen.__setitem__('d_out', g.clone()))
    out_sizes = sanitize_inputs(out.shape[1], pct)
    loss = (crit(out.transpose(0, 1), labels, out_sizes, sizes) / bsz).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(costs.sum()) / bsz) <= 1e-5 * max(1.0, abs(float(loss.detach())))
    info = crit.last_info
    post, risk = info['posterior'].double().cpu().numpy(), info['risk'].double().cpu().numpy()
    exp_risk, count = info['exp_risk'].double().cpu().numpy(), info['count'].cpu().numpy()
    d_fused, d_auto = seen['d_acts'].cpu().numpy(), seen['d_out'].transpose(0, 1).cpu().numpy()
    fam = cc.BOUNDS['main']
    for b in range(bsz):
        k = int(count[b])
        live = post[b, :k] > 0
        s_w = MWER['ctc_weight'] + float(np.sum(post[b, :k] * np.abs(risk[b, :k] - exp_risk[b])))
        spread = float(risk[b, :k][live].max() - risk[b, :k][live].min()) if live.any() else 0.0
        cond = s_w * fam['grad_max'] + 2.0 * spread * 2.0 * fam['cost_per_frame'] * int(out_sizes[b])
        err = float(np.abs(d_fused[:, b] - d_auto[:, b]).max()) * bsz
        print('utterance %d: fused - autograd %.2e, 2 x condition %.2e' % (b, err, 2 * cond))
        assert err <= 2.0 * cond
    assert any(len(set(risk[b, :int(count[b])].tolist())) > 1 for b in range(bsz))        # the MWER part is not zero
    scale = max(float(g.abs().max()) for g in g_fused)
    assert scale > 0.0
    for gf, q in zip(g_fused, auto._plist):
        assert float((gf - q.grad).abs().max()) <= 1e-4 * scale


def _two_steps(frozen_conv=False, **kwargs):
    from codes.engine import Trainer
    model = _build()
    if frozen_conv:                                # fine-tuning's ``freeze_layers: ["conv"]`` (training_utils.py:52-54)
        for p in model.conv.parameters():
            p.requires_grad_(False)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, nesterov=True)
    trainer = Trainer(model, opt, device='cuda', max_norm=5.0, **kwargs)
    assert trainer._fused
    for _ in range(2):
        trainer.update(_batch())
    assert trainer.mwer is None and trainer.last_expected_risk is None
    return model._flat_p.clone()


def test_without_the_block_the_parameters_are_bit_identical():
    """``mwer=None`` against a trainer built without the argument, two steps from the same seed, bit for bit.

    The conv layers are frozen in every trainer here, as a fine-tuning config's ``freeze_layers`` does it, because that is
    the setting in which the step itself is bit-reproducible and the comparison can tell anything: the conv weight and bias
    gradients (csrc/conv.hip) are summed over row splits with float atomics in an order that changes from run to run, and
    through the clip coefficient their last bits reach every parameter -- two trainers built the same way, conv layers
    trainable, differ by 1.5e-08 after two steps.  At this size (T B = 105 rows, below the split-K threshold of 512) no
    other gradient is touched by an atomic from more than one workgroup: with the conv layers frozen every parameter's
    gradient is the same bits run after run.  That is asserted first, as the precondition; then the argument."""
    plain, again = _two_steps(frozen_conv=True), _two_steps(frozen_conv=True)
    assert torch.equal(plain.view(torch.int32), again.view(torch.int32)), 'the step is not bit-reproducible here'
    none = _two_steps(frozen_conv=True, mwer=None, space_id=SPACE)
    assert torch.equal(plain.view(torch.int32), none.view(torch.int32))
    fresh = _build()
    fresh._ensure_flat()
    assert not torch.equal(plain, fresh._flat_p)                           # and the two steps did move the parameters


def test_without_the_block_the_same_calls_are_made(monkeypatch):
    """Without the block nothing changes: a trainer built with ``mwer=None`` makes exactly the library calls, in the same
    order, that one built without the argument makes, none of them the MWER entry or the N-best search, and never reaches
    ``mwer_costs_and_grad``."""
    from codes import engine
    from ds2hip import lib

    def boom(*args, **kwargs):
        raise AssertionError('mwer_costs_and_grad was called without the block')
    monkeypatch.setattr(engine, 'mwer_costs_and_grad', boom)
    real, names = lib.call, []

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', call)
    seqs = []
    for kwargs in ({}, {'mwer': None, 'space_id': SPACE}):
        del names[:]
        _two_steps(**kwargs)
        seqs.append(list(names))
    assert seqs[0] == seqs[1] and len(seqs[0]) > 20
    assert 'ds2_ctc_loss_grad' in seqs[0]
    assert not {'ds2_ctc_mwer_grad', 'ds2_ctc_beam_search_nbest', 'ds2_edit_stats'} & set(seqs[0])


def test_refusals_multi_task_and_missing_space():
    from codes.engine import Trainer, create_trainer
    from codes.model import DeepSpeech, MultiTaskModel, SequenceWiseClassifier
    model = _build()
    with pytest.raises(ValueError, match='space'):
        Trainer(model, _sgd(model), device='cuda', mwer={}, space_id=-1)
    with pytest.raises(ValueError, match='unknown'):
        Trainer(model, _sgd(model), device='cuda', mwer={'nbets': 2}, space_id=SPACE)
    Trainer(model, _sgd(model), device='cuda', mwer={'risk': 'char'}, space_id=-1)
    base = DeepSpeech(rnn_hidden_size=32, num_rnn_layers=2, include_classifier=False)
    multi = MultiTaskModel(base, [SequenceWiseClassifier(32, 29), SequenceWiseClassifier(32, 43)]).to('cuda')
    with pytest.raises(ValueError, match='multi-task'):
        create_trainer(multi, _sgd(multi), None, 'cuda', task_weights=[1, 1], mwer={}, space_id=SPACE)


def test_train_cli_runs_with_the_block(tmp_path):
    from tests.test_cli_gpu import _corpus
    _corpus(tmp_path)
    cfg = json.load(open(str(tmp_path / 'tiny.json')))
    cfg['training'].update(num_epochs=1, mwer={'nbest': 2, 'beam_width': 4})
    (tmp_path / 'tiny.json').write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / 'tiny.json'), '--data-dir',
                          str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                          str(tmp_path / 'val.csv'), '--local', '--num-workers', '0', '--save-folder',
                          str(tmp_path / 'results')], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    log = out.stderr + out.stdout
    assert 'MWER fine-tuning' in log and 'Epoch: [1][2/2]' in log and 'Validation Summary Epoch: [1]' in log
    cfg['training']['mwer'] = {'nbest': 9}
    (tmp_path / 'bad.json').write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / 'bad.json'), '--data-dir',
                          str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                          str(tmp_path / 'val.csv'), '--local', '--num-workers', '0', '--save-folder',
                          str(tmp_path / 'results')], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode != 0 and 'training.mwer: nbest 9 is outside 1..beam_width = 8' in out.stderr
