"""train.py with ``training.speed``: two steps on a tiny synthetic corpus at factors 0.9 / 1.1 with prob 1.0; the same loss
sequence with and without a block whose only factor is 1.0 (the identity copies bit for bit); a bad key fails when the config
is loaded, by name."""
import json
import math
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCK = {'factors': [0.9, 1.1], 'prob': 1.0}


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """Six one-second clips of seeded noise with two-word transcripts (the corpus of tests/test_cli_gpu.py)."""
    tmp_path = tmp_path_factory.mktemp('speed_cli')
    rng = np.random.default_rng(0)
    rows = []
    words = ['hello', 'world', 'speech', 'test', 'amd', 'gpu']
    for i in range(6):
        ns = 16000 + 1700 * i
        with wave.open(str(tmp_path / ('u%d.wav' % i)), 'wb') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(0.1 * rng.standard_normal(ns), -1, 1) * 32767).astype('<i2').tobytes())
        (tmp_path / ('u%d.txt' % i)).write_text(words[i % 6] + ' ' + words[(i + 1) % 6] + '\n')
        rows.append('u%d.wav,u%d.txt,%.3f' % (i, i, ns / 16000.0))
    (tmp_path / 'train.csv').write_text('\n'.join(rows) + '\n')
    (tmp_path / 'val.csv').write_text('\n'.join(rows[:3]) + '\n')
    for f in ('labels.en.json', 'labels.pt_BR.json'):
        (tmp_path / f).write_text(open(os.path.join(ROOT, 'data', f)).read())
    return tmp_path


def _run(tmp_path, name, augment, lr=None, **blocks):
    cfg = json.load(open(os.path.join(ROOT, 'scripts', 'librispeech-from_scratch.json')))
    if lr is not None:
        cfg['optimizer']['params']['lr'] = lr
    cfg['model']['name'] = name
    cfg['model']['params'] = {'rnn_hidden_size': 32, 'num_rnn_layers': 2}
    cfg['training'].update(num_epochs=1, batch_size=3, augment=augment, **blocks)           # 6 clips: two steps
    (tmp_path / (name + '.json')).write_text(json.dumps(cfg))
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / (name + '.json')), '--data-dir',
                           str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                           str(tmp_path / 'val.csv'), '--local', '--checkpoint', '--num-workers', '0', '--save-folder',
                           str(tmp_path / 'results')], capture_output=True, text=True, env=dict(os.environ), timeout=600)


def _step_losses(log):
    """The per-step losses train.py logs, as printed."""
    return re.findall(r'Epoch: \[\d+\]\[\d+/\d+\].*?Loss (\S+)', log)


def _train(tmp_path, name, augment=True, lr=None, **blocks):
    """train.py for one epoch of two steps; returns (log, checkpoint payload), every training loss checked finite."""
    out = _run(tmp_path, name, augment, lr, **blocks)
    assert out.returncode == 0, out.stderr[-3000:]
    log = out.stderr + out.stdout
    assert 'Epoch: [1][2/2]' in log
    payload = torch.load(str(tmp_path / 'results' / name / 'model_ckpt_1.pth'), map_location='cpu', weights_only=False)
    assert payload['iteration'] == 2
    losses = [float(v) for v in payload['metrics']['ctcloss']]
    print('%s: ctcloss %s' % (name, losses))
    assert losses and all(math.isfinite(v) for v in losses), losses
    return log, payload


def test_train_cli_with_the_speed_block(corpus):
    log, payload = _train(corpus, 'fast_slow', speed=BLOCK)
    assert 'Speed perturbation on the training set: SpeedPerturb(' in log and '(0.9, 1.1)' in log and 'prob=1.0' in log
    assert dict(payload['args']['config']['training']['speed']) == BLOCK


def test_an_identity_block_leaves_the_loss_sequence_as_it_is(corpus):
    """Without the block nothing is built, drawn or launched.  With ``{"factors": [1.0]}`` every clip draws, the stage runs
    and copies bit for bit: the losses of every step are equal, as logged and as the checkpoint keeps them.
    ``augment`` is off in both runs: the speed draws come from the same ``np.random`` stream as the tempo and gain draws, in
    front of them -- tests/test_speed_cpu.py holds that order -- so with ``augment`` on the block would change which tempo
    and gain a clip gets.  The learning rate is 0 in both runs: the backward pass adds with float atomics, whose order
    follows the timing of whatever else is on the device (profiles/trajectory_divergence.txt: two same-seed runs part in the
    last bits from the third step on).  Measured on an MI355X at the config's own learning rate: the first step's loss is
    equal (130.6338), and one more launch on the prefetch stream moves the SECOND step's loss in the last place (the epoch's
    mean 159.190847 without the block, 159.190837 with it), while two runs without the block gave equal numbers.  With the
    weights held still every step's loss is a forward pass, which is bit-reproducible (tests/test_model_gpu.py), over the
    frontend's output -- the thing the stage could change: 130.6338 and 179.2725 in both runs."""
    log_a, plain = _train(corpus, 'no_block', augment=False, lr=0.0)
    assert 'SpeedPerturb' not in log_a and 'speed' not in plain['args']['config']['training']
    log_b, same = _train(corpus, 'identity', augment=False, lr=0.0, speed={'factors': [1.0]})
    assert 'Speed perturbation on the training set: SpeedPerturb(' in log_b
    a, b = ([float(v) for v in p['metrics']['ctcloss']] for p in (plain, same))
    assert a == b and len(a) >= 1, (a, b)
    steps_a, steps_b = _step_losses(log_a), _step_losses(log_b)
    print('per-step losses: %s / %s' % (steps_a, steps_b))
    assert steps_a == steps_b and len(steps_a) == 2, (steps_a, steps_b)


def test_a_bad_key_fails_when_the_config_is_loaded(corpus):
    out = _run(corpus, 'bad_key', True, speed={'factors': [0.9], 'rates': [1.1]})
    assert out.returncode != 0 and 'training.speed' in out.stderr and 'rates' in out.stderr
    assert not os.path.exists(str(corpus / 'results' / 'bad_key' / 'model_ckpt_1.pth'))
    out = _run(corpus, 'bad_factor', True, speed={'factors': [0.9, 2.5]})
    assert out.returncode != 0 and '2.5' in out.stderr
