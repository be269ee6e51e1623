"""train.py with ``training.reverb``: two steps on a tiny synthetic corpus with a tools/make_rir.py set at prob 1.0, alone and
together with ``training.noise``; the checkpoint keeps the block; without the block no Reverb is built."""
import json
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests.noise_ref import write_noise_dir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


BLOCK = {'path': 'rooms', 'prob': 1.0, 'max_rir_seconds': 0.25}       # relative: resolved under --data-dir
NOISE = {'path': 'bg', 'noise_levels': [0.2, 0.4], 'prob': 1.0}


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """Six one-second clips of seeded noise with two-word transcripts (the corpus of tests/test_cli_gpu.py), a
    tools/make_rir.py set under rooms/ and a small noise set under bg/."""
    tmp_path = tmp_path_factory.mktemp('reverb_cli')
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_rir.py'), str(tmp_path / 'rooms'), '--rt60', '0.1',
                        '0.3', '--count', '2', '--seed', '4'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '4 files' in r.stdout, r.stderr[-2000:]
    write_noise_dir(str(tmp_path / 'bg'))
    return tmp_path


def _train(tmp_path, name, **blocks):
    """train.py for one epoch of two steps; returns (log, checkpoint payload), the last training loss checked finite."""
    cfg = json.load(open(os.path.join(ROOT, 'scripts', 'librispeech-from_scratch.json')))
    cfg['model']['name'] = name
    cfg['model']['params'] = {'rnn_hidden_size': 32, 'num_rnn_layers': 2}
    cfg['training'].update(num_epochs=1, batch_size=3, augment=True, **blocks)           # 6 clips: two steps
    (tmp_path / (name + '.json')).write_text(json.dumps(cfg))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / (name + '.json')), '--data-dir',
                          str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                          str(tmp_path / 'val.csv'), '--local', '--checkpoint', '--num-workers', '0', '--save-folder',
                          str(tmp_path / 'results')], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    log = out.stderr + out.stdout
    assert 'Epoch: [1][2/2]' in log
    payload = torch.load(str(tmp_path / 'results' / name / 'model_ckpt_1.pth'), map_location='cpu', weights_only=False)
    assert payload['iteration'] == 2
    loss = float(payload['metrics']['ctcloss'][-1])
    print('%s: two steps, ctcloss %.6f' % (name, loss))
    assert math.isfinite(loss), loss
    return log, payload


def test_train_cli_with_the_reverb_block(corpus):
    log, payload = _train(corpus, 'wet', reverb=BLOCK)
    assert 'Reverberation on the training set: Reverb(' in log and 'files=4' in log and 'prob=1.0' in log
    assert dict(payload['args']['config']['training']['reverb']) == BLOCK


def test_train_cli_with_reverb_and_noise(corpus):
    log, payload = _train(corpus, 'both', reverb=BLOCK, noise=NOISE)
    assert 'Reverberation on the training set: Reverb(' in log
    training = payload['args']['config']['training']
    assert dict(training['reverb']) == BLOCK and dict(training['noise']) == NOISE


def test_train_cli_without_the_block_builds_no_reverb(corpus):
    log, payload = _train(corpus, 'dry')
    assert 'Reverb' not in log and 'reverb' not in payload['args']['config']['training']
