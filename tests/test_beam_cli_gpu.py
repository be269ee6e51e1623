"""test.py with the device beam search: a tiny model is trained, then decoded with an LM built by tools/make_lm.py and
with --beam-device at zero LM weights (same summary as the host beam search)."""
import os
import subprocess
import sys

import pytest

from tests.test_cli_gpu import _corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _summary(out):
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('Test Summary')]
    assert len(lines) == 1, out.stdout
    return lines[0]


def test_train_then_decode_with_the_device_beam_search(tmp_path):
    _corpus(tmp_path)
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / 'tiny.json'), '--data-dir',
                          str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                          str(tmp_path / 'val.csv'), '--local', '--checkpoint', '--num-workers', '0', '--save-folder',
                          str(tmp_path / 'results')], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    ckpt = str(tmp_path / 'results' / 'tiny' / 'model_ckpt_2.pth')
    lm = str(tmp_path / 'char.arpa')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_lm.py'), '--order', '4', '--unit', 'char',
                        '--data-dir', str(tmp_path), '--manifest', str(tmp_path / 'train.csv'), '-o', lm],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    base = [sys.executable, os.path.join(ROOT, 'test.py'), '--model-path', ckpt, '--data-dir', str(tmp_path),
            '--manifest', str(tmp_path / 'val.csv'), '--batch-size', '2', '--num-workers', '0', '--decoder', 'beam',
            '--beam-width', '8']
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, env=env, timeout=600)  # noqa: E731
    assert 'Average CER' in _summary(run(['--lm-path', lm, '--lm-unit', 'char']))
    assert _summary(run(['--beam-device', '--alpha', '0', '--beta', '0'])) == _summary(run([]))
