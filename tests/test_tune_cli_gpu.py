"""tune_lm.py end to end: a tiny model is trained, an LM built by tools/make_lm.py, a 2 x 2 grid tuned; grid entries equal
the Test Summary of test.py runs with the same weights, and the refusals have their texts."""
import json
import os
import re
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
    m = re.search(r'Average WER (\S+)\tAverage CER (\S+)', lines[0])
    return m.group(1), m.group(2)


def test_tune_lm_against_test_py(tmp_path):
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
    common = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--manifest', str(tmp_path / 'val.csv'), '--batch-size', '2',
              '--num-workers', '0', '--beam-width', '8']
    tune = [sys.executable, os.path.join(ROOT, 'tune_lm.py')] + common + ['--lm-path', lm, '--lm-unit', 'char']
    test = [sys.executable, os.path.join(ROOT, 'test.py')] + common + ['--decoder', 'beam']
    run = lambda cmd: subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)      # noqa: E731

    table = str(tmp_path / 'tune.json')
    out = run(tune + ['--alphas', '0,0.9', '--betas', '0:1.2:1.2', '--rows-per-launch', '4', '--output-path', table])
    assert out.returncode == 0, out.stderr[-3000:]
    rep = json.load(open(table))
    assert [(e['alpha'], e['beta']) for e in rep['grid']] == [(0.0, 0.0), (0.0, 1.2), (0.9, 0.0), (0.9, 1.2)]
    for key in ('manifest', 'utterances', 'ref_words', 'ref_chars', 'beam_width', 'lm_path', 'lm_unit', 'greedy', 'beam_no_lm',
                'best'):
        assert key in rep, key
    assert rep['beam_width'] == 8 and rep['lm_unit'] == 'char' and rep['utterances'] > 0
    best = min(rep['grid'], key=lambda e: (e['word_dist'], e['char_dist'], e['alpha'], e['beta']))
    assert rep['best'] == best
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('Best alpha')]
    assert line == ['Best alpha %g beta %g WER %.3f CER %.3f' % (best['alpha'], best['beta'], best['wer'], best['cer'])]

    fmt = lambda e: ('%.3f' % e['wer'], '%.3f' % e['cer'])                                            # noqa: E731
    for e in (rep['grid'][0], rep['grid'][3]):
        got = _summary(run(test + ['--lm-path', lm, '--lm-unit', 'char', '--alpha', str(e['alpha']), '--beta', str(e['beta'])]))
        assert fmt(e) == got, (e['alpha'], e['beta'])
    assert fmt(rep['beam_no_lm']) == _summary(run(test + ['--beam-device']))

    out = run(tune + ['--alphas', '0', '--betas', '0', '--cache-gb', '0.000001'])
    assert out.returncode != 0 and 'more than --cache-gb 1e-06' in out.stderr and 'pass --cache-gb' in out.stderr
    out = run(tune + ['--alphas', '0:1', '--betas', '0'])
    assert out.returncode == 2 and "--alphas: '0:1' is neither a comma list of numbers nor lo:hi:step" in out.stderr
    out = run(tune + ['--alphas', '0', '--betas', ''])
    assert out.returncode == 2 and '--betas: the list is empty' in out.stderr
