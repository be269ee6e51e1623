"""--nbest in test.py and transcribe.py: a tiny model is trained as tests/test_beam_cli_gpu.py trains it; the Test Summary
stays that of the run without the flag, the Oracle Summary equals what the --nbest-path lines give, the flag is refused by
name with another decoder or an N past the beam width, and transcribe.py's segments gain ``alternatives`` while everything
else stays byte for byte."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_beam_cli_gpu import _summary
from tests.test_cli_gpu import _corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp('nbest_cli')
    _corpus(d)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(d / 'tiny.json'), '--data-dir', str(d),
                          '--train-manifest', str(d / 'train.csv'), '--val-manifest', str(d / 'val.csv'), '--local',
                          '--checkpoint', '--num-workers', '0', '--save-folder', str(d / 'results')],
                         capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return d, str(d / 'results' / 'tiny' / 'model_ckpt_2.pth')


def _test_py(trained, extra):
    d, ckpt = trained
    return subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '--model-path', ckpt, '--data-dir', str(d),
                           '--manifest', str(d / 'val.csv'), '--batch-size', '2', '--num-workers', '0', '--beam-width', '8']
                          + extra, capture_output=True, text=True, env=dict(os.environ), timeout=600)


def _oracle(out):
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('Oracle Summary')]
    assert len(lines) == 1, out.stdout
    return lines[0]


def test_the_oracle_summary_and_the_jsonl(trained, tmp_path):
    from codes.decoder import Decoder
    plain_run = _test_py(trained, ['--decoder', 'beam', '--beam-device'])
    plain = _summary(plain_run)
    assert 'Oracle Summary' not in plain_run.stdout
    path = tmp_path / 'f.jsonl'
    out = _test_py(trained, ['--decoder', 'beam', '--nbest', '4', '--nbest-path', str(path)])
    assert _summary(out) == plain                                           # alternative 0 is the 1-best: text and value
    recs = [json.loads(ln) for ln in path.read_text().splitlines()]
    d = trained[0]
    n_utt = len([ln for ln in (d / 'val.csv').read_text().splitlines() if ln.strip()])
    assert len(recs) == n_utt and all(list(r) == ['reference', 'alternatives'] for r in recs)
    dec = Decoder(['_', 'A'])                                               # wer / cer are the base class's
    wer = cer = best_wer = best_cer = words = chars = 0
    for r in recs:
        alts = r['alternatives']
        assert 1 <= len(alts) <= 4 and all(list(a) == ['text', 'score', 'ctc_logp', 'posterior'] for a in alts)
        scores = [a['score'] for a in alts]
        assert all(x >= y for x, y in zip(scores, scores[1:])) and len({a['text'] for a in alts}) == len(alts)
        assert abs(sum(a['posterior'] for a in alts) - 1.0) <= 1e-9
        ref = r['reference']
        wer += dec.wer(alts[0]['text'], ref)
        cer += dec.cer(alts[0]['text'], ref)
        best_wer += min(dec.wer(a['text'], ref) for a in alts)
        best_cer += min(dec.cer(a['text'], ref) for a in alts)
        words += len(ref.split())
        chars += len(ref)
    assert any(len(r['alternatives']) == 4 for r in recs)
    assert plain == 'Test Summary \tAverage WER {:.3f}\tAverage CER {:.3f}\t'.format(100.0 * wer / max(1, words),
                                                                                  100.0 * cer / max(1, chars))
    assert _oracle(out) == 'Oracle Summary \tN-best 4\tOracle WER {:.3f}\tOracle CER {:.3f}\t'.format(
        100.0 * best_wer / max(1, words), 100.0 * best_cer / max(1, chars))
    assert best_wer <= wer and best_cer <= cer                              # oracle <= summary
    # --nbest 1: the two lines carry equal numbers; and the flag combines with --hotword (a weight of 0 changes nothing)
    one_path = tmp_path / 'one.jsonl'
    one = _test_py(trained, ['--decoder', 'beam', '--nbest', '1', '--hotword', 'hello world', '--hotword-weight', '0',
                             '--nbest-path', str(one_path)])
    assert _summary(one) == plain
    assert _oracle(one).split('\t')[2:] == [f.replace('Average', 'Oracle') for f in plain.split('\t')[1:]]
    ones = [json.loads(ln) for ln in one_path.read_text().splitlines()]
    assert [(r['reference'], r['alternatives'][0]['text']) for r in ones] == \
        [(r['reference'], r['alternatives'][0]['text']) for r in recs]
    assert all(len(r['alternatives']) == 1 and r['alternatives'][0]['posterior'] == 1.0 for r in ones)
    assert [r['alternatives'][0]['score'] for r in ones] == [r['alternatives'][0]['score'] for r in recs]


def test_the_flag_is_refused_by_name(trained, tmp_path):
    out = _test_py(trained, ['--decoder', 'greedy', '--nbest', '2'])
    assert out.returncode != 0 and '--nbest needs --decoder beam' in out.stderr and 'Test Summary' not in out.stdout
    out = _test_py(trained, ['--decoder', 'beam', '--nbest', '9'])
    assert out.returncode != 0 and '--nbest 9' in out.stderr and '1..8' in out.stderr and 'Test Summary' not in out.stdout
    out = _test_py(trained, ['--decoder', 'greedy', '--nbest-path', str(tmp_path / 'x.jsonl')])
    assert out.returncode != 0 and '--nbest-path needs --decoder beam' in out.stderr


def test_transcribe_writes_the_alternatives(trained, tmp_path):
    d, ckpt = trained
    base = [sys.executable, os.path.join(ROOT, 'transcribe.py'), '--model-path', ckpt, '--data-dir', str(d), '--audio',
            str(d / 'u0.wav'), str(d / 'u1.wav'), '--decoder', 'beam', '--beam-width', '8']
    text = {}
    for name, extra in (('plain', ['--beam-device']), ('nbest', ['--nbest', '3'])):
        path = tmp_path / (name + '.jsonl')
        out = subprocess.run(base + extra + ['--output-path', str(path)], capture_output=True, text=True,
                             env=dict(os.environ), timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        text[name] = path.read_text()
    recs = [json.loads(ln) for ln in text['nbest'].splitlines()]
    plain = [json.loads(ln) for ln in text['plain'].splitlines()]
    assert len(recs) == 2 and sum(len(r['segments']) for r in recs) >= 1
    stripped = []
    for rec, old in zip(recs, plain):
        assert list(rec) == list(old) + ['nbest'] and rec['nbest'] == 3 and 'nbest' not in old
        for seg, old_seg in zip(rec['segments'], old['segments']):
            assert list(seg) == list(old_seg) + ['alternatives'] and 'alternatives' not in old_seg
            alts = seg.pop('alternatives')
            assert seg == old_seg                                           # text, words and times are the 1-best's
            assert 1 <= len(alts) <= 3 and all(list(a) == ['text', 'score', 'posterior'] for a in alts)
            assert alts[0]['text'] == seg['text'] and abs(sum(a['posterior'] for a in alts) - 1.0) <= 1e-9
            assert all(x['score'] >= y['score'] for x, y in zip(alts, alts[1:]))
        del rec['nbest']
        stripped.append(json.dumps(rec) + '\n')
    assert ''.join(stripped) == text['plain']                               # nothing else moved: byte for byte
    for extra, reason in ((['--decoder', 'greedy', '--nbest', '2'], '--nbest needs --decoder beam'),
                          (['--nbest', '9'], '--nbest 9')):
        out = subprocess.run(base + extra + ['--output-path', str(tmp_path / 'x.jsonl')], capture_output=True, text=True,
                             env=dict(os.environ), timeout=600)
        assert out.returncode != 0 and reason in out.stderr
