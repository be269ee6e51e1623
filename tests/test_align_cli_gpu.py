"""align.py end to end: a tiny model is trained on the tiny corpus of tests/test_cli_gpu.py, then its six clips
are aligned, scored and pruned."""
import json
import os
import subprocess
import sys
import wave

import pytest

from tests.test_cli_gpu import _corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_then_align_and_prune(tmp_path):
    from ds2hip import ops
    _corpus(tmp_path)
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(tmp_path / 'tiny.json'), '--data-dir',
                          str(tmp_path), '--train-manifest', str(tmp_path / 'train.csv'), '--val-manifest',
                          str(tmp_path / 'val.csv'), '--local', '--checkpoint', '--num-workers', '0', '--save-folder',
                          str(tmp_path / 'results')], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    ckpt = str(tmp_path / 'results' / 'tiny' / 'model_ckpt_2.pth')
    manifest = tmp_path / 'train.csv'                               # six clips: three minibatches of two
    rows = [ln for ln in manifest.read_text().splitlines() if ln.strip()]
    base = [sys.executable, os.path.join(ROOT, 'align.py'), '--model-path', ckpt, '--data-dir', str(tmp_path),
            '--manifest', str(manifest), '--batch-size', '2', '--num-workers', '0']
    jsonl = tmp_path / 'align.jsonl'
    out = subprocess.run(base + ['--output-path', str(jsonl)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(ln) for ln in jsonl.read_text().splitlines()]
    assert len(recs) == len(rows) == 6
    spec_frames = []
    for row in rows:
        with wave.open(str(tmp_path / row.split(',')[0])) as w:
            spec_frames.append(1 + w.getnframes() // 160)
    for k, (row, rec) in enumerate(zip(rows, recs)):
        wav, txt, _ = row.split(',')
        assert rec['path'] == wav
        want = open(str(tmp_path / txt)).read().strip().upper()
        # sizes are the model's output length scaled by each clip's share of its minibatch's longest clip, as in test.py
        pair = spec_frames[k - k % 2:k - k % 2 + 2]
        t_out = ops.conv_out_frames(max(pair))[1]
        assert rec['transcript'] == want and 0 < rec['frames'] <= t_out
        assert rec['frames'] == t_out or spec_frames[k] < max(pair)
        assert rec['score'] is not None and rec['score'] < 0
        assert rec['score_per_frame'] == pytest.approx(rec['score'] / rec['frames'])
        assert ' '.join(w['word'] for w in rec['words']) == ' '.join(want.split())
        assert ''.join(c['char'] for c in rec['chars']) == want
        last = -1
        for c in rec['chars']:
            assert last < c['start_frame'] <= c['end_frame'] < rec['frames']
            last = c['end_frame']
        for item in rec['chars'] + rec['words']:
            assert item['start'] == pytest.approx((2 * item['start_frame'] + 5) / 100.0, abs=1e-9)
            assert item['end'] == pytest.approx((2 * item['end_frame'] + 5) / 100.0, abs=1e-9)
        i = 0
        for w in rec['words']:
            cs = rec['chars'][i:i + len(w['word'])]
            assert ''.join(c['char'] for c in cs) == w['word']
            assert (w['start_frame'], w['end_frame']) == (cs[0]['start_frame'], cs[-1]['end_frame'])
            i += len(w['word']) + 1
    # prune at the median score per frame: exactly the rows at or above it stay, in manifest order
    thr = sorted(rec['score_per_frame'] for rec in recs)[3]
    pruned = tmp_path / 'pruned.csv'
    out = subprocess.run(base + ['--output-path', str(tmp_path / 'again.jsonl'), '--min-score-per-frame', repr(thr),
                                 '--pruned-manifest', str(pruned)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    again = [json.loads(ln) for ln in (tmp_path / 'again.jsonl').read_text().splitlines()]
    assert [rec['path'] for rec in again] == [rec['path'] for rec in recs]
    kept = pruned.read_text().splitlines()
    assert kept == [row for row, rec in zip(rows, again) if rec['score_per_frame'] >= thr] and 0 < len(kept) < 6
