"""search.py end to end on the six-clip recording of tests/vad_ref.py with an untrained tiny model (seeded weights: what it
"hears" is arbitrary): the JSON lines are what the stated segmentation, batching and placement rules and tests/kws_ref.py
give from the model's own probabilities, in-process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import kws_ref
from tests import vad_ref as ref
from tests.test_transcribe_cli_gpu import _checkpoint, _write_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_a_long_recording_and_a_silent_one(tmp_path):
    from codes.segment import Segmenter
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    ckpt = _checkpoint(tmp_path)
    x, _ = ref.six_clip_recording()
    long_wav, silent_wav = str(tmp_path / 'long.wav'), str(tmp_path / 'silent.wav')
    _write_wav(long_wav, x)
    _write_wav(silent_wav, np.zeros(32000, np.int16))
    kw_file = tmp_path / 'kw.txt'
    kw_file.write_text('the cat\n\non\n')
    per_char, max_hits = -3.0, 2
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'search.py'), '--model-path', ckpt, '--data-dir', str(tmp_path),
                          '--batch-size', '4', '--audio', long_wav, silent_wav, '--keyword', 'a!', '--keywords',
                          str(kw_file), '--min-score-per-char', str(per_char), '--max-hits', str(max_hits),
                          '--output-path', str(tmp_path / 'out.jsonl')],
                         capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    rec, silent = [json.loads(ln) for ln in (tmp_path / 'out.jsonl').read_text().splitlines()]
    phrases = ['A', 'THE CAT', 'ON']
    assert silent == {'path': silent_wav, 'duration': 2.0, 'noise_floor_db': None, 'threshold_db': -60.51,
                      'speech_seconds': 0.0, 'keywords': phrases, 'truncated': 0, 'hits': []}

    s = Segmenter()
    nb = -(-len(x) // 160)
    want = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    blocks = want['segs'].tolist()
    assert len(blocks) == 6
    assert list(rec) == ['path', 'duration', 'noise_floor_db', 'threshold_db', 'speech_seconds', 'keywords', 'truncated',
                         'hits']
    assert rec['path'] == long_wav and rec['keywords'] == phrases
    assert rec['duration'] == round(len(x) / 16000.0, 3) and rec['speech_seconds'] == want['info'][3] / 100.0

    # in-process: the same segments, longest first (ties by start) in groups of 4, through the frontend and the model; the
    # log of its probabilities (taken on the device, as the searcher takes it) goes to the reference
    alphabet = json.load(open(os.path.join(ROOT, 'data', 'labels.en.json')))
    labels = [[alphabet.index(c) for c in p] for p in phrases]
    torch.set_grad_enabled(False)
    try:
        model, _, val_t, _ = load_model(ckpt, return_transforms=True, data_dir=str(tmp_path))
        model.eval().to('cuda')
        frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
        order = sorted(range(6), key=lambda i: (-(blocks[i][1] - blocks[i][0]), blocks[i][0]))
        found = {}
        for group in (order[:4], order[4:]):
            wavs = [torch.from_numpy(x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])].astype(np.float32)
                                     * np.float32(frontend.scale)).to('cuda') for i in group]
            inputs, pct = frontend(wavs)
            probs = model(inputs)
            sizes = pct.mul_(int(probs.shape[1])).int().tolist()
            logp = torch.log(probs.float()).cpu().numpy()
            for j, i in enumerate(group):
                found[i] = [kws_ref.search_pair(logp[j], sizes[j], lab, np.float64(per_char) * len(lab)) for lab in labels]
    finally:
        torch.set_grad_enabled(True)
    hits, truncated = [], 0
    for i in range(6):
        for k, pair in enumerate(found[i]):
            truncated += len(pair) > max_hits
            for a, b, score in pair[:max_hits]:
                hits.append({'keyword': phrases[k], 'start': round(blocks[i][0] / 100.0 + (2 * a + 5) * 0.01, 3),
                             'end': round(blocks[i][0] / 100.0 + (2 * b + 5) * 0.01, 3), 'score': score,
                             'score_per_char': score / len(labels[k]), 'segment': i})
    hits.sort(key=lambda h: (h['start'], phrases.index(h['keyword'])))
    assert rec['truncated'] == truncated and truncated > 0
    assert len(rec['hits']) == len(hits) > 0
    assert rec['hits'] == hits


def test_search_refuses_another_sample_rate_by_name(tmp_path):
    ckpt = _checkpoint(tmp_path)
    ok, fast = str(tmp_path / 'ok.wav'), str(tmp_path / 'cd44k.wav')
    _write_wav(ok, np.zeros(1600, np.int16))
    _write_wav(fast, np.zeros(4410, np.int16), rate=44100)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'search.py'), '--model-path', ckpt, '--data-dir', str(tmp_path),
                          '--audio', ok, fast, '--keyword', 'cat', '--output-path', str(tmp_path / 'out.jsonl')],
                         capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode != 0
    assert 'cd44k.wav' in out.stderr and '44100' in out.stderr
    assert not os.path.exists(str(tmp_path / 'out.jsonl'))
