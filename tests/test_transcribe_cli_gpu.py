"""transcribe.py end to end on the six-clip recording of tests/vad_ref.py with an untrained tiny model (seeded weights: the
texts are whatever it says): the segments are the reference's, the JSON is consistent, two runs agree, and the strings and
word times are what the stated batching rule gives in-process."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import vad_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_wav(path, samples, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(samples, '<i2').tobytes())


def _checkpoint(tmp_path):
    from codes.model import DeepSpeech
    from codes.utils import model_utils as mu
    from codes.utils.io_utils import AttrDict
    (tmp_path / 'labels.en.json').write_text(open(os.path.join(ROOT, 'data', 'labels.en.json')).read())
    params = {'rnn_hidden_size': 32, 'num_rnn_layers': 2}
    args = AttrDict({'data_dir': str(tmp_path),
                     'config': {'model': {'name': 'tiny', 'langs': ['en'], 'params': dict(params)}, 'training': {}}})
    torch.manual_seed(11)
    model = DeepSpeech(**params)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    path = str(tmp_path / 'tiny.pth')
    torch.save(mu.make_checkpoint(args, model, opt, None, 0, 0), path)
    return path


def test_transcribe_a_long_recording_and_a_silent_one(tmp_path):
    from codes.align import ForcedAligner
    from codes.decoder import GreedyDecoder
    from codes.segment import Segmenter
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    ckpt = _checkpoint(tmp_path)
    x, clips = ref.six_clip_recording()
    long_wav, silent_wav, empty_wav = (str(tmp_path / f) for f in ('long.wav', 'silent.wav', 'empty.wav'))
    _write_wav(long_wav, x)
    _write_wav(silent_wav, np.zeros(32000, np.int16))
    _write_wav(empty_wav, np.zeros(0, np.int16))
    base = [sys.executable, os.path.join(ROOT, 'transcribe.py'), '--model-path', ckpt, '--data-dir', str(tmp_path),
            '--batch-size', '4']
    texts = []
    for k in range(2):
        out = subprocess.run(base + ['--audio', long_wav, silent_wav, empty_wav, '--output-path',
                                     str(tmp_path / ('out%d.jsonl' % k))],
                             capture_output=True, text=True, env=dict(os.environ), timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        texts.append((tmp_path / ('out%d.jsonl' % k)).read_text())
    assert texts[0] == texts[1]
    recs = [json.loads(ln) for ln in texts[0].splitlines()]
    assert [r['path'] for r in recs] == [long_wav, silent_wav, empty_wav]
    rec, silent, empty = recs

    s = Segmenter()
    nb = -(-len(x) // 160)
    want = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    blocks = want['segs'].tolist()
    assert len(rec['segments']) == len(blocks) == 6
    assert [(g['start'], g['end']) for g in rec['segments']] == [(a / 100.0, b / 100.0) for a, b in blocks]
    assert rec['duration'] == round(len(x) / 16000.0, 3) and rec['speech_seconds'] == want['info'][3] / 100.0
    assert -61.0 < rec['noise_floor_db'] <= -60.0 and -49.0 < rec['threshold_db'] < -48.0
    assert rec['text'] == ' '.join(g['text'] for g in rec['segments'])
    assert any(g['words'] for g in rec['segments'])                      # (the seeded model does write something)
    for g in rec['segments']:
        assert ' '.join(w['word'] for w in g['words']) == ' '.join(g['text'].split())
        last = g['start']
        for w in g['words']:
            assert last <= w['start'] <= w['end'] <= g['end']
            last = w['end']
    # (all zeros: the floor is bin 0, which has no level, and min_db sets the threshold: the lower edge of bin 75)
    assert silent == {'path': silent_wav, 'duration': 2.0, 'noise_floor_db': None, 'threshold_db': -60.51,
                      'speech_seconds': 0.0, 'text': '', 'segments': []}
    assert empty == {'path': empty_wav, 'duration': 0.0, 'noise_floor_db': None, 'threshold_db': None,
                     'speech_seconds': 0.0, 'text': '', 'segments': []}

    # in-process: the same segments, longest first (ties by start) in groups of 4, through the frontend, the model and the
    # greedy decoder
    torch.set_grad_enabled(False)
    try:
        model, _, val_t, target_t = load_model(ckpt, return_transforms=True, data_dir=str(tmp_path))
        model.eval().to('cuda')
        frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
        decoder = GreedyDecoder(target_t[0].label_encoder)
        order = sorted(range(6), key=lambda i: (-(blocks[i][1] - blocks[i][0]), blocks[i][0]))
        assert order != list(range(6))
        got = {}
        for group in (order[:4], order[4:]):
            wavs = [torch.from_numpy(x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])].astype(np.float32)
                                     * np.float32(frontend.scale)).to('cuda') for i in group]
            inputs, pct = frontend(wavs)
            out = model(inputs)
            strings, offsets = decoder.decode(out, pct.mul_(int(out.shape[1])).int())
            for k, i in enumerate(group):
                got[i] = (strings[k][0], offsets[k][0].tolist())
    finally:
        torch.set_grad_enabled(True)
    for i, g in enumerate(rec['segments']):
        text, offs = got[i]
        assert g['text'] == text
        spans, run = [], []
        for c, o in list(zip(text, offs)) + [(' ', -1)]:
            if c == ' ':
                if run:
                    spans.append((run[0], run[-1]))
                run = []
            else:
                run.append(o)
        assert len(spans) == len(g['words'])
        for (a, b), w in zip(spans, g['words']):
            assert w['start'] == round(blocks[i][0] / 100.0 + ForcedAligner.frame_to_seconds(a), 3)
            assert w['end'] == round(blocks[i][0] / 100.0 + (2 * b + 5) / 100.0, 3)


def test_transcribe_refuses_another_sample_rate_by_name(tmp_path):
    ckpt = _checkpoint(tmp_path)
    ok, fast = str(tmp_path / 'ok.wav'), str(tmp_path / 'fast22k.wav')
    _write_wav(ok, np.zeros(1600, np.int16))
    _write_wav(fast, np.zeros(2205, np.int16), rate=22050)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'transcribe.py'), '--model-path', ckpt, '--data-dir',
                          str(tmp_path), '--audio', ok, fast, '--output-path', str(tmp_path / 'out.jsonl')],
                         capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode != 0
    assert 'fast22k.wav' in out.stderr and '22050' in out.stderr
