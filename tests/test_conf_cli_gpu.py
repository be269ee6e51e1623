"""--confidence in transcribe.py and --confidence-path in test.py, on the untrained seeded tiny model of
tests/test_transcribe_cli_gpu.py (the texts are whatever it says).  The command lines' ``main`` is called in this process.
Without the flag the output is what it was; with it every word carries the value tests/conf_ref.py gives for its labels and
span, and test.py's lines and summary are consistent with ``codes.metrics.word_matches``."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import conf_ref as cr
from tests import vad_ref
from tests.test_cli_gpu import _corpus
from tests.test_transcribe_cli_gpu import _checkpoint, _write_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location('ds2_cli_' + name, os.path.join(ROOT, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def main(argv):
        try:
            return mod.main(argv)
        finally:
            torch.set_grad_enabled(True)                    # (the command lines switch it off for their process)
    return main


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp('conf_cli')
    ckpt = _checkpoint(d)
    x, _ = vad_ref.six_clip_recording()
    wav = str(d / 'long.wav')
    _write_wav(wav, x)
    return d, ckpt, wav, x


def _reference_words(ckpt, d, x, blocks, decoder_kind):
    """per segment: [(word, reference logp, span frames)] from an in-process run of the stated batching rule"""
    from codes.decoder import DeviceBeamCTCDecoder, GreedyDecoder
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    torch.set_grad_enabled(False)
    try:
        model, _, val_t, target_t = load_model(ckpt, return_transforms=True, data_dir=str(d))
        model.eval().to('cuda')
        enc = target_t[0].label_encoder
        classes = [str(c) for c in enc.classes_.tolist()]
        frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
        decoder = GreedyDecoder(enc) if decoder_kind == 'greedy' else DeviceBeamCTCDecoder(enc, beam_width=8)
        order = sorted(range(len(blocks)), key=lambda i: (-(blocks[i][1] - blocks[i][0]), blocks[i][0]))
        out_words = {}
        for group in (order[:4], order[4:]):
            if not group:
                continue
            wavs = [torch.from_numpy(x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])].astype(np.float32)
                                     * np.float32(frontend.scale)).to('cuda') for i in group]
            inputs, pct = frontend(wavs)
            out = model(inputs)
            strings, offsets = decoder.decode(out, pct.mul_(int(out.shape[1])).int())
            probs = out.float().cpu().numpy()
            for k, i in enumerate(group):
                text, offs = strings[k][0], offsets[k][0].tolist()
                labels = [classes.index(c) for c in text]
                words = []
                for first, ln in cr.find_units(labels, classes.index(' ')):
                    span = probs[k, offs[first]:offs[first + ln - 1] + 1]
                    words.append((text[first:first + ln], cr.forward(span, labels[first:first + ln], 0), len(span)))
                out_words[i] = words
    finally:
        torch.set_grad_enabled(True)
    return out_words


@pytest.mark.parametrize('kind', ['greedy', 'beam'])
def test_transcribe_confidence(setup, tmp_path, kind):
    d, ckpt, wav, x = setup
    main = _cli('transcribe')
    base = ['--model-path', ckpt, '--data-dir', str(d), '--batch-size', '4', '--audio', wav, '--decoder', kind,
            '--beam-width', '8']
    plain_path, conf_path = str(tmp_path / 'plain.jsonl'), str(tmp_path / 'conf.jsonl')
    main(base + ['--output-path', plain_path] + (['--beam-device'] if kind == 'beam' else []))
    main(base + ['--output-path', conf_path, '--confidence'])            # (with beam the flag implies the device search)
    plain = json.loads(open(plain_path).read())
    rec = json.loads(open(conf_path).read())
    blocks = [(int(round(g['start'] * 100)), int(round(g['end'] * 100))) for g in rec['segments']]
    want = _reference_words(ckpt, d, x, blocks, kind)
    seen = 0
    for i, g in enumerate(rec['segments']):
        assert [w[0] for w in want[i]] == [w['word'] for w in g['words']]
        for (word, logp, n), w in zip(want[i], g['words']):
            assert list(w) == ['word', 'start', 'end', 'confidence']
            p = math.exp(logp)
            # the kernel's bound on logp carried to P, and the rounding to 4 decimals
            assert abs(w.pop('confidence') - p) <= 0.5e-4 + 1e-12 + p * math.expm1(cr.bound(n, logp)), (word, p)
            seen += 1
    assert seen >= 3                                                       # (the seeded model does write something)
    assert rec == plain                                                    # the two outputs differ only by the new keys
    if kind == 'greedy':
        return
    nbest_path = str(tmp_path / 'nbest.jsonl')
    main(base + ['--output-path', nbest_path, '--confidence', '--nbest', '3'])
    nb = json.loads(open(nbest_path).read())
    for g, g1 in zip(nb['segments'], json.loads(open(conf_path).read())['segments']):
        assert g['words'] == g1['words']
        for alt in g['alternatives']:
            assert list(alt) == ['text', 'score', 'posterior', 'word_confidences']
            assert len(alt['word_confidences']) == len(alt['text'].split())
        assert g['alternatives'][0]['word_confidences'] == [w['confidence'] for w in g['words']]


def _lines(capsys, prefix):
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(prefix)]


@pytest.mark.parametrize('kind', ['greedy', 'beam'])
def test_test_py_confidence_path(setup, tmp_path, capsys, kind):
    from codes.metrics import word_matches
    d, ckpt, _, _ = setup
    if not (d / 'val.csv').exists():
        _corpus(d)
    main = _cli('test')
    base = ['--model-path', ckpt, '--data-dir', str(d), '--manifest', str(d / 'val.csv'), '--batch-size', '2',
            '--num-workers', '0', '--decoder', kind, '--beam-width', '8']
    main(base + (['--beam-device'] if kind == 'beam' else []))
    plain = _lines(capsys, 'Test Summary')
    path = tmp_path / 'c.jsonl'
    main(base + ['--confidence-path', str(path)])
    out = capsys.readouterr().out.splitlines()
    assert [ln for ln in out if ln.startswith('Test Summary')] == plain and len(plain) == 1
    assert out.index(plain[0]) + 1 == [i for i, ln in enumerate(out) if ln.startswith('Confidence Summary')][0]
    recs = [json.loads(ln) for ln in path.read_text().splitlines()]
    refs = [open(str(d / ln.split(',')[1])).read().strip().lower() for ln in (d / 'val.csv').read_text().splitlines() if ln]
    assert [r['reference'].lower() for r in recs] == refs and len(set(refs)) == len(refs)     # manifest order
    n = [0, 0]
    sums = [0.0, 0.0]
    for r in recs:
        assert list(r) == ['reference', 'text', 'words']
        assert [w['word'] for w in r['words']] == r['text'].split()
        assert [w['correct'] for w in r['words']] == word_matches(r['text'].split(), r['reference'].split())
        for w in r['words']:
            assert list(w) == ['word', 'confidence', 'correct'] and 0.0 <= w['confidence'] <= 1.0 + 1e-5
            n[w['correct']] += 1
            sums[w['correct']] += w['confidence']
    line = 'Confidence Summary \twords {}\tcorrect {}\tmean confidence correct {:.3f}\twrong {:.3f}\t'.format(
        n[0] + n[1], n[1], sums[1] / max(1, n[1]), sums[0] / max(1, n[0]))
    assert line in out
    assert n[0] + n[1] >= 1


def test_test_py_refuses_the_flag_without_a_decoder(setup, tmp_path, capsys):
    d, ckpt, _, _ = setup
    with pytest.raises(SystemExit) as err:
        _cli('test')(['--model-path', ckpt, '--data-dir', str(d), '--manifest', str(d / 'val.csv'), '--decoder', 'none',
                      '--confidence-path', str(tmp_path / 'x.jsonl')])
    assert err.value.code != 0
    assert '--confidence-path needs --decoder greedy or beam' in capsys.readouterr().err
