"""--hotword in test.py and transcribe.py: a tiny model is trained as tests/test_beam_cli_gpu.py trains it; a weight of 0
prints the summary of the run without the flag, the decoder object agrees with the direct ops call, the flags are refused
by name with another decoder or a phrase that cannot be boosted, and transcribe.py's record gains ``hotwords``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_beam_cli_gpu import _summary
from tests.test_cli_gpu import _corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp('bias_cli')
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


def test_a_weight_of_zero_prints_the_summary_of_the_run_without_the_flag(trained):
    plain = _summary(_test_py(trained, ['--decoder', 'beam', '--beam-device']))
    assert 'Average CER' in plain
    assert _summary(_test_py(trained, ['--decoder', 'beam', '--beam-device', '--hotword', 'hello world',
                                       '--hotword-weight', '0'])) == plain
    # the flag alone implies the device search, as --lm-path does
    assert _summary(_test_py(trained, ['--decoder', 'beam', '--hotword', 'hello world', '--hotword-weight', '0'])) == plain


def test_the_flags_are_refused_by_name(trained, tmp_path):
    out = _test_py(trained, ['--decoder', 'greedy', '--hotword', 'hello'])
    assert out.returncode != 0 and '--decoder beam' in out.stderr and 'boost' in out.stderr
    listed = tmp_path / 'words.txt'
    listed.write_text('hello\n\nHELLO!\n')
    for extra, reason in ((['--hotword', ''], 'normalises to nothing'), (['--hotword', 'x' * 65], '65 labels'),
                          (['--hotword', 'amd', '--hotwords', str(listed)], "'HELLO!'")):
        out = _test_py(trained, ['--decoder', 'beam'] + extra)
        assert out.returncode != 0 and 'test.py: PhraseBooster' in out.stderr and reason in out.stderr, out.stderr[-2000:]
        assert 'Test Summary' not in out.stdout


def test_the_decoder_object_agrees_with_the_direct_call(trained):
    from codes.bias import PhraseBooster
    from codes.data import AudioDataLoader, AudioDataset
    from codes.decoder import DeviceBeamCTCDecoder
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    from ds2hip import ops
    d, ckpt = trained
    torch.set_grad_enabled(False)
    try:
        model, _, val_t, target_t = load_model(ckpt, return_transforms=True, data_dir=str(d))
        model.eval().to('cuda')
        target_t = target_t[0]
        loader = AudioDataLoader(AudioDataset(str(d), str(d / 'val.csv'), transforms=val_t, target_transforms=target_t),
                                 batch_size=3, num_workers=0, raw_audio=True)
        frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
        wavs = next(iter(loader))[0]
        inputs, pct = frontend(wavs)
        out = model(inputs)
        sizes = pct.mul_(int(out.shape[1])).int()
    finally:
        torch.set_grad_enabled(True)
    booster = PhraseBooster(target_t, ['hello', 'speech test', ' gpu'], weight=3.0)
    assert booster.keywords == ['HELLO', 'SPEECH TEST', ' GPU']
    dec = DeviceBeamCTCDecoder(target_t.label_encoder, beam_width=8, booster=booster)
    strings, offsets = dec.decode(out, sizes)
    trans, final = booster.tables(out.device)
    labels, offs, lens, score, ctc, bias = [x.cpu().numpy() for x in ops.ctc_beam_search_bias(
        out.contiguous().float(), sizes.to('cuda', torch.int32), 8, trans, final, 3.0)]
    for b in range(out.shape[0]):
        ids = labels[b, :lens[b]]
        assert strings[b][0] == ''.join(target_t.label_encoder.inverse_transform(ids)) if len(ids) else strings[b][0] == ''
        assert offsets[b][0].tolist() == offs[b, :lens[b]].tolist()
        assert bias[b] == booster.graph.walk(ids.tolist())[1]
    assert dec.last_bias_counts == bias.tolist() and dec.last_scores == score.tolist()
    dl, dn = dec.decode_labels(out, sizes)
    assert np.array_equal(dl.cpu().numpy(), labels) and np.array_equal(dn.cpu().numpy(), lens)
    assert dec.last_bias_counts.cpu().tolist() == bias.tolist()
    plain = DeviceBeamCTCDecoder(target_t.label_encoder, beam_width=8)
    plain.decode(out, sizes)
    assert plain.last_bias_counts is None and plain.booster is None
    with pytest.raises(ValueError, match='phrase booster'):
        DeviceBeamCTCDecoder(target_t.label_encoder, blank_index=1, beam_width=8, booster=booster)


def test_transcribe_writes_the_hotwords(trained, tmp_path):
    d, ckpt = trained
    base = [sys.executable, os.path.join(ROOT, 'transcribe.py'), '--model-path', ckpt, '--data-dir', str(d), '--audio',
            str(d / 'u0.wav'), str(d / 'u1.wav'), '--decoder', 'beam', '--beam-width', '8']
    recs = {}
    for name, extra in (('plain', ['--beam-device']), ('hot', ['--hotword', 'hello world', '--hotword', " Don't",
                                                                '--hotword-weight', '0'])):
        path = tmp_path / (name + '.jsonl')
        out = subprocess.run(base + extra + ['--output-path', str(path)], capture_output=True, text=True,
                             env=dict(os.environ), timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        recs[name] = [json.loads(ln) for ln in path.read_text().splitlines()]
    assert len(recs['hot']) == 2
    for plain, hot in zip(recs['plain'], recs['hot']):
        assert list(hot) == list(plain) + ['hotwords'] and hot['hotwords'] == ['HELLO WORLD', " DON'T"]
        assert {k: v for k, v in hot.items() if k != 'hotwords'} == plain          # a weight of 0 changes nothing else
    out = subprocess.run(base[:-4] + ['--hotword', 'hello', '--output-path', str(tmp_path / 'x.jsonl')],
                         capture_output=True, text=True, env=dict(os.environ), timeout=600)
    assert out.returncode != 0 and '--decoder beam' in out.stderr
