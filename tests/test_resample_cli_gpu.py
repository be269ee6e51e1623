"""``--resample`` end to end with the untrained tiny model of tests/test_transcribe_cli_gpu.py: a 48 kHz stereo (44.1 kHz mono)
recording through transcribe.py (align_long.py) gives the record of the 16 kHz file written from ``ops.resample``'s own
output; a 16 kHz mono file gives its flagless record plus the two new fields; an unsupported rate is refused by name before
any work; and the noise and RIR banks built with ``resample=True`` hold ``ops.resample``'s samples."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import vad_ref
from tests.test_transcribe_cli_gpu import _checkpoint, _write_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSCRIPT = 'the quick brown fox jumps over the lazy dog\n'


def _write(path, samples, rate, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(np.asarray(samples, '<i2').tobytes() if width == 2 else bytes(samples))


def _read(path):
    with wave.open(str(path), 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')


def _held(x, rate):
    """x (16 kHz) at ``rate`` by holding samples: content with the same speech and silence, nothing more is needed."""
    return x[(np.arange(len(x) * rate // 16000, dtype=np.int64) * 16000) // rate]


def _converted(samples, rate, channels):
    from ds2hip import ops
    out, off = ops.resample(torch.from_numpy(np.ascontiguousarray(samples, np.int16)).to('cuda'), [0, len(samples)], rate,
                            channels=channels)
    assert off == [0, out.numel()]
    return out.cpu().numpy()


def _run(script, args, tmp_path):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True,
                          env=dict(os.environ), timeout=600, cwd=str(tmp_path))


def _without(rec, *keys):
    return {k: v for k, v in rec.items() if k not in keys}


def test_transcribe_resample_equals_the_converted_file_and_the_identity(tmp_path):
    ckpt = _checkpoint(tmp_path)
    x, _ = vad_ref.six_clip_recording()
    x48 = _held(x, 48000)
    stereo = np.stack([x48, -(x48 // 2)], axis=1).reshape(-1)                 # interleaved; the mean is about x / 4
    stereo_wav, mono_wav, conv_wav = (str(tmp_path / f) for f in ('stereo48.wav', 'mono16.wav', 'conv16.wav'))
    _write(stereo_wav, stereo, 48000, channels=2)
    _write_wav(mono_wav, x)
    conv = _converted(stereo, 48000, 2)
    assert len(conv) == len(x48) // 3 and np.abs(conv).max() > 1000
    _write_wav(conv_wav, conv)
    base = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--batch-size', '4']
    out = _run('transcribe.py', base + ['--resample', '--audio', stereo_wav, mono_wav, '--output-path',
                                        str(tmp_path / 'res.jsonl')], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    out = _run('transcribe.py', base + ['--audio', conv_wav, mono_wav, '--output-path', str(tmp_path / 'plain.jsonl')], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [json.loads(ln) for ln in (tmp_path / 'res.jsonl').read_text().splitlines()]
    plain = [json.loads(ln) for ln in (tmp_path / 'plain.jsonl').read_text().splitlines()]
    assert (res[0]['path'], res[0]['source_rate'], res[0]['source_channels']) == (stereo_wav, 48000, 2)
    assert _without(res[0], 'path', 'source_rate', 'source_channels') == _without(plain[0], 'path')
    assert res[0]['duration'] == round(len(conv) / 16000.0, 3) and len(res[0]['segments']) > 0
    assert 'source_rate' not in plain[0] and 'source_channels' not in plain[1]
    assert res[1] == dict(plain[1], source_rate=16000, source_channels=1) and len(res[1]['segments']) == 6


def test_transcribe_resample_refuses_an_unsupported_rate_by_name(tmp_path):
    ckpt = _checkpoint(tmp_path)
    ok, odd, wide = str(tmp_path / 'ok.wav'), str(tmp_path / 'odd44056.wav'), str(tmp_path / 'wide24.wav')
    _write(ok, np.zeros(4800, np.int16), 48000)
    _write(odd, np.zeros(4405, np.int16), 44056)
    _write(wide, bytes(3 * 480), 48000, width=3)
    base = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--resample', '--output-path', str(tmp_path / 'out.jsonl')]
    out = _run('transcribe.py', base + ['--audio', ok, odd], tmp_path)
    assert out.returncode != 0 and 'odd44056.wav' in out.stderr and '44056' in out.stderr
    assert not os.path.exists(str(tmp_path / 'out.jsonl'))                    # refused before any work
    out = _run('transcribe.py', base + ['--audio', ok, wide], tmp_path)
    assert out.returncode != 0 and 'wide24.wav' in out.stderr and '24-bit' in out.stderr
    assert not os.path.exists(str(tmp_path / 'out.jsonl'))


def test_align_long_resample_equals_the_converted_file_and_writes_16k_clips(tmp_path):
    ckpt = _checkpoint(tmp_path)
    x, _ = vad_ref.six_clip_recording()
    x44 = _held(x, 44100)
    cd_wav, conv_wav, txt = str(tmp_path / 'talk44.wav'), str(tmp_path / 'talk16.wav'), str(tmp_path / 'talk.txt')
    _write(cd_wav, x44, 44100)
    conv = _converted(x44, 44100, 1)
    _write_wav(conv_wav, conv)
    (tmp_path / 'talk.txt').write_text(TRANSCRIPT)
    # gaps of up to 2 s closed: ONE segment, which is clean whatever the model says, so its clip is always written
    base = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--batch-size', '4', '--band-states', '64', '--min-silence', '2.0',
            '--transcript', txt]
    recs = []
    for tag, extra in (('res', ['--resample', '--audio', cd_wav]), ('plain', ['--audio', conv_wav])):
        out = _run('align_long.py', base + extra + ['--output-path', str(tmp_path / (tag + '.jsonl')), '--clips-dir',
                                                    str(tmp_path / (tag + '_clips')), '--clips-manifest',
                                                    str(tmp_path / (tag + '.csv')), '--min-score-per-frame', '-1000000.0'], tmp_path)
        assert out.returncode == 0, out.stderr[-3000:]
        recs.append(json.loads((tmp_path / (tag + '.jsonl')).read_text()))
    res, plain = recs
    assert (res['path'], res['source_rate'], res['source_channels']) == (cd_wav, 44100, 1)
    assert _without(res, 'path', 'source_rate', 'source_channels') == _without(plain, 'path') and 'source_rate' not in plain
    assert res['duration'] == round(len(conv) / 16000.0, 3) and len(res['segments']) == 1 and res['score'] is not None
    assert os.listdir(str(tmp_path / 'res_clips')) and sorted(os.listdir(str(tmp_path / 'res_clips'))) == \
        [f.replace('talk16', 'talk44') for f in sorted(os.listdir(str(tmp_path / 'plain_clips')))]
    got = _read(tmp_path / 'res_clips' / 'talk44_00000.wav')                  # (16 kHz mono: _read checks the header)
    assert np.array_equal(got, _read(tmp_path / 'plain_clips' / 'talk16_00000.wav'))
    g = res['segments'][0]
    a, b = int(round(g['start'] * 100)), int(round(g['end'] * 100))
    assert np.array_equal(got, conv[160 * a:min(len(conv), 160 * b)])
    # without the flag the 44.1 kHz file is refused as before
    out = _run('align_long.py', base + ['--audio', cd_wav, '--output-path', str(tmp_path / 'no.jsonl')], tmp_path)
    assert out.returncode != 0 and 'talk44.wav' in out.stderr and '44100' in out.stderr
    assert not os.path.exists(str(tmp_path / 'no.jsonl'))


def _bank_files(root, rng, make):
    """An 8 kHz mono, a 48 kHz stereo and a 16 kHz mono file, named so that the foreign ones sort first."""
    files = [('a_8k.wav', 8000, 1), ('b_48k.wav', 48000, 2), ('c_16k.wav', 16000, 1)]
    want = []
    for name, rate, channels in files:
        pcm = make(rate, channels, rng)
        _write(os.path.join(root, name), pcm, rate, channels=channels)
        want.append(_converted(pcm, rate, channels) if (rate, channels) != (16000, 1) else pcm)
    return want


def test_noise_bank_with_resample_holds_the_converted_files(tmp_path):
    from codes.transforms import NoiseInjection
    from codes.utils.training_utils import get_noise
    rng = np.random.RandomState(3)
    want = _bank_files(str(tmp_path), rng, lambda rate, ch, r: r.randint(-9000, 9001, size=(rate // 5) * ch).astype(np.int16))
    noise = NoiseInjection(str(tmp_path), resample=True)
    assert noise.lengths == [len(w) for w in want] == [3200, 3200, 3200]
    assert np.array_equal(noise.bank('cuda').cpu().numpy(), np.concatenate(want))
    via_config = get_noise(None, {'training': {'noise': {'path': str(tmp_path), 'resample': True}}})
    assert via_config.resample and via_config.lengths == noise.lengths
    for build in (lambda: NoiseInjection(str(tmp_path)), lambda: NoiseInjection(str(tmp_path), resample=False),
                  lambda: get_noise(None, {'training': {'noise': {'path': str(tmp_path)}}})):
        with pytest.raises(ValueError, match=r'a_8k\.wav: 8000 Hz.*nothing is resampled here'):
            build()


def test_rir_bank_with_resample_holds_the_converted_files(tmp_path):
    from codes.transforms import Reverb, rir_from_pcm
    from codes.utils.training_utils import get_reverb

    def make(rate, channels, r):
        n = rate // 10
        h = r.randn(n) * np.exp(-np.arange(n) / (0.02 * rate)) * 3000
        h[rate // 200] = 20000                                                # the direct path, 5 ms in
        return np.repeat(np.rint(h).astype(np.int16), channels)
    rng = np.random.RandomState(4)
    want = [rir_from_pcm(w, 8000) for w in _bank_files(str(tmp_path), rng, make)]
    rir = Reverb(str(tmp_path), resample=True)
    assert rir.lengths == [len(w) for w in want] and all(w[0] == 1.0 for w in want)
    assert np.array_equal(rir.bank('cuda').cpu().numpy(), np.concatenate(want))
    assert get_reverb(None, {'training': {'reverb': {'path': str(tmp_path), 'resample': True}}}).lengths == rir.lengths
    for build in (lambda: Reverb(str(tmp_path)), lambda: get_reverb(None, {'training': {'reverb': {'path': str(tmp_path)}}})):
        with pytest.raises(ValueError, match=r'a_8k\.wav: 8000 Hz.*nothing is resampled here'):
            build()


def test_resample_wav_tool_writes_the_converted_files(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import resample_wav
    finally:
        sys.path.pop(0)
    rng = np.random.RandomState(9)
    src = tmp_path / 'in'
    src.mkdir()
    clips = {'a.wav': (22050, 1), 'b.wav': (32000, 3), 'c.wav': (16000, 1)}
    want = {}
    for name, (rate, channels) in clips.items():
        pcm = rng.randint(-20000, 20001, size=(rate // 4) * channels).astype(np.int16)
        _write(src / name, pcm, rate, channels=channels)
        want[name] = _converted(pcm, rate, channels)
    resample_wav.main([str(src / n) for n in clips] + ['--out-dir', str(tmp_path / 'out')])
    assert len(capsys.readouterr().out.splitlines()) == 3
    for name in clips:
        assert np.array_equal(_read(tmp_path / 'out' / name), want[name]) and len(want[name]) == 4000
    _write(src / 'odd.wav', np.zeros(10, np.int16), 44056)
    with pytest.raises(SystemExit, match=r'odd\.wav.*44056'):
        resample_wav.main([str(src / 'a.wav'), str(src / 'odd.wav'), '--out-dir', str(tmp_path / 'out2')])
    assert not os.path.exists(str(tmp_path / 'out2'))
