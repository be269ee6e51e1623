"""Noise injection without a GPU: the C ABI's new entry points, the float64 reference (tests/noise_ref.py) against the
formula written out, the start rule, NoiseInjection's host behaviour and draws, and the config wiring."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ C ABI
def test_noise_entry_points_are_declared_bound_and_exported():
    from ds2hip import lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, res, nargs in (('ds2_noise_mix_ws_bytes', 'size_t', 2), ('ds2_noise_mix', 'int', 14)):
        m = re.search(r'\n\s*%s\s+%s\s*\(([^;]*?)\)\s*;' % (res, name), code)
        assert m, name + ' is not declared in include/ds2hip.h'
        assert len(m.group(1).split(',')) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(handle, name), name + ' is not exported'
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404
    assert int(re.search(r'#define\s+DS2_NOISE_CHUNK\s+(\d+)', hdr).group(1)) == ops.NOISE_CHUNK


def test_noise_workspace_query_grows_with_batch_and_length():
    from ds2hip import lib, ops
    q = lambda b, n: lib.query('ds2_noise_mix_ws_bytes', b, n)          # noqa: E731
    ch = ops.NOISE_CHUNK
    for b in (1, 5, 65):
        for n in (1, ch - 1, ch, ch + 1, 3 * ch + 7, 240000):
            assert q(b, n) >= 16 * b * -(-n // ch), (b, n)
    assert q(1, ch) < q(1, ch + 1) < q(1, 240000) and q(1, 240000) < q(2, 240000) < q(10, 240000)
    assert q(1, 0) >= 16


def test_noise_mix_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    fn = lib.load().ds2_noise_mix
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    ok = [one, one, 1, one, one, one, one, one, 1.0, one, None, one, 16, None]
    for null_at in (0, 1, 3, 4, 5, 6, 7, 9, 11):
        args = list(ok)
        args[null_at] = None
        assert fn(*args) == lib.ERR_ARG, null_at
    for pos, bad in ((2, 0), (2, 65536), (2, -1), (8, 0.0), (8, -1.0), (12, 8), (12, 0)):
        args = list(ok)
        args[pos] = bad
        assert fn(*args) == lib.ERR_ARG, (pos, bad)
    args = list(ok)
    args[2], args[12] = 3, 32                                           # one partial per clip at the least: 3 clips need 48
    assert fn(*args) == lib.ERR_ARG


def test_noise_mix_wrapper_refuses_cpu_tensors_and_bad_draws():
    from ds2hip import ops
    wav, bank = torch.zeros(8), torch.zeros(8, dtype=torch.int16)
    with pytest.raises(RuntimeError):
        ops.noise_mix(wav, [0, 8], bank, [0], [8], [0], [0.1], 1.0)


# ------------------------------------------------------------------------------------------------ the reference
def _direct(wav, crop16, level, scale):
    nz = crop16.astype(np.float64) * float(np.float32(scale))
    w = wav.astype(np.float64)
    coef = float(np.float32(level)) * np.sqrt(np.mean(w * w)) / np.sqrt(np.mean(nz * nz))
    return w + coef * nz, coef


def test_reference_against_the_formula_written_out():
    rng = np.random.RandomState(1)
    bank = (rng.standard_normal(1000) * 2000).astype(np.int16)
    bank[300:420] = 0                                                   # a silent stretch inside the second recording
    wav = (rng.standard_normal(100) * 0.1).astype(np.float32)
    scale = 1.0 / 32768.0
    # a crop without wrap: recording bank[200:900], crop from 500 of it
    out, coef = noise_ref.mix_ref(wav, bank, 200, 700, 500, 0.25, scale)
    want, wcoef = _direct(wav, bank[700:800], 0.25, scale)
    assert coef == pytest.approx(wcoef, rel=1e-14) and np.allclose(out, want, rtol=0, atol=1e-15)
    assert coef > 0
    # a wrapped recording: 30 samples from bank[10:40], start 25 -> 25..29, 0..29, 0..29, ...
    out, coef = noise_ref.mix_ref(wav, bank, 10, 30, 25, 0.5, 65536.0)
    idx = 10 + (25 + np.arange(100)) % 30
    want, wcoef = _direct(wav, bank[idx], 0.5, 65536.0)
    assert list(idx[:7]) == [35, 36, 37, 38, 39, 10, 11]
    assert coef == pytest.approx(wcoef, rel=1e-14) and np.allclose(out, want, rtol=1e-15, atol=0)
    # a silent crop: nothing added, nothing not finite
    out, coef = noise_ref.mix_ref(wav, bank, 200, 700, 105, 0.5, scale)
    assert coef == 0.0 and np.array_equal(out, wav.astype(np.float64))
    # level 0, and no noise drawn
    out, coef = noise_ref.mix_ref(wav, bank, 0, 200, 3, 0.0, scale)
    assert coef == 0.0 and np.array_equal(out, wav.astype(np.float64))
    out, coef = noise_ref.mix_ref(wav, bank, 0, 0, 0, 0.5, scale)
    assert coef == 0.0 and np.array_equal(out, wav.astype(np.float64))
    # the scale cancels in the mixed signal's noise share: rms(out - wav) = level * rms(wav) at every scale
    for s in (scale, 65536.0):
        out, _ = noise_ref.mix_ref(wav * np.float32(s * 32768), bank, 500, 400, 7, 0.25, s)
        w = (wav * np.float32(s * 32768)).astype(np.float64)
        assert np.sqrt(np.mean((out - w) ** 2)) == pytest.approx(float(np.float32(0.25)) * np.sqrt(np.mean(w * w)), rel=1e-12)


@pytest.mark.parametrize('noise_len,n', [(1000, 300), (300, 300), (299, 300), (100, 12295), (1, 1), (5, 1), (1, 5)])
def test_start_rule_stays_inside_the_recording(noise_len, n):
    from codes.transforms import noise_start
    last_u = float(np.nextafter(np.float32(1.0), np.float32(0.0)))      # the largest value torch.rand(()) can give
    for u in (0.0, 0.25, 0.5, last_u, float(np.nextafter(1.0, 0.0))):
        s = noise_start(u, noise_len, n)
        assert s == noise_ref.start_rule(u, noise_len, n)
        assert 0 <= s < noise_len
        if noise_len >= n:
            assert s + n <= noise_len                                   # a plain crop never reads past the end
    assert noise_start(0.0, noise_len, n) == 0
    if noise_len > n:
        assert noise_start(last_u, noise_len, n) == noise_len - n - 1
        assert noise_start(0.5, noise_len, n) == (noise_len - n) // 2
    elif noise_len < n:
        assert noise_start(last_u, noise_len, n) == noise_len - 1
        assert noise_start(0.5, noise_len, n) == noise_len // 2


# ------------------------------------------------------------------------------------------------ NoiseInjection on the host
@pytest.fixture()
def noise_dir(tmp_path):
    root = str(tmp_path / 'noise')
    return root, noise_ref.write_noise_dir(root)


def test_listing_is_sorted_and_recursive(noise_dir):
    from codes.transforms import NoiseInjection
    root, files = noise_dir
    open(os.path.join(root, 'README.txt'), 'w').write('not audio')
    ni = NoiseInjection(root)
    _, starts, lengths, order = noise_ref.bank_of(root, files)
    assert ni.paths == [os.path.join(root, r) for r in order] == sorted(ni.paths) and len(ni.paths) == 3
    assert {os.path.dirname(os.path.relpath(p, root)) for p in ni.paths} == {'', 'a', 'b'}
    assert ni.lengths == lengths and ni.starts == starts
    assert ni.prob == 0.4 and ni.noise_levels == (0.0, 0.5) and ni.sample_rate == 16000
    text = repr(ni)
    assert 'NoiseInjection' in text and root in text and 'prob=0.4' in text and 'files=3' in text


def test_missing_and_empty_directories_are_refused(tmp_path):
    from codes.transforms import NoiseInjection
    with pytest.raises(IOError):
        NoiseInjection(str(tmp_path / 'nowhere'))
    os.makedirs(str(tmp_path / 'empty'))
    with pytest.raises(ValueError, match='no .wav file'):
        NoiseInjection(str(tmp_path / 'empty'))


@pytest.mark.parametrize('kind', ['8 kHz', 'stereo', 'empty', '8 bit'])
def test_files_the_bank_cannot_take_are_refused_by_name(noise_dir, kind):
    from codes.transforms import NoiseInjection
    root, _ = noise_dir
    x = np.arange(800, dtype=np.int16)
    bad = os.path.join(root, 'a', 'bad_one.wav')
    if kind == '8 kHz':
        noise_ref.write_wav(bad, x, rate=8000)
    elif kind == 'stereo':
        noise_ref.write_wav(bad, x, channels=2)
    elif kind == '8 bit':
        noise_ref.write_wav(bad, x, width=1)
    else:
        noise_ref.write_wav(bad, x[:0])
    with pytest.raises(ValueError, match='bad_one.wav'):
        NoiseInjection(root)


def test_a_set_longer_than_the_limit_is_refused_with_both_numbers(noise_dir):
    from codes.transforms import NoiseInjection
    root, files = noise_dir
    total = sum(len(v) for v in files.values()) / 16000.0               # 0.45 s
    with pytest.raises(ValueError) as e:
        NoiseInjection(root, max_bank_seconds=0.4)
    assert '0.4' in str(e.value) and ('%.1f' % total) in str(e.value)
    NoiseInjection(root, max_bank_seconds=total)                        # exactly at the limit is allowed


# ------------------------------------------------------------------------------------------------ draws
def test_prob_zero_never_draws_and_costs_one_binomial(noise_dir):
    from codes.transforms import NoiseInjection
    ni = NoiseInjection(noise_dir[0], prob=0.0)
    np.random.seed(11)
    torch.manual_seed(11)
    assert all(ni.draw() is None for _ in range(50))
    after, t_after = np.random.uniform(), float(torch.rand(()))
    np.random.seed(11)
    torch.manual_seed(11)
    for _ in range(50):
        np.random.binomial(1, 0.0)
    assert after == np.random.uniform() and t_after == float(torch.rand(()))
    # a miss at a probability strictly between 0 and 1 costs the one binomial variate and nothing else
    ni = NoiseInjection(noise_dir[0], prob=0.5)
    np.random.seed(12)
    got = [ni.draw() for _ in range(40)]
    after = np.random.uniform()
    np.random.seed(12)
    for d in got:
        hit = np.random.binomial(1, 0.5)
        assert bool(hit) == (d is not None)
        if hit:
            np.random.choice(3)
            np.random.uniform(0, 0.5)
    assert after == np.random.uniform() and any(d is None for d in got) and any(d is not None for d in got)


def test_prob_one_always_draws_in_range_and_in_the_documented_order(noise_dir):
    from codes.transforms import NoiseInjection
    ni = NoiseInjection(noise_dir[0], noise_levels=(0.1, 0.3), prob=1.0)
    np.random.seed(5)
    torch.manual_seed(5)
    draws = [ni.draw() for _ in range(60)]
    assert all(d is not None for d in draws)
    assert {d[0] for d in draws} == {0, 1, 2}
    assert all(0.1 <= d[1] < 0.3 and 0.0 <= d[2] < 1.0 for d in draws)
    assert all(isinstance(d[0], int) and isinstance(d[1], float) and isinstance(d[2], float) for d in draws)
    np.random.seed(5)
    torch.manual_seed(5)
    for d in draws[:10]:                       # binomial, choice, uniform from np.random, then torch.rand
        assert np.random.binomial(1, 1.0) == 1
        assert d == (int(np.random.choice(3)), float(np.random.uniform(0.1, 0.3)), float(torch.rand(())))
    np.random.seed(5)
    torch.manual_seed(5)
    assert [ni.draw() for _ in range(60)] == draws                      # reproducible under a seed
    rng = np.random.RandomState(3)                                      # an explicit generator leaves the global streams alone
    np.random.seed(6)
    first = ni.draw(rng)
    assert first is not None and np.random.uniform() == np.random.RandomState(6).uniform()
    assert ni.draw(np.random.RandomState(3)) == first


def _write_clip(path, n, seed):
    x = (np.random.RandomState(seed).standard_normal(n) * 3000).astype(np.int16)
    return noise_ref.write_wav(path, x), x


def test_totensor_without_noise_keeps_its_random_stream(tmp_path, noise_dir):
    """Tempo and gain of the first five clips under a seed are np.random.uniform's own values, tempo first -- with no noise
    configured nothing else is drawn; with noise, the draw comes behind them."""
    from codes.transforms import NoiseInjection, PCMClip, ToTensor
    path, x = _write_clip(str(tmp_path / 'clip.wav'), 2000, 0)
    tt = ToTensor(augment=True, defer=True)
    assert tt.noise is None
    np.random.seed(21)
    clips = [tt(path) for _ in range(5)]
    np.random.seed(21)
    for c in clips:
        assert isinstance(c, PCMClip) and c.noise is None and np.array_equal(c.pcm.numpy(), x)
        assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
        assert c.gain_db == float(np.random.uniform(low=-6, high=8))
    ni = NoiseInjection(noise_dir[0], prob=1.0)
    tn = ToTensor(augment=True, defer=True, noise=ni)
    np.random.seed(21)
    torch.manual_seed(21)
    c = tn(path)
    np.random.seed(21)
    torch.manual_seed(21)
    assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
    assert c.gain_db == float(np.random.uniform(low=-6, high=8))
    assert c.noise == ni.draw() and c.noise is not None
    # noise without tempo / gain augmentation: the two are independent
    c = ToTensor(augment=False, defer=True, noise=ni)(path)
    assert c.tempo is None and c.gain_db is None and c.noise is not None


def test_batch_carries_the_draws_or_none(noise_dir):
    from codes.transforms import NoiseInjection, PCMClip, RawAudioBatch
    pcm = lambda n: torch.arange(n, dtype=torch.int16)                  # noqa: E731
    plain = RawAudioBatch.from_clips([PCMClip(pcm(5)), PCMClip(pcm(3), tempo=1.1, gain_db=2.0)])
    assert plain.noise is None and plain.tempos == [1.0, 1.1]
    draws = [None, (2, 0.25, 0.5), None]
    batch = RawAudioBatch.from_clips([PCMClip(pcm(5), noise=d) for d in draws])
    assert batch.noise == draws and batch.tempos is None and batch.offsets == [0, 5, 10, 15]
    assert batch.to('cpu').noise == draws
    ni = NoiseInjection(noise_dir[0])
    lo, ln, st, lv = ni.params(draws, [5, 5, 5])
    assert ln == [0, ni.lengths[2], 0] and lo[1] == ni.starts[2] and lv == [0.0, 0.25, 0.0]
    assert st[1] == noise_ref.start_rule(0.5, ni.lengths[2], 5)


def test_frontend_without_a_bank_refuses_a_batch_with_draws():
    """(refused before anything touches the device: no GPU needed)"""
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch
    front = BatchSpectrogram()
    assert front.noise is None
    batch = RawAudioBatch.from_clips([PCMClip(torch.zeros(400, dtype=torch.int16), noise=(0, 0.25, 0.5))])
    with pytest.raises(RuntimeError, match='noise bank'):
        front(batch)


# ------------------------------------------------------------------------------------------------ config
def _config(noise=None, **training):
    from codes.utils.io_utils import AttrDict
    if noise is not None:
        training['noise'] = AttrDict(noise)
    return AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})


def test_default_transforms_with_and_without_the_block(tmp_path, noise_dir, monkeypatch):
    import shutil

    from codes import transforms as T
    from codes.utils import training_utils as tu
    data = str(tmp_path / 'data')
    os.makedirs(data)
    for f in ('labels.en.json',):
        shutil.copy(os.path.join(ROOT, 'data', f), data)
    shutil.copytree(noise_dir[0], os.path.join(data, 'bg'))
    monkeypatch.chdir(str(tmp_path))                                    # 'bg' does not exist from here: only under data
    # without the block: exactly today's transforms
    train_t, val_t, _ = tu.get_default_transforms(data, _config(augment=True))
    assert T.waveform_noise(train_t) is None and T.waveform_noise(val_t) is None
    assert [type(t) for t in train_t.transforms] == [T.ToTensor] and train_t.transforms[0].augment
    # with it: the training loader draws, validation never does; relative path under the data directory
    cfg = _config(noise={'path': 'bg', 'noise_levels': [0.1, 0.2], 'prob': 0.7}, audio_scale='int32')
    train_t, val_t, _ = tu.get_default_transforms(data, cfg)
    ni = T.waveform_noise(train_t)
    assert isinstance(ni, T.NoiseInjection) and T.waveform_noise(val_t) is None
    assert ni.path == os.path.join(data, 'bg') and len(ni.paths) == 3
    assert ni.prob == 0.7 and ni.noise_levels == (0.1, 0.2) and ni.scale == 65536.0
    assert not train_t.transforms[0].augment and train_t.transforms[0].defer       # independent of training.augment
    assert all(t.noise is None for t in val_t.transforms if isinstance(t, T.ToTensor))
    # evaluation does not even look at the block (the directory may be gone by then)
    gone = _config(noise={'path': 'no_such_dir'})
    with pytest.raises(IOError):
        tu.get_default_transforms(data, gone)
    train_t, val_t, _ = tu.get_default_transforms(data, gone, noise=False)
    assert T.waveform_noise(train_t) is None
    # the reference's per-utterance contract: the transform stands between the loader and the spectrogram
    train_t, val_t, _ = tu.get_default_transforms(data, cfg, gpu_frontend=False)
    assert [type(t) for t in train_t.transforms] == [T.ToTensor, T.NoiseInjection, T.ToSpectrogram]
    assert [type(t) for t in val_t.transforms] == [T.ToTensor, T.ToSpectrogram]
    assert train_t.transforms[0].noise is None
    with pytest.raises(ValueError, match='training.noise'):
        tu.get_default_transforms(data, _config(noise={'path': 'bg', 'level': 3}))
