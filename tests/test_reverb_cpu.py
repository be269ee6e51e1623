"""Reverberation without a GPU: the C ABI's new entry points and refusals, the float64 reference (tests/reverb_ref.py) against
itself, the bank rule on hand-made files, Reverb's host behaviour and draws, the config wiring and tools/make_rir.py."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import reverb_ref as ref
from tests.noise_ref import write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make_rir():
    spec = importlib.util.spec_from_file_location('ds2_make_rir', os.path.join(ROOT, 'tools', 'make_rir.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ C ABI
def test_reverb_entry_points_are_declared_bound_and_exported():
    from ds2hip import lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, res, nargs in (('ds2_reverb_ws_bytes', 'size_t', 2), ('ds2_reverb', 'int', 12)):
        m = re.search(r'\n\s*%s\s+%s\s*\(([^;]*?)\)\s*;' % (res, name), code)
        assert m, name + ' is not declared in include/ds2hip.h'
        assert len(m.group(1).split(',')) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(handle, name), name + ' is not exported'
    const = lambda n: int(re.search(r'#define\s+%s\s+(\d+)' % n, hdr).group(1))      # noqa: E731
    assert const('DS2_REVERB_TILE') == ops.REVERB_TILE and ops.REVERB_TILE % 256 == 0
    assert const('DS2_REVERB_TAPS_STEP') == ops.REVERB_TAPS_STEP and ops.REVERB_TAPS_STEP % 4 == 0
    assert const('DS2_REVERB_MAX_TAPS') == ops.REVERB_MAX_TAPS >= 16000
    assert 'reverberation' in hdr


def test_reverb_workspace_query_grows_with_batch_and_length():
    from ds2hip import lib, ops
    q = lambda b, n: lib.query('ds2_reverb_ws_bytes', b, n)             # noqa: E731
    t = ops.REVERB_TILE
    for b in (1, 5, 65):
        for n in (1, t - 1, t, t + 1, 3 * t + 7, 240000):
            assert q(b, n) >= 16 * b * -(-n // t), (b, n)
    assert q(1, t) < q(1, t + 1) < q(1, 240000) < q(2, 240000) < q(10, 240000)
    assert q(1, 0) >= 16


def test_reverb_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    handle = lib.load()
    fn = handle.ds2_reverb
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)               # never dereferenced: the call is refused first
    ok = [one, one, 1, one, one, one, 1, two, None, one, 16, None]
    for null_at in (0, 1, 3, 4, 5, 7, 9):
        args = list(ok)
        args[null_at] = None
        assert fn(*args) == lib.ERR_ARG, null_at
        assert b'ds2_reverb' in handle.ds2_last_error()
    for pos, bad in ((2, 0), (2, 65536), (2, -1), (6, 2), (6, -1), (10, 8), (10, 0)):
        args = list(ok)
        args[pos] = bad
        assert fn(*args) == lib.ERR_ARG, (pos, bad)
        assert b'ds2_reverb' in handle.ds2_last_error()
    args = list(ok)
    args[7] = one                                                       # out == wav: the convolution is out of place
    assert fn(*args) == lib.ERR_ARG and b'out != wav' in handle.ds2_last_error()
    args = list(ok)
    args[2], args[10] = 3, 32                                           # one pair per clip at the least: 3 clips need 48
    assert fn(*args) == lib.ERR_ARG


def test_reverb_wrapper_refuses_cpu_tensors():
    from ds2hip import ops
    with pytest.raises(RuntimeError, match='on the device'):
        ops.reverb(torch.zeros(8), [0, 8], torch.ones(4), [0], [4])


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('n,k', [(1, 1), (17, 40), (1000, 1), (4103, 515), (6000, 8000), (20000, 8000)])
def test_fft_and_direct_references_agree(n, k):
    rng = np.random.RandomState(n + k)
    x = (rng.standard_normal(n) * 0.2).astype(np.float32)
    h = ref.synth_rir_taps(k, 0.4, k)
    a, b, s = ref.conv_direct(x, h), ref.conv_fft(x, h), ref.abs_sum(x, h)
    assert a.shape == b.shape == (n,)
    worst = float(np.max(np.abs(a - b) / np.maximum(s, 1e-300)))
    print('fft vs direct at N=%d K=%d: %.2e of S' % (n, k, worst))
    assert np.all(np.abs(a - b) <= 1e-10 * s + 1e-300)
    # the sum written out, at a few places
    for i in sorted({0, n // 2, n - 1}):
        want = sum(float(h[j]) * float(x[i - j]) for j in range(min(i, k - 1) + 1))
        assert abs(a[i] - want) <= 1e-12 * max(s[i], 1e-300)
    assert ref.conv_ref(x, h).shape == (n,)


def test_chain_yardstick_and_gain_reference():
    x = np.array([1, 2, 3, 4], np.float32)
    h = np.array([1, 0.5, 0.25], np.float32)
    assert ref.chain32(x, h).tolist() == [1.0, 2.5, 4.25, 6.0] == ref.conv_direct(x, h).tolist()
    assert ref.gain_ref(x, ref.chain32(x, h)) == pytest.approx(np.sqrt(30.0 / (1 + 6.25 + 4.25 ** 2 + 36)), rel=1e-15)
    assert ref.gain_ref(np.zeros(4, np.float32), np.zeros(4, np.float32)) == 1.0
    assert ref.gain_ref(np.full(4, 3e38, np.float32), np.full(4, 1e-45, np.float32)) == 1.0      # not finite as a float


# ------------------------------------------------------------------------------------------------ the bank rule
def _i16(values):
    return np.asarray(values, np.int16)


def test_bank_rule_on_hand_made_files(tmp_path):
    from codes.transforms import Reverb, rir_from_pcm
    files = {
        'b/neg.wav': _i16([100, -16384, 8192, 0, -4096, 0, 0]),            # a negative peak, trailing zeros
        'a/mid.wav': _i16([0, 0, 50, -60, 20000, 10000, -5000, 2500, 1]),  # a peak in the middle
        'tie.wav': _i16([3, -3000, 3000, 1500]),                           # |peak| twice: the FIRST one
        'zlong.wav': _i16([32767] + [1000] * 40),                          # truncated at max_taps
    }
    root = ref.write_rir_dir(str(tmp_path / 'rirs'), files)
    open(os.path.join(root, 'README.txt'), 'w').write('not audio')
    rv = Reverb(root, max_rir_seconds=16 / 16000.0)
    order = sorted(files, key=lambda rel: os.path.join(root, rel))
    assert rv.paths == [os.path.join(root, r) for r in order] and rv.max_taps == 16
    want = {'b/neg.wav': [1.0, -0.5, 0.0, 0.25], 'a/mid.wav': [1.0, 0.5, -0.25, 0.125, 1 / 20000.0],
            'tie.wav': [1.0, -1.0, -0.5], 'zlong.wav': [1.0] + [1000 / 32767.0] * 15}
    for rel, n in zip(order, rv.lengths):
        got = rir_from_pcm(files[rel], 16)
        assert got.dtype == np.float32 and got[0] == 1.0 and got.size == n == len(want[rel])
        assert np.array_equal(got, np.asarray(want[rel], np.float64).astype(np.float32))
        assert np.array_equal(got, ref.rir_rule(files[rel], 16))
    assert rv.starts == [0] + list(np.cumsum(rv.lengths[:-1]))
    assert rv.prob == 0.3 and rv.max_rir_seconds == 16 / 16000.0 and rv.max_bank_seconds == 600
    text = repr(rv)
    assert 'Reverb' in text and root in text and 'prob=0.3' in text and 'files=4' in text
    # the bank-size refusal: not truncated, both numbers named; exactly at the limit is allowed
    total = sum(rv.lengths)
    with pytest.raises(ValueError, match='max_bank_seconds'):
        Reverb(root, max_rir_seconds=16 / 16000.0, max_bank_seconds=(total - 1) / 16000.0)
    Reverb(root, max_rir_seconds=16 / 16000.0, max_bank_seconds=total / 16000.0)


@pytest.mark.parametrize('kind', ['8 kHz', 'stereo', '8 bit', 'empty', 'silent'])
def test_files_the_bank_cannot_take_are_refused_by_name(tmp_path, kind):
    from codes.transforms import Reverb
    root = ref.write_rir_dir(str(tmp_path / 'rirs'), {'ok.wav': _i16([20000, 5000, -300])})
    Reverb(root)
    x = _i16([20000, 100, -100, 50])
    bad = os.path.join(root, 'sub', 'bad_one.wav')
    if kind == '8 kHz':
        write_wav(bad, x, rate=8000)
    elif kind == 'stereo':
        write_wav(bad, x, channels=2)
    elif kind == '8 bit':
        write_wav(bad, x, width=1)
    elif kind == 'empty':
        write_wav(bad, x[:0])
    else:
        write_wav(bad, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match='bad_one.wav'):
        Reverb(root)


def test_missing_and_empty_directories_and_bad_limits_are_refused(tmp_path):
    from codes.transforms import Reverb
    from ds2hip import ops
    with pytest.raises(IOError):
        Reverb(str(tmp_path / 'nowhere'))
    os.makedirs(str(tmp_path / 'empty'))
    with pytest.raises(ValueError, match='no .wav file'):
        Reverb(str(tmp_path / 'empty'))
    root = ref.write_rir_dir(str(tmp_path / 'rirs'), {'ok.wav': _i16([20000, 5000, -300])})
    with pytest.raises(ValueError, match='16000'):
        Reverb(root, sample_rate=8000)
    with pytest.raises(ValueError, match='max_rir_seconds'):
        Reverb(root, max_rir_seconds=(ops.REVERB_MAX_TAPS + 1) / 16000.0)
    with pytest.raises(ValueError, match='max_rir_seconds'):
        Reverb(root, max_rir_seconds=0)


def test_make_rir_files_pass_the_bank_rule(tmp_path):
    from codes.transforms import Reverb
    mk = _make_rir()
    root = str(tmp_path / 'set')
    paths = mk.write_set(root, rt60s=(0.1, 0.3), count=2, seed=3)
    assert len(paths) == 4 and sorted(paths) == paths
    rv = Reverb(root)
    assert rv.paths == paths and all(1 < n <= 8000 for n in rv.lengths)
    assert rv.lengths[0] < rv.lengths[2]                                # RT60 0.1 s is shorter than 0.3 s (1.5 RT60 each)
    for p in paths:
        h = rv._taps(p)
        assert h[0] == 1.0 and np.all(np.abs(h[1:]) < 1.0) and h[-1] != 0
        tail = h[1:].astype(np.float64)
        assert 0.05 < np.sum(tail * tail) < 1.5                         # direct-to-reverberant ratio 0..10 dB, roughly
    again = str(tmp_path / 'again')
    mk.write_set(again, rt60s=(0.1, 0.3), count=2, seed=3)
    assert all(open(a, 'rb').read() == open(os.path.join(again, os.path.basename(a)), 'rb').read() for a in paths)
    assert mk.main([str(tmp_path / 'cli'), '--rt60', '0.05', '--count', '1']) == 0
    assert Reverb(str(tmp_path / 'cli')).lengths[0] <= int(0.05 * 1.5 * 16000)


# ------------------------------------------------------------------------------------------------ draws
@pytest.fixture()
def rir_dir(tmp_path):
    return ref.write_rir_dir(str(tmp_path / 'rirs'), {'a.wav': _i16([20000, 5000]), 'b.wav': _i16([-20000, 100, 7]),
                                                     'c/c.wav': _i16([1, 30000, -200, 10, 3])})


def test_draw_order_binomial_first_choice_only_on_a_hit(rir_dir):
    from codes.transforms import Reverb
    rv = Reverb(rir_dir, prob=0.5)
    np.random.seed(12)
    got = [rv.draw() for _ in range(60)]
    after = np.random.uniform()
    np.random.seed(12)
    for d in got:
        hit = np.random.binomial(1, 0.5)
        assert bool(hit) == (d is not None)
        if hit:
            assert d == int(np.random.choice(3)) and isinstance(d, int)
    assert after == np.random.uniform() and any(d is None for d in got) and {d for d in got if d is not None} == {0, 1, 2}
    rv0 = Reverb(rir_dir, prob=0.0)
    np.random.seed(3)
    assert all(rv0.draw() is None for _ in range(20))
    after = np.random.uniform()
    np.random.seed(3)
    for _ in range(20):
        np.random.binomial(1, 0.0)
    assert after == np.random.uniform()
    rng = np.random.RandomState(3)                                      # an explicit generator leaves the global stream alone
    rv1 = Reverb(rir_dir, prob=1.0)
    np.random.seed(6)
    first = rv1.draw(rng)
    assert first is not None and np.random.uniform() == np.random.RandomState(6).uniform()
    assert rv1.draw(np.random.RandomState(3)) == first
    assert rv1.params([None, 2, 0]) == ([0, rv1.starts[2], 0], [0, rv1.lengths[2], rv1.lengths[0]])


def test_totensor_draws_between_gain_and_noise_and_nothing_without_it(tmp_path, rir_dir):
    from codes.transforms import NoiseInjection, PCMClip, Reverb, ToTensor
    from tests.noise_ref import write_noise_dir
    x = (np.random.RandomState(0).standard_normal(2000) * 3000).astype(np.int16)
    path = write_wav(str(tmp_path / 'clip.wav'), x)
    tt = ToTensor(augment=True, defer=True)
    assert tt.reverb is None
    np.random.seed(21)
    clips = [tt(path) for _ in range(5)]
    np.random.seed(21)
    for c in clips:                                                     # exactly what it drew before the feature existed
        assert isinstance(c, PCMClip) and c.reverb is None and c.noise is None
        assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
        assert c.gain_db == float(np.random.uniform(low=-6, high=8))
    write_noise_dir(str(tmp_path / 'noise'))
    ni, rv = NoiseInjection(str(tmp_path / 'noise'), prob=1.0), Reverb(rir_dir, prob=1.0)
    tr = ToTensor(augment=True, defer=True, noise=ni, reverb=rv)
    np.random.seed(21)
    torch.manual_seed(21)
    c = tr(path)
    np.random.seed(21)
    torch.manual_seed(21)
    assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
    assert c.gain_db == float(np.random.uniform(low=-6, high=8))
    assert c.reverb == rv.draw() and c.reverb is not None               # behind the gain ...
    assert c.noise == ni.draw() and c.noise is not None                 # ... and in front of the noise
    c = ToTensor(augment=False, defer=True, reverb=rv)(path)
    assert c.tempo is None and c.gain_db is None and c.noise is None and c.reverb is not None


def test_batch_carries_the_draws_or_none():
    from codes.transforms import PCMClip, RawAudioBatch
    pcm = lambda n: torch.arange(n, dtype=torch.int16)                  # noqa: E731
    plain = RawAudioBatch.from_clips([PCMClip(pcm(5)), PCMClip(pcm(3), tempo=1.1, gain_db=2.0)])
    assert plain.reverb is None and plain.noise is None and plain.spec is None
    draws = [None, 2, None]
    batch = RawAudioBatch.from_clips([PCMClip(pcm(5), reverb=d) for d in draws])
    assert batch.reverb == draws and batch.noise is None and batch.offsets == [0, 5, 10, 15]
    assert batch.to('cpu').reverb == draws and batch.pin_memory.__self__ is batch
    assert RawAudioBatch(batch.pcm, batch.offsets).reverb is None
    zero = RawAudioBatch.from_clips([PCMClip(pcm(5), reverb=0)])        # file index 0 is a draw, not "none"
    assert zero.reverb == [0]


def test_frontend_without_a_bank_refuses_a_batch_with_draws():
    """(refused before anything touches the device: no GPU needed)"""
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch
    front = BatchSpectrogram()
    assert front.reverb is None
    batch = RawAudioBatch.from_clips([PCMClip(torch.zeros(400, dtype=torch.int16), reverb=0)])
    with pytest.raises(RuntimeError, match='RIR bank'):
        front(batch)


def test_pickling_drops_the_bank(rir_dir):
    from codes.transforms import Reverb
    rv = Reverb(rir_dir, prob=0.25)
    rv._banks['stand-in'] = torch.ones(3)
    back = pickle.loads(pickle.dumps(rv))
    assert back._banks == {} and back._lock is not None and rv._banks
    assert (back.paths, back.lengths, back.starts, back.prob, back.max_taps) == \
        (rv.paths, rv.lengths, rv.starts, 0.25, rv.max_taps)
    assert back.draw(np.random.RandomState(1)) == rv.draw(np.random.RandomState(1))


# ------------------------------------------------------------------------------------------------ config
def _config(reverb=None, **training):
    from codes.utils.io_utils import AttrDict
    if reverb is not None:
        training['reverb'] = AttrDict(reverb)
    return AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})


def test_default_transforms_with_and_without_the_block(tmp_path, rir_dir, monkeypatch):
    import shutil

    from codes import transforms as T
    from codes.utils import training_utils as tu
    from tests.noise_ref import write_noise_dir
    data = str(tmp_path / 'data')
    os.makedirs(data)
    shutil.copy(os.path.join(ROOT, 'data', 'labels.en.json'), data)
    shutil.copytree(rir_dir, os.path.join(data, 'rooms'))
    write_noise_dir(os.path.join(data, 'bg'))
    monkeypatch.chdir(str(tmp_path))                                    # 'rooms' does not exist from here: only under data
    train_t, val_t, _ = tu.get_default_transforms(data, _config(augment=True))
    assert T.waveform_reverb(train_t) is None and T.waveform_reverb(val_t) is None
    assert [type(t) for t in train_t.transforms] == [T.ToTensor]
    assert tu.get_reverb(data, _config()) is None
    cfg = _config(reverb={'path': 'rooms', 'prob': 0.7, 'max_rir_seconds': 0.25, 'max_bank_seconds': 5})
    train_t, val_t, _ = tu.get_default_transforms(data, cfg)
    rv = T.waveform_reverb(train_t)
    assert isinstance(rv, T.Reverb) and T.waveform_reverb(val_t) is None
    assert rv.path == os.path.join(data, 'rooms') and len(rv.paths) == 3
    assert (rv.prob, rv.max_rir_seconds, rv.max_bank_seconds, rv.max_taps) == (0.7, 0.25, 5, 4000)
    assert not train_t.transforms[0].augment and train_t.transforms[0].defer          # independent of training.augment
    assert T.waveform_noise(train_t) is None and T.waveform_spec_augment(train_t) is None
    # evaluation does not even look at the block
    gone = _config(reverb={'path': 'no_such_dir'})
    with pytest.raises(IOError):
        tu.get_default_transforms(data, gone)
    train_t, _, _ = tu.get_default_transforms(data, gone, noise=False)
    assert T.waveform_reverb(train_t) is None
    # the per-clip form: Reverb stands before NoiseInjection
    both = _config(reverb={'path': 'rooms'}, noise=None)
    both.training['noise'] = {'path': 'bg'}
    train_t, val_t, _ = tu.get_default_transforms(data, both, gpu_frontend=False)
    assert [type(t) for t in train_t.transforms] == [T.ToTensor, T.Reverb, T.NoiseInjection, T.ToSpectrogram]
    assert [type(t) for t in val_t.transforms] == [T.ToTensor, T.ToSpectrogram]
    assert train_t.transforms[0].reverb is None
    train_t, _, _ = tu.get_default_transforms(data, both)
    assert T.waveform_reverb(train_t) is not None and T.waveform_noise(train_t) is not None
    with pytest.raises(ValueError, match='rt60'):
        tu.get_default_transforms(data, _config(reverb={'path': 'rooms', 'rt60': 3}))
    with pytest.raises(ValueError, match='path'):
        tu.get_default_transforms(data, _config(reverb={'prob': 0.5}))
