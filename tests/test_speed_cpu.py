"""Speed perturbation, the parts that need no GPU: the table of a factor against the existing design, the quality of the
0.9 and 1.1 tables on the float64 reference (printed before it is asserted), the draw rule and its place in front of the tempo
draw, the carriers' positional arguments, pickling, the config block and the C ABI's declaration and refusals."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as ref
from tests import reverb_ref
from tests.noise_ref import write_noise_dir, write_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMK = {0.9: (10, 9, 53), 1.1: (10, 11, 57), 1.0: (1, 1, 1), 0.937: (1000, 937, 53), 2.0: (1, 2, 103)}


# ------------------------------------------------------------------------------------------------ design
@pytest.mark.parametrize('factor', sorted(LMK))
def test_speed_design_is_the_resample_design_of_16000_f(factor):
    from ds2hip import ops
    L, M, taps = ops.speed_design(factor)
    want = ops.resample_design(16 * int(round(1000 * factor)))
    assert (L, M) == want[:2] and taps is want[2]                                   # the same cached table: no new constants
    assert (L, M, taps.shape[1]) == LMK[factor] and taps.shape[0] == L and taps.dtype == np.float32
    rL, rM, rtaps = ref.design(16 * int(round(1000 * factor)))
    assert (L, M) == (rL, rM) and np.array_equal(taps.view(np.uint32), rtaps.view(np.uint32))
    assert L <= 1000 and M * 1000 == int(round(1000 * factor)) * L                  # M / L = factor, reduced
    if factor == 1.0:
        assert taps.tolist() == [[1.0]]
    if factor == 0.937:
        assert L * taps.shape[1] == 53000                                           # larger than the LDS table: the cache path


def test_speed_design_takes_three_decimals_and_refuses_by_value():
    from ds2hip import ops
    assert ops.speed_design(0.90004)[2] is ops.speed_design(0.9)[2]
    assert ops.speed_design(1.0996)[:2] == (10, 11) and ops.speed_design(0.5)[:2] == (2, 1)
    assert ops.speed_factor(0.93651) == 0.937 and ops.speed_factor(1) == 1.0
    for bad, text in ((0.4999, '0.4999'), (2.001, '2.001'), (float('nan'), 'nan'), (True, 'True'), (False, 'False')):
        with pytest.raises(ValueError, match=text):
            ops.speed_design(bad)
    with pytest.raises(ValueError, match="'1.1'"):
        ops.speed_design('1.1')


def _db(v):
    return 20 * np.log10(max(float(v), 1e-300))


@pytest.mark.parametrize('factor', [0.9, 1.1])
def test_a_1_khz_sine_comes_out_at_1000_f_hz(factor):
    """On tests/resample_ref.py in float64: sin(2 pi 1000 j / 16000) through the designed table is sin(2 pi 1000 f m / 16000),
    away from the first and last 400 outputs, within tests/test_resample_cpu.py's own -85 dB (the same design function)."""
    from ds2hip import ops
    L, M, taps = ops.speed_design(factor)
    n = 1700 * M // L + 1
    j = np.arange(n, dtype=np.float64)
    m = np.arange(ref.out_len(n, L, M), dtype=np.float64)
    assert len(m) >= 1600
    y = ref.convolve(np.sin(2 * np.pi * 1000.0 * j / 16000.0), L, M, taps)
    err = np.abs(y - np.sin(2 * np.pi * 1000.0 * factor * m / 16000.0))[400:-400].max()
    print('speed %.1f: 1 kHz -> %.0f Hz: error %.1f dB' % (factor, 1000 * factor, _db(err)))
    assert _db(err) < -85.0


# ------------------------------------------------------------------------------------------------ SpeedPerturb
def test_constructor_defaults_tables_and_refusals():
    from codes.transforms import SpeedPerturb
    sp = SpeedPerturb()
    assert sp.factors == (0.9, 1.0, 1.1) and sp.prob == 1.0
    assert [t[:2] for t in sp.tables()] == [(1, 1), (10, 9), (10, 11)]                # the identity first
    assert sp.table_ids([None, 0, 1, 2]) == [0, 1, 0, 2]                              # factor 1.0 IS the identity
    assert sp.out_len(16000, None) == 16000 and sp.out_len(16000, 0) == 17778 and sp.out_len(16000, 2) == 14546
    assert 'SpeedPerturb' in repr(sp) and '0.9' in repr(sp) and 'prob=1.0' in repr(sp)
    dup = SpeedPerturb(factors=[1.1, 0.9, 1.1, 0.90004])                              # repeated factors weigh the draw
    assert dup.factors == (1.1, 0.9, 1.1, 0.9) and dup.table_ids([0, 1, 2, 3]) == [1, 2, 1, 2] and len(dup.tables()) == 3
    SpeedPerturb(factors=[0.8 + 0.01 * i for i in range(15)])                         # 15 distinct: the limit
    with pytest.raises(ValueError, match='factors is empty'):
        SpeedPerturb(factors=[])
    with pytest.raises(ValueError, match='16 distinct'):
        SpeedPerturb(factors=[0.8 + 0.01 * i for i in range(16)])
    with pytest.raises(ValueError, match=r'factors.*2\.5'):
        SpeedPerturb(factors=[0.9, 2.5])
    with pytest.raises(ValueError, match=r'factors.*0\.3'):
        SpeedPerturb(factors=[0.3])
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='prob'):
            SpeedPerturb(prob=bad)


def test_draw_order_binomial_first_choice_only_on_a_hit():
    from codes.transforms import SpeedPerturb
    sp = SpeedPerturb(prob=0.5)
    np.random.seed(12)
    got = [sp.draw() for _ in range(60)]
    after = np.random.uniform()
    np.random.seed(12)
    for d in got:
        hit = np.random.binomial(1, 0.5)
        assert bool(hit) == (d is not None)
        if hit:
            assert d == int(np.random.choice(3)) and isinstance(d, int)
    assert after == np.random.uniform() and any(d is None for d in got) and {d for d in got if d is not None} == {0, 1, 2}
    sp0 = SpeedPerturb(prob=0.0)
    np.random.seed(3)
    assert all(sp0.draw() is None for _ in range(20))
    after = np.random.uniform()
    np.random.seed(3)
    for _ in range(20):
        np.random.binomial(1, 0.0)
    assert after == np.random.uniform()
    np.random.seed(6)                                                   # an explicit generator leaves the global stream alone
    first = SpeedPerturb().draw(np.random.RandomState(3))
    assert first is not None and np.random.uniform() == np.random.RandomState(6).uniform()


@pytest.fixture()
def banks(tmp_path):
    i16 = lambda v: np.asarray(v, np.int16)                             # noqa: E731
    rirs = reverb_ref.write_rir_dir(str(tmp_path / 'rirs'), {'a.wav': i16([20000, 5000]), 'b.wav': i16([-20000, 100, 7]),
                                                             'c/c.wav': i16([1, 30000, -200, 10, 3])})
    write_noise_dir(str(tmp_path / 'noise'))
    x = (np.random.RandomState(0).standard_normal(2000) * 3000).astype(np.int16)
    return rirs, str(tmp_path / 'noise'), write_wav(str(tmp_path / 'clip.wav'), x), x


def _expected(n_rir, n_noise, levels, speed_n=None):
    """One clip's draws written out from the stated rule: [speed: binomial, choice;] tempo; gain; reverb: binomial, choice;
    noise: binomial, choice, uniform, torch.rand.  Every prob is 1."""
    out = {}
    if speed_n is not None:
        assert np.random.binomial(1, 1.0) == 1
        out['speed'] = int(np.random.choice(speed_n))
    out['tempo'] = float(np.random.uniform(low=0.85, high=1.15))
    out['gain'] = float(np.random.uniform(low=-6, high=8))
    assert np.random.binomial(1, 1.0) == 1
    out['reverb'] = int(np.random.choice(n_rir))
    assert np.random.binomial(1, 1.0) == 1
    out['noise'] = (int(np.random.choice(n_noise)), float(np.random.uniform(*levels)), float(torch.rand(())))
    return out


def test_totensor_draws_speed_first_and_nothing_without_it(banks):
    from codes.transforms import NoiseInjection, PCMClip, Reverb, SpeedPerturb, ToTensor
    rirs, noise_dir, path, x = banks
    ni, rv = NoiseInjection(noise_dir, prob=1.0), Reverb(rirs, prob=1.0)
    tt = ToTensor(augment=True, defer=True, reverb=rv, noise=ni)
    assert tt.speed is None
    np.random.seed(21)
    torch.manual_seed(21)
    clips = [tt(path) for _ in range(5)]
    np.random.seed(21)
    torch.manual_seed(21)
    for c in clips:                                                     # exactly what it drew before the feature existed
        want = _expected(len(rv.paths), len(ni.paths), ni.noise_levels)
        assert isinstance(c, PCMClip) and c.speed is None and np.array_equal(c.pcm.numpy(), x)
        assert (c.tempo, c.gain_db, c.reverb, c.noise) == (want['tempo'], want['gain'], want['reverb'], want['noise'])
    sp = SpeedPerturb(prob=1.0)
    ts = ToTensor(augment=True, defer=True, reverb=rv, noise=ni, speed=sp)
    np.random.seed(21)
    torch.manual_seed(21)
    clips = [ts(path) for _ in range(5)]
    np.random.seed(21)
    torch.manual_seed(21)
    for c in clips:                                                     # the speed draw precedes them
        want = _expected(len(rv.paths), len(ni.paths), ni.noise_levels, speed_n=3)
        assert (c.speed, c.tempo, c.gain_db, c.reverb, c.noise) == \
            (want['speed'], want['tempo'], want['gain'], want['reverb'], want['noise'])
        assert np.array_equal(c.pcm.numpy(), x)                         # the worker only draws
    c = ToTensor(augment=False, defer=True, speed=sp)(path)
    assert c.tempo is None and c.gain_db is None and c.noise is None and c.reverb is None and c.speed in (0, 1, 2)
    c = ToTensor(augment=True, defer=True, speed=SpeedPerturb(prob=0.0))(path)
    assert c.speed is None and c.tempo is not None


def test_carriers_keep_their_positional_arguments():
    from codes.transforms import PCMClip, RawAudioBatch
    pcm = lambda n: torch.arange(n, dtype=torch.int16)                  # noqa: E731
    c = PCMClip(pcm(4), 1.1, 2.0, None, None, 7)
    assert (c.tempo, c.gain_db, c.noise, c.spec, c.reverb, c.speed) == (1.1, 2.0, None, None, 7, None)
    b = RawAudioBatch(pcm(8), [0, 3, 8], [1.0, 1.1], [0.0, 2.0], [None, (0, 0.1, 0.2)], [None, (0.5,)], [None, 2])
    assert (b.tempos, b.gains_db, b.noise, b.spec, b.reverb, b.speed) == \
        ([1.0, 1.1], [0.0, 2.0], [None, (0, 0.1, 0.2)], [None, (0.5,)], [None, 2], None)
    plain = RawAudioBatch.from_clips([PCMClip(pcm(5)), PCMClip(pcm(3), tempo=1.1, gain_db=2.0, reverb=1)])
    assert plain.speed is None and plain.reverb == [None, 1] and plain.tempos == [1.0, 1.1]
    draws = [None, 2, 0]
    batch = RawAudioBatch.from_clips([PCMClip(pcm(5), speed=d) for d in draws])
    assert batch.speed == draws and batch.tempos is None and batch.reverb is None and batch.offsets == [0, 5, 10, 15]
    assert batch.to('cpu').speed == draws and batch.pin_memory.__self__ is batch
    assert RawAudioBatch(batch.pcm, batch.offsets).speed is None
    assert RawAudioBatch.from_clips([PCMClip(pcm(5), speed=0)]).speed == [0]          # index 0 is a draw, not "none"


def test_frontend_without_the_tables_refuses_a_batch_with_draws():
    """(refused before anything touches the device: no GPU needed)"""
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch
    front = BatchSpectrogram()
    assert front.speed is None
    batch = RawAudioBatch.from_clips([PCMClip(torch.zeros(400, dtype=torch.int16), speed=0)])
    with pytest.raises(RuntimeError, match='speed draws'):
        front(batch)


def test_pickling_carries_no_device_tensor():
    from codes.transforms import SpeedPerturb
    sp = SpeedPerturb(factors=(0.9, 1.1), prob=0.25)
    sp.tables()
    back = pickle.loads(pickle.dumps(sp))
    assert (back.factors, back.prob, back._table_of) == (sp.factors, 0.25, sp._table_of) and back._tables is None

    def tensors(v):
        if isinstance(v, torch.Tensor):
            yield v
        elif isinstance(v, dict):
            for w in v.values():
                yield from tensors(w)
        elif isinstance(v, (list, tuple)):
            for w in v:
                yield from tensors(w)
    assert not list(tensors(back.__dict__)) and not list(tensors(sp.__getstate__()))
    assert back.draw(np.random.RandomState(1)) == sp.draw(np.random.RandomState(1))
    assert [t[:2] for t in back.tables()] == [(1, 1), (10, 9), (10, 11)]


# ------------------------------------------------------------------------------------------------ config
def _config(speed=None, **training):
    from codes.utils.io_utils import AttrDict
    if speed is not None:
        training['speed'] = AttrDict(speed)
    return AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})


def test_config_block(tmp_path):
    import shutil

    from codes import transforms as T
    from codes.utils import training_utils as tu
    assert tu.get_speed(_config()) is None and tu.get_speed(_config(augment=True)) is None
    sp = tu.get_speed(_config(speed={}))
    assert isinstance(sp, T.SpeedPerturb) and sp.factors == (0.9, 1.0, 1.1) and sp.prob == 1.0
    sp = tu.get_speed(_config(speed={'factors': [0.95, 1.05], 'prob': 0.5}))
    assert sp.factors == (0.95, 1.05) and sp.prob == 0.5
    with pytest.raises(ValueError, match='factor_list'):
        tu.get_speed(_config(speed={'factor_list': [0.9]}))
    with pytest.raises(ValueError, match=r'3\.0'):
        tu.get_speed(_config(speed={'factors': [3.0]}))
    data = str(tmp_path / 'data')
    os.makedirs(data)
    shutil.copy(os.path.join(ROOT, 'data', 'labels.en.json'), data)
    train_t, val_t, _ = tu.get_default_transforms(data, _config(augment=True))
    assert T.waveform_speed(train_t) is None and T.waveform_speed(val_t) is None
    cfg = _config(speed={'factors': [0.9, 1.1]})
    train_t, val_t, _ = tu.get_default_transforms(data, cfg)
    assert isinstance(T.waveform_speed(train_t), T.SpeedPerturb) and T.waveform_speed(val_t) is None      # training set only
    assert not train_t.transforms[0].augment and T.waveform_reverb(train_t) is None                       # independent
    train_t, _, _ = tu.get_default_transforms(data, cfg, noise=False)                 # evaluation does not look at the block
    assert T.waveform_speed(train_t) is None
    train_t, val_t, _ = tu.get_default_transforms(data, cfg, gpu_frontend=False)      # per clip: ToTensor applies it itself
    assert [type(t) for t in train_t.transforms] == [T.ToTensor, T.ToSpectrogram]
    assert train_t.transforms[0].speed is not None and val_t.transforms[0].speed is None
    with pytest.raises(ValueError, match='rate'):
        tu.get_default_transforms(data, _config(speed={'rate': 1.1}))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_point_is_declared_bound_exported_and_documented():
    from ds2hip import lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\n\s*int\s+ds2_resample_var\s*\(([^;]*?)\)\s*;', code)
    assert m and len(m.group(1).split(',')) == 12 == len(lib.SIGNATURES['ds2_resample_var'][1])
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'ds2_resample_var')
    assert 'speed perturbation / per-clip ratio' in hdr
    assert int(re.search(r'#define\s+DS2_RESAMPLE_VAR_TABLES\s+(\d+)', hdr).group(1)) == ops.RESAMPLE_VAR_TABLES == 16
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404                # new symbols only
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        assert 'ds2_resample_var' in open(os.path.join(ROOT, doc)).read(), doc


def test_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    handle = lib.load()
    fn = handle.ds2_resample_var
    p = ctypes.c_void_p(1 << 20)                                        # device pointers: never dereferenced, refused first

    def call(tables, bank_floats=4096, B=1, n_tables=None, max_out=10, null=None):
        desc = np.asarray(tables, np.int32).reshape(-1, 4)
        args = [p, p, p, p, B, desc.ctypes.data, len(desc) if n_tables is None else n_tables, p, bank_floats, max_out, p, None]
        if null is not None:
            args[null] = None
        return fn(*args), handle.ds2_last_error().decode()
    ok = [1, 1, 1, 0]
    for kw in (dict(B=0), dict(B=65536), dict(n_tables=0), dict(tables=[ok] * 17), dict(max_out=-1)):
        rc, text = call(kw.pop('tables', [ok]), **kw)
        assert rc == lib.ERR_ARG and 'ds2_resample_var' in text, kw
    for bad in ([0, 1, 1, 0], [1025, 1, 1, 0], [1, 0, 1, 0], [1, 4097, 1, 0], [1, 1, 0, 0], [1, 1, 2, 0], [1, 1, 1025, 0],
                [1, 1, 1, -1], [1, 1, 1, 4096], [2, 1, 3, 4091], [1, 1, 1, 2 ** 31 - 1]):
        rc, text = call([ok, bad])
        assert rc == lib.ERR_ARG and 'table 1' in text, bad
    for null in (0, 1, 2, 3, 5, 7, 10):
        assert call([ok], null=null)[0] == lib.ERR_ARG, null
    assert call([ok, [2, 1, 3, 4090]], max_out=0)[0] == 0                            # valid and empty: nothing is launched


def test_wrapper_refuses_before_any_launch():
    from ds2hip import ops
    with pytest.raises(RuntimeError, match='on the device'):
        ops.resample_var(torch.zeros(8, dtype=torch.int16), [0, 8], [0], [ops.speed_design(1.0)])
