"""SpecAugment without a GPU: the C ABI's new entry point and its refusals, the numpy reference (tests/specaug_ref.py) on
cases worked out by hand, SpecAugment's draws and ``params``, and the config wiring."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import specaug_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_point_is_declared_bound_and_exported():
    from ds2hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\n\s*int\s+ds2_spec_augment\s*\(([^;]*?)\)\s*;', code)
    assert m, 'ds2_spec_augment is not declared in include/ds2hip.h'
    assert len(m.group(1).split(',')) == 12
    assert len(lib.SIGNATURES['ds2_spec_augment'][1]) == 12
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), 'ds2_spec_augment'), 'ds2_spec_augment is not exported'
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404
    for doc in ('INTEGRATION.md', 'README.md'):
        assert 'ds2_spec_augment' in open(os.path.join(ROOT, doc)).read(), doc


# argument positions of ds2_spec_augment
X, OUT, B, TMAX, FRAMES, WARP, FMASK, MF, TMASK, MT, VALUE, STREAM = range(12)


def test_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    fn = lib.load().ds2_spec_augment
    ptr = ctypes.c_void_p
    x, far, tab = ptr(1 << 20), ptr(1 << 40), ptr(16)                   # never dereferenced: every call is refused first
    nbytes = 4 * 37 * 161 * 4
    ok = [x, far, 4, 37, tab, tab, tab, 2, tab, 2, 0.0, None]          # (a valid call: never made)
    bad = [(X, None), (OUT, None), (FRAMES, None),
           (B, 0), (B, -1), (B, 65536), (TMAX, 0), (TMAX, -5),
           (MF, -1), (MF, 9), (MT, -1), (MT, 9),
           (FMASK, None), (TMASK, None),                                 # a null table with a non-zero count
           (OUT, x),                                                     # in place with a warp
           (OUT, ptr((1 << 20) + 4)), (OUT, ptr((1 << 20) + nbytes - 4)), (OUT, ptr((1 << 20) - nbytes + 4))]
    for pos, value in bad:
        args = list(ok)
        args[pos] = value
        assert fn(*args) == lib.ERR_ARG, (pos, value)
        assert b'ds2_spec_augment' in lib.load().ds2_last_error()
    # without a warp a partial overlap is refused as well (equal pointers are the in-place form)
    args = list(ok)
    args[WARP], args[OUT] = None, ptr((1 << 20) + 644)
    assert fn(*args) == lib.ERR_ARG


def test_nothing_to_do_returns_at_once():
    """Every table NULL with MF == MT == 0, in place: not an error and no launch (the pointers are never dereferenced, and
    this process has no device)."""
    from ds2hip import lib
    fn = lib.load().ds2_spec_augment
    x = ctypes.c_void_p(1 << 20)
    assert fn(x, x, 3, 50, ctypes.c_void_p(16), None, None, 0, None, 0, -1.0, None) == 0
    assert fn(x, x, 3, 50, ctypes.c_void_p(16), None, ctypes.c_void_p(16), 0, ctypes.c_void_p(16), 0, -1.0, None) == 0


def test_wrapper_refuses_cpu_tensors():
    from ds2hip import ops
    with pytest.raises(RuntimeError):
        ops.spec_augment(torch.zeros(1, 5, 161), [5], fmask=[[[0, 3]]])


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_warp_by_hand():
    # T = 10, frame 4 lands on frame 6: left half t < 6 reads 4 t / 6, right half reads 4 + (t - 6) 6 / 4
    i0, i1, rem, den = ref.warp_rows(10, 4, 6)
    assert list(i0) == [0, 0, 1, 2, 2, 3, 4, 5, 7, 8]
    assert list(i1) == [1, 1, 2, 3, 3, 4, 5, 6, 8, 9]
    assert list(rem) == [0, 4, 2, 0, 4, 2, 0, 2, 0, 2] and list(den) == [6] * 6 + [4] * 4
    x = np.zeros((12, 161), np.float32)
    x[:10] = np.arange(10, dtype=np.float32)[:, None] * 3.0 + np.arange(161, dtype=np.float32)[None, :]
    x[10:] = 99.0                                                       # padding of the input is never looked at
    out, bound = ref.spec_augment_ref(x, 10, warp=(4, 6))
    pos = np.array([0, 4 / 6., 8 / 6., 2, 16 / 6., 20 / 6., 4, 5.5, 7, 8.5])     # a ramp is resampled exactly
    np.testing.assert_allclose(out[:10, 0], 3.0 * pos, rtol=1e-15)
    np.testing.assert_allclose(out[:10, 160], 3.0 * pos + 160, rtol=1e-15)
    assert np.all(out[10:] == 0) and np.all(bound[10:] == 0)
    assert np.all(bound[[0, 3, 6, 8]] == 0) and np.all(bound[[1, 2, 4, 5, 7, 9]] > 0)
    # the identity, the two ends, and the last frame repeating itself
    for T in (1, 2, 7):
        for c in range(T):
            i0, i1, rem, den = ref.warp_rows(T, c, c)
            assert list(i0) == list(range(T)) and not rem.any()
    i0, i1, rem, den = ref.warp_rows(5, 3, 0)                           # c2 = 0: no left half, the right one reads 3 + 2 t / 5
    assert list(i0) == [3, 3, 3, 4, 4] and list(rem) == [0, 2, 4, 1, 3] and list(i1) == [4, 4, 4, 4, 4]
    i0, i1, rem, den = ref.warp_rows(5, 1, 4)                           # c2 = T - 1: the right half is the one frame c
    assert list(i0) == [0, 0, 0, 0, 1] and list(rem) == [0, 1, 2, 3, 0] and list(den) == [4, 4, 4, 4, 1]


def test_reference_masks_by_hand():
    x = np.random.RandomState(0).standard_normal((9, 161)).astype(np.float32)
    x[1, 3], x[2, 100] = np.nan, np.inf                                 # one under a mask, one beside
    out, bound = ref.spec_augment_ref(x, 7, fmask=[(-2, 5), (159, 40), (50, 0)], tmask=[(5, 9), (0, -3)], mask_value=-3.5)
    m = np.zeros((9, 161), bool)
    m[:7, 0:3] = m[:7, 159:161] = True
    m[5:7] = True
    assert np.all(out[m] == -3.5) and not bound.any()
    keep = ~m
    keep[7:] = False
    assert np.array_equal(out[keep], x[keep].astype(np.float64), equal_nan=True)
    assert np.isnan(out[1, 3]) and np.isinf(out[2, 100])                # beside the masks: untouched
    assert np.all(out[7:] == 0)                                         # padding is zero whatever the mask value
    assert ref.masked_cells(7, [(0, 0)], [(3, 0)]).sum() == 0


# ------------------------------------------------------------------------------------------------ constructor, draws
def test_constructor_defaults_repr_and_validation():
    from codes.transforms import SpecAugment
    sa = SpecAugment()
    assert (sa.freq_masks, sa.freq_width, sa.time_masks, sa.time_width, sa.time_ratio, sa.time_warp, sa.prob,
            sa.mask_value) == (2, 27, 2, 100, 0.2, 0, 1.0, 0.0)
    text = repr(SpecAugment(time_warp=5, prob=0.5, mask_value=-1.0))
    for part in ('SpecAugment(', 'freq_masks=2', 'freq_width=27', 'time_masks=2', 'time_width=100', 'time_ratio=0.2',
                 'time_warp=5', 'prob=0.5', 'mask_value=-1.0'):
        assert part in text, part
    SpecAugment(freq_masks=0, time_masks=8, freq_width=161, time_width=0, time_ratio=1.0, prob=0.0)
    for name, value in (('freq_masks', -1), ('freq_masks', 9), ('time_masks', -1), ('time_masks', 9), ('freq_width', -1),
                        ('freq_width', 162), ('time_width', -1), ('time_ratio', -0.1), ('time_ratio', 1.5), ('prob', -0.1),
                        ('prob', 1.01), ('time_warp', -1), ('freq_masks', 1.5)):
        with pytest.raises(ValueError, match=name):
            SpecAugment(**{name: value})


def test_draw_order_and_count_under_a_seed():
    from codes.transforms import SpecAugment
    for kw, n in (({}, 8), ({'time_warp': 5}, 10), ({'freq_masks': 0, 'time_masks': 3}, 6),
                  ({'freq_masks': 8, 'time_masks': 8, 'time_warp': 1}, 34), ({'freq_masks': 0, 'time_masks': 0}, 0)):
        sa = SpecAugment(prob=1.0, **kw)
        got = sa.draw(np.random.RandomState(3))
        want = np.random.RandomState(3)
        assert want.binomial(1, 1.0) == 1
        u = want.uniform(0, 1, size=n)
        assert isinstance(got, tuple) and len(got) == n and got == tuple(float(v) for v in u)
        assert all(isinstance(v, float) and 0.0 <= v < 1.0 for v in got)
    # the global generator: binomial first, then ONE uniform call, and nothing else
    sa = SpecAugment(prob=0.5, time_warp=2)
    np.random.seed(12)
    got = [sa.draw() for _ in range(40)]
    after = np.random.uniform()
    np.random.seed(12)
    for d in got:
        hit = np.random.binomial(1, 0.5)
        assert bool(hit) == (d is not None)
        if hit:
            assert d == tuple(float(v) for v in np.random.uniform(0, 1, size=10))
    assert after == np.random.uniform() and any(d is None for d in got) and any(d is not None for d in got)
    # an explicit generator leaves the global stream alone
    np.random.seed(6)
    sa.draw(np.random.RandomState(1))
    assert np.random.uniform() == np.random.RandomState(6).uniform()
    assert all(SpecAugment(prob=0.0).draw() is None for _ in range(20))


def _write_clip(path, n, seed):
    import wave
    x = (np.random.RandomState(seed).standard_normal(n) * 3000).astype(np.int16)
    with wave.open(path, 'wb') as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(x.astype('<i2').tobytes())
    return path, x


class _FakeNoise(object):
    """Stands where a NoiseInjection would: one binomial and one uniform per clip (no directory of recordings needed)."""

    def draw(self):
        return (0, float(np.random.uniform(0, 0.5)), 0.25) if np.random.binomial(1, 0.5) else None


def test_no_draw_at_all_without_the_object(tmp_path):
    """ToTensor(augment=True, noise=...) leaves the global np.random state exactly where the same sequence of the
    documented draws leaves it -- nothing is drawn for SpecAugment unless it is configured -- and with it the draw comes
    last, behind tempo, gain and noise."""
    from codes.transforms import PCMClip, SpecAugment, ToTensor
    path, x = _write_clip(str(tmp_path / 'clip.wav'), 2000, 0)
    tt = ToTensor(augment=True, defer=True, noise=_FakeNoise())
    assert tt.spec_augment is None
    np.random.seed(21)
    clips = [tt(path) for _ in range(6)]
    state = np.random.get_state()
    np.random.seed(21)
    noise = _FakeNoise()
    for c in clips:
        assert isinstance(c, PCMClip) and c.spec is None and np.array_equal(c.pcm.numpy(), x)
        assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
        assert c.gain_db == float(np.random.uniform(low=-6, high=8))
        assert c.noise == noise.draw()
    want = np.random.get_state()
    assert state[0] == want[0] and np.array_equal(state[1], want[1]) and state[2:] == want[2:]
    sa = SpecAugment(time_warp=3)
    ts = ToTensor(augment=True, defer=True, noise=_FakeNoise(), spec_augment=sa)
    np.random.seed(21)
    c = ts(path)
    np.random.seed(21)
    assert c.tempo == float(np.random.uniform(low=0.85, high=1.15))
    assert c.gain_db == float(np.random.uniform(low=-6, high=8))
    assert c.noise == noise.draw()
    assert c.spec == sa.draw() and len(c.spec) == 10
    # independent of tempo / gain and of noise
    c = ToTensor(defer=True, spec_augment=sa)(path)
    assert c.tempo is None and c.gain_db is None and c.noise is None and len(c.spec) == 10
    with pytest.raises(ValueError, match='defer=True'):
        ToTensor(defer=False, spec_augment=sa)


# ------------------------------------------------------------------------------------------------ params
LAST = float(np.nextafter(1.0, 0.0))
W = 5


@pytest.mark.parametrize('T', [1, 2 * W, 2 * W + 1, 4096])
def test_params_stay_inside_the_clip(T):
    from codes.transforms import SpecAugment
    sa = SpecAugment(freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=0.2, time_warp=W)
    n = 10
    cap = min(100, int(np.floor(0.2 * T)))
    for u in (0.0, LAST, 0.5):
        for u2 in (0.0, LAST, 0.5):
            draw = (u, u2) * (n // 2)                                   # every (width, start) pair: (u, u2)
            warp, fmask, tmask = sa.params([draw], [T])
            (c, c2), = warp
            assert 0 <= c < T and 0 <= c2 < T
            if T > 2 * W:
                assert W <= c <= T - W - 1 and abs(c2 - c) <= W
                if u == 0.0:
                    assert c == W
                if u == LAST:
                    assert c == T - W - 1
                assert c2 - c == {0.0: -W, LAST: W, 0.5: 0}[u2]
            else:
                assert c == c2                                          # too short to warp: the identity
            assert len(fmask[0]) == 2 and len(tmask[0]) == 2
            for f0, f in fmask[0]:
                assert 0 <= f <= 27 and 0 <= f0 and f0 + f <= 161
                assert f == {0.0: 0, LAST: 27, 0.5: 14}[u]
                if u2 == LAST:
                    assert f0 + f == 161
            for t0, t in tmask[0]:
                assert 0 <= t <= cap and 0 <= t0 and t0 + t <= T
                assert t == {0.0: 0, LAST: cap, 0.5: int(np.floor(0.5 * (cap + 1)))}[u]
                if u2 == LAST:
                    assert t0 + t == T
                if u2 == 0.0:
                    assert t0 == 0


def test_params_special_cases():
    from codes.transforms import SpecAugment
    sa = SpecAugment(freq_masks=1, time_masks=3, time_ratio=0.0)
    warp, fmask, tmask = sa.params([(LAST,) * 8], [500])
    assert warp is None and fmask == [[[161 - 27, 27]]]
    assert all(t == 0 for _, t in tmask[0])                             # time_ratio = 0: no time mask
    # a None draw is the identity: no warp, zero-width masks -- beside a drawn clip
    sa = SpecAugment(time_warp=4)
    warp, fmask, tmask = sa.params([None, (0.5,) * 10], [300, 200])
    assert warp[0][0] == warp[0][1] and fmask[0] == [[0, 0], [0, 0]] and tmask[0] == [[0, 0], [0, 0]]
    assert warp[1] == [4 + 96, 100] and fmask[1] == [[(161 - 14 + 1) // 2, 14]] * 2
    assert tmask[1] == [[(200 - 20 + 1) // 2, 20]] * 2                  # cap = min(100, 0.2 * 200) = 40
    # time_width caps before time_ratio does
    sa = SpecAugment(freq_masks=0, time_masks=1, time_width=7, time_ratio=1.0)
    assert sa.params([(LAST, 0.0)], [1000]) == (None, [[]], [[[0, 7]]])
    # the reference applies what params gives (the tables have the shape ops.spec_augment takes)
    out, _ = ref.batch_ref(np.ones((2, 300, 161), np.float32), [300, 200], warp, fmask, tmask, mask_value=-1.0)
    assert np.all(out[0] == 1.0) and np.all(out[1, 200:] == 0.0)
    assert np.all(out[1, :200, 74:88] == -1.0) and np.all(out[1, 90:110] == -1.0) and out[1, 89, 0] == 1.0


# ------------------------------------------------------------------------------------------------ the batch, the frontend
def test_batch_carries_the_draws_or_none():
    from codes.transforms import PCMClip, RawAudioBatch
    pcm = lambda n: torch.arange(n, dtype=torch.int16)                  # noqa: E731
    assert PCMClip(pcm(3)).spec is None
    plain = RawAudioBatch.from_clips([PCMClip(pcm(5)), PCMClip(pcm(3), tempo=1.1, gain_db=2.0, noise=(0, 0.1, 0.2))])
    assert plain.spec is None and plain.noise == [None, (0, 0.1, 0.2)]
    draws = [None, (0.1, 0.2, 0.3, 0.4), None]
    batch = RawAudioBatch.from_clips([PCMClip(pcm(5), spec=d) for d in draws])
    assert batch.spec == draws and batch.noise is None and batch.tempos is None and batch.offsets == [0, 5, 10, 15]
    assert batch.to('cpu').spec == draws
    assert RawAudioBatch(batch.pcm, batch.offsets).spec is None


def test_pin_memory_keeps_the_draws(monkeypatch):
    """pin_memory replaces the int16 buffer and nothing else (page-locking itself needs a device: stood in for here)."""
    from codes.transforms import PCMClip, RawAudioBatch
    draws = [(0.5, 0.5), None]
    batch = RawAudioBatch.from_clips([PCMClip(torch.zeros(4, dtype=torch.int16), spec=d) for d in draws])
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **k: self.clone())
    pinned = batch.pin_memory()
    assert pinned.spec == draws and pinned.offsets == [0, 4, 8]
    assert pinned.to('cpu', non_blocking=True).spec == draws


def test_frontend_without_the_object_refuses_a_batch_with_draws():
    """(refused before anything touches the device: no GPU needed)"""
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, SpecAugment
    front = BatchSpectrogram()
    assert front.spec_augment is None
    batch = RawAudioBatch.from_clips([PCMClip(torch.zeros(400, dtype=torch.int16), spec=(0.5,) * 8)])
    with pytest.raises(RuntimeError, match='SpecAugment'):
        front(batch)
    sa = SpecAugment()
    assert BatchSpectrogram(spec_augment=sa).spec_augment is sa


# ------------------------------------------------------------------------------------------------ config
def _config(spec_augment=None, **training):
    from codes.utils.io_utils import AttrDict
    if spec_augment is not None:
        training['spec_augment'] = AttrDict(spec_augment)
    return AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})


def test_config_block():
    from codes import transforms as T
    from codes.utils import training_utils as tu
    assert tu.get_spec_augment(_config(augment=True)) is None           # an absent block
    sa = tu.get_spec_augment(_config(spec_augment={}))                  # an empty one: every default
    assert isinstance(sa, T.SpecAugment) and repr(sa) == repr(T.SpecAugment())
    sa = tu.get_spec_augment(_config(spec_augment={'time_warp': 40, 'freq_masks': 1, 'prob': 0.5, 'mask_value': -1.0}))
    assert (sa.time_warp, sa.freq_masks, sa.prob, sa.mask_value) == (40, 1, 0.5, -1.0)
    assert (sa.freq_width, sa.time_masks, sa.time_width, sa.time_ratio) == (27, 2, 100, 0.2)
    with pytest.raises(ValueError) as e:
        tu.get_spec_augment(_config(spec_augment={'freq_mask': 3, 'prob': 1.0}))
    assert "freq_mask" in str(e.value) and 'training.spec_augment' in str(e.value)
    for known in ('freq_masks', 'freq_width', 'time_masks', 'time_width', 'time_ratio', 'time_warp', 'prob', 'mask_value'):
        assert known in str(e.value)
    with pytest.raises(ValueError, match='time_ratio'):
        tu.get_spec_augment(_config(spec_augment={'time_ratio': 2.0}))


def test_default_transforms_with_and_without_the_block():
    from codes import transforms as T
    from codes.utils import training_utils as tu
    data = os.path.join(ROOT, 'data')
    # without the block: exactly today's transforms
    train_t, val_t, _ = tu.get_default_transforms(data, _config(augment=True))
    assert T.waveform_spec_augment(train_t) is None and T.waveform_spec_augment(val_t) is None
    assert [type(t) for t in train_t.transforms] == [T.ToTensor]
    # with it: the training loader draws, validation never does; independent of training.augment and training.noise
    cfg = _config(spec_augment={'time_warp': 8})
    train_t, val_t, _ = tu.get_default_transforms(data, cfg)
    sa = T.waveform_spec_augment(train_t)
    assert isinstance(sa, T.SpecAugment) and sa.time_warp == 8 and T.waveform_spec_augment(val_t) is None
    assert not train_t.transforms[0].augment and train_t.transforms[0].defer and T.waveform_noise(train_t) is None
    assert all(t.spec_augment is None for t in val_t.transforms if isinstance(t, T.ToTensor))
    # evaluation (load_model(return_transforms=True) passes noise=False) does not even look at the block
    broken = _config(spec_augment={'no_such_key': 1})
    with pytest.raises(ValueError, match='no_such_key'):
        tu.get_default_transforms(data, broken)
    train_t, val_t, _ = tu.get_default_transforms(data, broken, noise=False)
    assert T.waveform_spec_augment(train_t) is None
    # the per-utterance contract: the object stands behind the spectrogram, on the training side only
    train_t, val_t, _ = tu.get_default_transforms(data, cfg, gpu_frontend=False)
    assert [type(t) for t in train_t.transforms] == [T.ToTensor, T.ToSpectrogram, T.SpecAugment]
    assert [type(t) for t in val_t.transforms] == [T.ToTensor, T.ToSpectrogram]
    assert train_t.transforms[0].spec_augment is None
