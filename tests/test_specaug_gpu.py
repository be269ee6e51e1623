"""SpecAugment on the device (csrc/specaug.hip, ``ds2_spec_augment``) against tests/specaug_ref.py.

Masks, padding and every frame the warp copies (frac == 0) are exact.  A warped cell is
fmaf(frac, x[i1] - x[i0], x[i0]) with frac = (float)(num % den) / (float)den: three float32 roundings (the quotient, the
difference, the fma), so it must lie within

    2^-24 * (3 * |x[i1] - x[i0]| + max(|x[i0]|, |x[i1]|))

of the float64 value computed from the same integers -- derived from the formula, not measured.  Each warp test prints the
largest ratio of error to bound it saw (profiles/specaug_errors.md records a run)."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import specaug_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
NB = 161
B, TMAX = 4, 37


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


def _input(frames, t_max, seed, pad=0.0):
    """Random normal clips; frames past a clip's own hold ``pad`` (0 is what the frontend writes)."""
    x = np.random.RandomState(seed).standard_normal((len(frames), t_max, NB)).astype(np.float32)
    for b, t in enumerate(frames):
        x[b, t:] = pad
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run(ops, x, frames, warp=None, fmask=None, tmask=None, mask_value=0.0, prefill=None):
    """-> (result as numpy, the device input after the call as numpy).  ``prefill``: a separate out filled with it."""
    xd = torch.from_numpy(x).to(DEV)
    out = None if prefill is None else torch.full(x.shape, prefill, dtype=torch.float32, device=DEV)
    got = ops.spec_augment(xd, frames, warp, fmask, tmask, mask_value, out=out)
    torch.cuda.synchronize()
    if warp is None and prefill is None:
        assert got is xd                                                # masks only: in place
    else:
        assert got is not xd and (out is None or got is out)
    return got.cpu().numpy(), xd.cpu().numpy()


def _ratio(got, want, bound):
    """Largest error / bound over the cells with a bound; every other cell must be exact."""
    exact = bound == 0
    assert np.array_equal(got[exact].astype(np.float64), want[exact], equal_nan=True), 'a copied / masked / padded cell differs'
    if exact.all():
        return 0.0
    err = np.abs(got[~exact].astype(np.float64) - want[~exact])
    return float((err / bound[~exact]).max())


# ------------------------------------------------------------------------------------------------ masks only, in place
MASK_CASES = {
    # name: (frames, fmask (B, MF, 2), tmask (B, MT, 2), mask_value)
    'edges': ([37, 30, 37, 12], [[[0, 5], [150, 11]]] * 4,               # bin 0, and ending at bin 161
              [[[30, 7]], [[23, 7]], [[0, 1]], [[11, 1]]], 0.0),         # time masks ending exactly at T_b
    'clamped': ([37, 20, 37, 9], [[[-4, 9], [158, 1000]]] * 4, [[[-3, 5], [18, 500]]] * 4, 1.25),
    'overlapping': ([37, 37, 25, 31], [[[10, 30], [25, 30], [25, 5]]] * 4, [[[5, 10], [8, 3], [14, 6]]] * 4, 0.0),
    'zero widths': ([37, 37, 37, 37], [[[10, 0], [0, 0]]] * 4, [[[5, 0], [36, 0]]] * 4, 7.0),
    'eight of each': ([37, 33, 29, 36], [[[20 * m + b, m + 1] for m in range(8)] for b in range(4)],
                      [[[4 * m + b, 1 + m % 3] for m in range(8)] for b in range(4)], -1.0),
    'one frame': ([1, 1, 37, 1], [[[3, 4]]] * 4, [[[0, 1]], [[0, 0]], [[1, 2]], [[5, 3]]], 2.0),
    'short clip, other value': ([37, 11, 5, 20], [[[100, 27]]] * 4, [[[2, 6]]] * 4, -3.5),
    'frequency only': ([37, 18, 37, 2], [[[0, 161]], [[160, 1]], [[80, 1]], [[0, 1]]], None, 0.5),
    'time only': ([37, 18, 37, 2], None, [[[0, 37]], [[17, 1]], [[16, 16]], [[1, 1]]], 0.5),
}


@pytest.mark.parametrize('name', sorted(MASK_CASES))
def test_masks_in_place_are_exact(ops, name):
    frames, fmask, tmask, value = MASK_CASES[name]
    x = _input(frames, TMAX, 1)
    got, _ = _run(ops, x, frames, None, fmask, tmask, value)
    want, bound = ref.batch_ref(x, frames, None, fmask, tmask, value)
    assert not bound.any()
    assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))    # masked cells, and every other cell bit for bit
    masked = np.stack([np.pad(ref.masked_cells(t, None if fmask is None else fmask[b], None if tmask is None else tmask[b]),
                              ((0, TMAX - t), (0, 0))) for b, t in enumerate(frames)])
    assert np.array_equal(_bits(got[~masked]), _bits(x[~masked]))
    assert np.all(got[masked] == np.float32(value)) and (masked.any() or name == 'zero widths')
    for b, t in enumerate(frames):
        assert not got[b, t:].any() and not np.signbit(got[b, t:]).any()   # padding: exactly +0


def test_nan_and_inf_under_and_beside_a_mask(ops):
    frames = [37, 20, 37, 37]
    x = _input(frames, TMAX, 2)
    fmask, tmask = [[[40, 10]]] * 4, [[[12, 4]]] * 4
    under = [(0, 3, 40), (0, 30, 49), (1, 12, 0), (2, 15, 160), (3, 13, 45)]
    beside = [(0, 3, 39), (0, 30, 50), (1, 11, 0), (2, 16, 160), (3, 16, 39)]
    for k, (b, t, f) in enumerate(under):
        x[b, t, f] = np.nan if k % 2 else np.inf
    for k, (b, t, f) in enumerate(beside):
        x[b, t, f] = np.inf if k % 2 else np.nan
    got, _ = _run(ops, x, frames, None, fmask, tmask, -2.0)
    want, _ = ref.batch_ref(x, frames, None, fmask, tmask, -2.0)
    assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    for b, t, f in under:
        assert got[b, t, f] == -2.0
    for b, t, f in beside:
        assert _bits(got[b, t, f]) == _bits(x[b, t, f]) and not np.isfinite(got[b, t, f])
    assert np.isfinite(got).sum() == got.size - len(beside)


def test_nothing_to_do_and_wrapper_refusals(ops):
    frames = [37, 20, 37, 5]
    x = _input(frames, TMAX, 3)
    got, _ = _run(ops, x, frames)                                       # no table at all: returns x untouched
    assert np.array_equal(_bits(got), _bits(x))
    xd = torch.from_numpy(x).to(DEV)
    with pytest.raises(ValueError, match='4096'):                       # T_b = 4097 with a warp
        ops.spec_augment(torch.zeros(1, 4097, NB, device=DEV), [4097], warp=[[5, 5]])
    for bad in (dict(warp=[[0, 0], [0, 20], [0, 0], [0, 0]]), dict(warp=[[0, 0], [-1, 0], [0, 0], [0, 0]]),
                dict(warp=[[0, 0]] * 4, out=xd), dict(fmask=[[[0, 1]] * 9] * 4), dict(tmask=[[[0, 1]] * 9] * 4),
                dict(fmask=[[[0.5, 1]]] * 4)):
        with pytest.raises(ValueError):
            ops.spec_augment(xd, frames, **bad)
    for bad_frames in ([37, 20, 37], [37, 20, 38, 5], [37, 0, 37, 5]):
        with pytest.raises(ValueError):
            ops.spec_augment(xd, bad_frames, fmask=[[[0, 1]]] * len(bad_frames))
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x))            # nothing was launched
    # tensors are taken as well as lists
    a = ops.spec_augment(xd.clone(), torch.tensor(frames), None, torch.tensor([[[3, 4]]] * 4), torch.tensor([[[2, 2]]] * 4), 9.0)
    b = ops.spec_augment(xd.clone(), frames, None, [[[3, 4]]] * 4, [[[2, 2]]] * 4, 9.0)
    assert torch.equal(a, b) and float(a[0, 2, 0]) == 9.0


# ------------------------------------------------------------------------------------------------ warp
W = 5
WARP_CASES = {
    # name: (frames, warp (B, 2))
    'identity': ([37, 20, 1, 11], [[18, 18], [0, 0], [0, 0], [10, 10]]),
    'c2 = 0': ([37, 20, 2, 11], [[18, 0], [1, 0], [1, 0], [10, 0]]),
    'c2 = T - 1': ([37, 20, 2, 11], [[18, 36], [1, 19], [0, 1], [0, 10]]),
    'T = 2W + 1': ([11, 11, 11, 11], [[5, 0], [5, 10], [5, 3], [5, 6]]),
    'mixed': ([37, 36, 35, 34], [[10, 20], [20, 10], [1, 34], [33, 1]]),
}


@pytest.mark.parametrize('name', sorted(WARP_CASES))
def test_warp_within_three_roundings(ops, name):
    frames, warp = WARP_CASES[name]
    x = _input(frames, TMAX, 4, pad=123.0)                              # the input's padding is never read
    got, x_after = _run(ops, x, frames, warp)
    assert np.array_equal(_bits(x_after), _bits(x))                     # the input is not written
    want, bound = ref.batch_ref(x, frames, warp)
    r = _ratio(got, want, bound)
    print('specaug warp %s: error / bound %.3f' % (name, r))
    assert r <= 1.0
    for b, t in enumerate(frames):
        assert not got[b, t:].any()
    if name == 'identity':
        assert not bound.any()
        for b, t in enumerate(frames):
            assert np.array_equal(_bits(got[b, :t]), _bits(x[b, :t]))   # c2 == c: the input bit for bit
    else:
        assert bound.any() and not np.array_equal(got[0, :frames[0]], x[0, :frames[0]])


def test_identity_warp_keeps_negative_zero_and_non_finite_neighbours(ops):
    x = _input([37], TMAX, 5)
    x[0, 3, 7], x[0, 4, 7], x[0, 10, 0] = -0.0, np.inf, np.nan
    got, _ = _run(ops, x, [37], [[9, 9]])
    assert np.array_equal(_bits(got), _bits(x))


def test_warp_of_the_longest_clip(ops):
    """One clip at T_b = t_max = 4096: the products num reach 2^24 - 1 and are still exact in float."""
    T = 4096
    x = _input([T], T, 6)
    for warp in ([[2048, 2000]], [[4000, 96]], [[1, 4095]]):
        got, _ = _run(ops, x, [T], warp)
        want, bound = ref.batch_ref(x, [T], warp)
        r = _ratio(got, want, bound)
        print('specaug warp T = 4096 %s: error / bound %.3f' % (warp[0], r))
        assert r <= 1.0 and bound.any()


# ------------------------------------------------------------------------------------------------ warp + masks
def test_warp_and_masks_into_a_nan_filled_out(ops):
    frames = [37, 20, 1, 29]
    warp = [[10, 20], [12, 5], [0, 0], [14, 14]]
    fmask = [[[0, 5], [150, 11]], [[-4, 9], [60, 27]], [[3, 4], [0, 0]], [[80, 1], [81, 1]]]
    tmask = [[[30, 7], [0, 2]], [[18, 500], [5, 0]], [[0, 0], [0, 0]], [[28, 1], [3, 9]]]
    x = _input(frames, TMAX, 7, pad=np.nan)                             # NaN in the input's padding: never read
    got, _ = _run(ops, x, frames, warp, fmask, tmask, -3.5, prefill=np.nan)
    assert not np.isnan(got).any()                                      # every cell was written
    want, bound = ref.batch_ref(np.nan_to_num(x), frames, warp, fmask, tmask, -3.5)
    r = _ratio(got, want, bound)
    print('specaug warp + masks: error / bound %.3f' % r)
    assert r <= 1.0
    for b, t in enumerate(frames):
        assert not got[b, t:].any() and not np.signbit(got[b, t:]).any()   # padding exactly +0, not mask_value
        m = ref.masked_cells(t, fmask[b], tmask[b])
        assert np.all(got[b, :t][m] == np.float32(-3.5))
    # no warp, a separate out: a copy with masks, every cell written as well
    got, x_after = _run(ops, x, frames, None, fmask, tmask, -3.5, prefill=np.nan)
    want, bound = ref.batch_ref(np.nan_to_num(x), frames, None, fmask, tmask, -3.5)
    assert not bound.any() and np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    assert np.array_equal(_bits(x_after), _bits(x))


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize('warped', [False, True])
def test_a_clip_does_not_depend_on_its_company(ops, warped):
    T = 29
    clip = _input([T], T, 8)[0]
    warp, fmask, tmask = [11, 17], [[5, 20], [140, 30]], [[20, 4], [0, 3]]

    def run(pos, n, t_max, seed, prefill):
        frames = [min(t_max, 7 + 9 * k) for k in range(n)]
        frames[pos] = T
        x = _input(frames, t_max, seed)
        x[pos, :T] = clip
        rng = np.random.RandomState(seed)
        wp = [[int(rng.randint(f)), int(rng.randint(f))] for f in frames]
        fm = [[[int(rng.randint(150)), int(rng.randint(28))] for _ in range(2)] for _ in frames]
        tm = [[[int(rng.randint(f)), int(rng.randint(9))] for _ in range(2)] for f in frames]
        wp[pos], fm[pos], tm[pos] = warp, fmask, tmask
        got, _ = _run(ops, x, frames, wp if warped else None, fm, tm, -1.5, prefill=prefill if warped else None)
        assert not got[pos, T:].any()
        return got[pos, :T]

    alone = run(0, 1, T, 0, np.nan)
    want, bound = ref.spec_augment_ref(clip, T, warp if warped else None, fmask, tmask, -1.5)
    assert _ratio(alone, want, bound) <= 1.0
    for pos, n, t_max, seed, prefill in ((0, 4, 37, 1, 0.0), (3, 4, 37, 2, 5.0), (3, 4, 64, 3, np.inf), (0, 4, 64, 4, -1.0),
                                         (1, 2, 37, 5, np.nan)):
        assert np.array_equal(_bits(run(pos, n, t_max, seed, prefill)), _bits(alone)), (pos, n, t_max)


# ------------------------------------------------------------------------------------------------ through the classes
def _pcm(n, seed):
    return (np.random.RandomState(seed).standard_normal(n) * 3277).clip(-32768, 32767).astype(np.int16)


def _write_wav(path, samples):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(np.asarray(samples, dtype='<i2').tobytes())
    return path


@pytest.fixture(scope='module')
def wav_set(tmp_path_factory):
    root = tmp_path_factory.mktemp('specaug_wavs')
    return [_write_wav(str(root / ('u%d.wav' % i)), _pcm(n, 50 + i)) for i, n in enumerate((16000, 21000, 9000))]


@pytest.mark.parametrize('time_warp', [0, 6])
def test_loader_to_frontend_equals_the_reference(wav_set, time_warp):
    from codes.transforms import BatchSpectrogram, RawAudioBatch, SpecAugment, ToTensor
    sa = SpecAugment(freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=0.2, time_warp=time_warp,
                     mask_value=-0.75)
    loader_t = ToTensor(augment=True, defer=True, spec_augment=sa)
    np.random.seed(31)
    batch = RawAudioBatch.from_clips([loader_t(p) for p in wav_set])
    assert batch.spec is not None and all(len(d) == 8 + 2 * (time_warp > 0) for d in batch.spec)
    got, pct = BatchSpectrogram(spec_augment=sa)(batch.to(DEV))
    plain_batch = RawAudioBatch(batch.pcm, batch.offsets, batch.tempos, batch.gains_db)
    plain, plain_pct = BatchSpectrogram()(plain_batch.to(DEV))
    assert torch.equal(pct, plain_pct)
    t_max = plain.shape[1]
    frames = [int(round(float(p) * t_max)) for p in pct]
    assert max(frames) == t_max and len(set(frames)) == 3               # tempo was drawn: three different lengths
    warp, fmask, tmask = sa.params(batch.spec, frames)
    assert (warp is None) == (time_warp == 0)
    want, bound = ref.batch_ref(plain.cpu().numpy(), frames, warp, fmask, tmask, -0.75)
    got = got.cpu().numpy()
    if time_warp == 0:
        assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))
    else:
        assert any(c != c2 for c, c2 in warp)
        r = _ratio(got, want, bound)
        print('specaug through the frontend, time_warp %d: error / bound %.3f' % (time_warp, r))
        assert r <= 1.0
    masked = sum(int(ref.masked_cells(t, fmask[b], tmask[b]).sum()) for b, t in enumerate(frames))
    assert masked > 0 and int((got == np.float32(-0.75)).sum()) >= masked


def test_prob_zero_is_the_plain_frontend(wav_set):
    from codes.transforms import BatchSpectrogram, RawAudioBatch, SpecAugment, ToTensor
    sa = SpecAugment(prob=0.0, time_warp=4)
    np.random.seed(32)
    batch = RawAudioBatch.from_clips([ToTensor(augment=True, defer=True, spec_augment=sa)(p) for p in wav_set])
    assert batch.spec is None                                            # no clip drew: nothing travels, nothing is launched
    a, pa = BatchSpectrogram(spec_augment=sa)(batch.to(DEV))
    b, pb = BatchSpectrogram()(batch.to(DEV))
    assert torch.equal(a, b) and torch.equal(pa, pb)
    # a batch in which SOME clip missed: that clip is the plain frontend's, bit for bit
    sa = SpecAugment(time_warp=4)
    batch.spec = [None, sa.draw(np.random.RandomState(1)), None]
    c, _ = BatchSpectrogram(spec_augment=sa)(batch.to(DEV))
    assert torch.equal(c[0], b[0]) and torch.equal(c[2], b[2]) and not torch.equal(c[1], b[1])
    with pytest.raises(RuntimeError, match='SpecAugment'):
        BatchSpectrogram()(batch.to(DEV))


def test_per_clip_call_equals_the_batched_result(ops):
    from codes.transforms import SpecAugment
    x = torch.from_numpy(_input([50], 50, 9)[0])
    for time_warp in (0, 7):
        sa = SpecAugment(time_warp=time_warp, time_ratio=0.5)
        np.random.seed(8)
        draw = sa.draw()
        np.random.seed(8)
        y = sa(x)
        assert y.device.type == 'cpu' and y.shape == x.shape and not torch.equal(y, x)
        want = sa.apply_batch(x.to(DEV).unsqueeze(0).clone(), [50], [draw])[0]
        assert torch.equal(want.cpu(), y)
        x_dev = x.to(DEV)
        np.random.seed(8)
        on_dev = sa(x_dev)                                               # a device tensor stays there, and x is not written
        assert on_dev.is_cuda and torch.equal(on_dev.cpu(), y) and torch.equal(x_dev.cpu(), x)
    assert SpecAugment(prob=0.0)(x) is x


# ------------------------------------------------------------------------------------------------ one training step
def test_one_training_step_with_the_config_block(tmp_path, wav_set):
    from codes.data import AudioDataLoader, AudioDataset
    from codes.engine import Trainer
    from codes.model import DeepSpeech
    from codes.transforms import BatchSpectrogram, waveform_noise, waveform_scale, waveform_spec_augment
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    rows = []
    for i, p in enumerate(wav_set):
        (tmp_path / ('u%d.txt' % i)).write_text('HELLO WORLD %s' % ('AB' * (i + 1)))
        rows.append('%s,u%d.txt,1.0' % (p, i))
    (tmp_path / 'm.csv').write_text('\n'.join(rows) + '\n')

    def one_step(block):
        training = {'augment': True, 'batch_size': 3}
        if block is not None:
            training['spec_augment'] = AttrDict(block)
        cfg = AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})
        train_t, val_t, target_t = tu.get_default_transforms(os.path.join(ROOT, 'data'), cfg)
        assert waveform_spec_augment(val_t) is None and (waveform_spec_augment(train_t) is not None) == (block is not None)
        ds = AudioDataset(str(tmp_path), str(tmp_path / 'm.csv'), train_t, target_t[0])
        loader = AudioDataLoader(ds, batch_size=3, num_workers=0, raw_audio=True)
        torch.manual_seed(5)
        np.random.seed(5)
        model = DeepSpeech(rnn_hidden_size=32, num_rnn_layers=2, num_classes=29).to(DEV)
        opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
        frontend = BatchSpectrogram(device=DEV, scale=waveform_scale(train_t), noise=waveform_noise(train_t),
                                    spec_augment=waveform_spec_augment(train_t))
        trainer = Trainer(model, opt, device=DEV, max_norm=400, frontend=frontend)
        batch = next(iter(loader))
        assert (batch[0].spec is not None) == (block is not None)
        return float(trainer.update(batch))

    block = {'time_warp': 5, 'freq_width': 40, 'mask_value': 0.0}
    with_it, again, without = one_step(block), one_step(block), one_step(None)
    print('one step: loss %.6f with SpecAugment, %.6f again, %.6f without' % (with_it, again, without))
    assert np.isfinite(with_it) and np.isfinite(without)
    assert with_it == again
    assert with_it != without
