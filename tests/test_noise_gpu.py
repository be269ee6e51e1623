"""Noise injection on the device (csrc/noise.hip, ``ds2_noise_mix``) against tests/noise_ref.py.

The bound needs no measurement.  The kernel's float64 sums differ from numpy's only in their order (relative 3e-11 at
240 000 terms); coef is rounded to float once, the product once and the sum once, so for every sample

    |out - out64|  <= 1.001 * (2^-23 * |coef64 * nz| + 2^-24 * |out64|)
    |coef - coef64| <= 1.001 * 2^-24 * |coef64|

Each test prints the largest ratio of error to bound it saw (profiles/noise_errors.md records a run)."""
import os

import numpy as np
import pytest
import torch

from tests import noise_ref
from tests import small_refs as refs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
SCALES = {'unit': 1.0 / 32768.0, 'int32': 65536.0}
LONG = 240000                                        # 15 s: 59 chunk partials
ZERO_LO, ZERO_LEN = 20000, 12352                    # an all-zero stretch of the bank


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def bank():
    """One int16 buffer; a 'recording' of a case is any range of it.  (numpy, device tensor)"""
    x = (np.random.RandomState(7).standard_normal(LONG + 4200) * 2500).clip(-32768, 32767).astype(np.int16)
    x[ZERO_LO:ZERO_LO + ZERO_LEN] = 0
    return x, torch.from_numpy(x).to(DEV)


def _clip(n, seed, scale):
    """What decode_augment hands on: 16-bit integers times the amplitude scale (some of them -0.0, as its rint leaves them)."""
    q = np.rint(np.random.RandomState(seed).standard_normal(n) * 3000).clip(-32768, 32767).astype(np.float32)
    q[q == 0] = -0.0
    return q * np.float32(scale)


def _cases(chunk):
    """(clip length, recording lo, recording length, start): every clip length against a longer recording (start 0 and the
    last valid start of a plain crop), one exactly as long, one shorter by a sample, and 100 samples under 3 chunks + 7."""
    out = []
    for k, n in enumerate((1, 161, chunk - 1, chunk, chunk + 1, 3 * chunk + 7, LONG)):
        lo = 40001 + 2 * k + 1 if n < LONG else 3                  # odd int16 offsets: no alignment to lean on
        out += [(n, lo, n + 37, 0), (n, lo, n + 37, 37), (n, lo, n, 0)]
        if n > 1:
            out.append((n, lo, n - 1, (n - 1) // 2))
    out.append((3 * chunk + 7, 1001, 100, 63))
    return out


def _run(ops, bank_d, clips, draws, levels, scale, **kw):
    """clips: list of float32 arrays; draws: list of (lo, len, start).  -> (list of per-clip outputs, coef) as numpy."""
    offs = [0] + [int(v) for v in np.cumsum([len(c) for c in clips])]
    wav = torch.from_numpy(np.concatenate(clips)).to(DEV)
    out, coef = ops.noise_mix(wav, offs, bank_d, [d[0] for d in draws], [d[1] for d in draws], [d[2] for d in draws],
                              levels, scale, return_coef=True, **kw)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return [out[offs[i]:offs[i + 1]] for i in range(len(clips))], coef.cpu().numpy()


def _ratios(got, coef, clip, bank_np, draw, level, scale):
    """(worst sample error / bound, coef error / bound) of one clip; asserts nothing."""
    lo, ln, st = draw
    want, coef64 = noise_ref.mix_ref(clip, bank_np, lo, ln, st, level, scale)
    assert np.all(np.isfinite(got)) and np.isfinite(coef)
    if coef64 == 0.0:
        return (0.0 if np.array_equal(got, clip) else np.inf), (0.0 if coef == 0.0 else np.inf)
    nz = noise_ref.noise_crop(bank_np, lo, ln, st, len(clip), scale).astype(np.float64)
    bound = 1.001 * (2.0 ** -23 * np.abs(coef64 * nz) + 2.0 ** -24 * np.abs(want))
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()), float(abs(float(coef) - coef64) / (1.001 * 2.0 ** -24 * abs(coef64)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('scale_name', ['unit', 'int32'])
def test_every_length_and_recording_within_the_bound(ops, bank, scale_name):
    bank_np, bank_d = bank
    scale = SCALES[scale_name]
    cases = _cases(ops.NOISE_CHUNK)
    clips = {n: _clip(n, 100 + n % 97, scale) for n in {c[0] for c in cases}}
    levels = [float(np.float32(v)) for v in np.random.RandomState(3).uniform(0.05, 0.5, len(cases))]
    outs, coefs = _run(ops, bank_d, [clips[c[0]] for c in cases], [c[1:] for c in cases], levels, scale)
    worst = (0.0, 0.0)
    for c, got, coef, level in zip(cases, outs, coefs, levels):
        r_out, r_coef = _ratios(got, coef, clips[c[0]], bank_np, c[1:], level, scale)
        print('noise %s n=%d rec=%d start=%d: out error / bound %.3f, coef error / bound %.3f' %
              (scale_name, c[0], c[2], c[3], r_out, r_coef))
        assert coef > 0
        assert r_out <= 1.0 and r_coef <= 1.0, (c, r_out, r_coef)
        worst = (max(worst[0], r_out), max(worst[1], r_coef))
    print('noise %s WORST: out %.3f coef %.3f over %d clips' % ((scale_name,) + worst + (len(cases),)))


def test_exact_cases(ops, bank):
    bank_np, bank_d = bank
    scale = SCALES['unit']
    ch = ops.NOISE_CHUNK
    n = 2 * ch + 5
    assert n <= ZERO_LEN
    x = _clip(n, 1, scale)
    assert np.signbit(x[x == 0]).any()                               # the input does hold negative zeros
    zeros = np.zeros(n, np.float32)
    clips = [x, x, x, zeros, x]
    draws = [(101, n + 50, 7),                                       # level 0
             (0, 0, 0),                                              # no noise drawn
             (ZERO_LO - 500, ZERO_LEN + 1000, 500),                  # an all-zero crop of a recording non-zero elsewhere
             (101, n + 50, 7),                                       # an all-zero clip
             (101, n + 50, 7)]                                       # an ordinary one, for the in-place comparison
    levels = [0.0, 0.3, 0.3, 0.3, 0.3]
    assert np.any(bank_np[ZERO_LO - 500:ZERO_LO] != 0) and not np.any(bank_np[ZERO_LO:ZERO_LO + n])
    outs, coef = _run(ops, bank_d, clips, draws, levels, scale)
    for k in (0, 1, 2):
        assert np.array_equal(_bits(outs[k]), _bits(x)), k
        assert coef[k] == 0.0
    assert np.array_equal(_bits(outs[3]), _bits(zeros)) and coef[3] == 0.0
    assert coef[4] > 0 and not np.array_equal(outs[4], x)
    assert all(np.all(np.isfinite(o)) for o in outs) and np.all(np.isfinite(coef))
    # in place == out of place, bit for bit
    offs = [0] + [int(v) for v in np.cumsum([len(c) for c in clips])]
    wav = torch.from_numpy(np.concatenate(clips)).to(DEV)
    same = ops.noise_mix(wav, offs, bank_d, [d[0] for d in draws], [d[1] for d in draws], [d[2] for d in draws], levels,
                         scale, out=wav)
    assert same is wav
    assert np.array_equal(_bits(wav.cpu().numpy()), _bits(np.concatenate(outs)))


def test_a_clip_does_not_depend_on_its_company(ops, bank):
    bank_np, bank_d = bank
    scale = SCALES['unit']
    ch = ops.NOISE_CHUNK
    n = 5 * ch + 321
    x, draw, level = _clip(n, 2, scale), (777, 2000, 1234), 0.37     # a recording that wraps, six chunk partials
    (alone,), (c_alone,) = _run(ops, bank_d, [x], [draw], [level], scale)
    r_out, r_coef = _ratios(alone, c_alone, x, bank_np, draw, level, scale)
    assert r_out <= 1.0 and r_coef <= 1.0 and c_alone > 0
    # position 3 of 5, among clips of other lengths, drawn and undrawn mixed, behind an odd number of samples
    others = [_clip(m, 10 + m, scale) for m in (161, 3 * ch + 8, 1000, 7)]
    assert sum(len(o) for o in others[:3]) % 2 == 1
    clips = others[:3] + [x] + others[3:]
    draws = [(5, 300, 2), (0, 0, 0), (9001, 3 * ch + 100, 17), draw, (0, 0, 0)]
    outs, coefs = _run(ops, bank_d, clips, draws, [0.2, 0.0, 0.5, level, 0.1], scale)
    assert np.array_equal(_bits(outs[3]), _bits(alone)) and _bits(coefs[3:4])[0] == _bits([c_alone])[0]
    assert np.array_equal(_bits(outs[1]), _bits(clips[1])) and coefs[1] == 0.0
    # a workspace full of NaN bytes
    from ds2hip import lib
    nbytes = lib.query('ds2_noise_mix_ws_bytes', 1, n)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    assert bool(torch.isnan(ws.view(torch.float64)).all())
    (dirty,), (c_dirty,) = _run(ops, bank_d, [x], [draw], [level], scale, ws=ws)
    assert np.array_equal(_bits(dirty), _bits(alone)) and c_dirty == c_alone


def test_sixty_five_short_clips_in_one_launch(ops, bank):
    bank_np, bank_d = bank
    scale = SCALES['int32']
    rng = np.random.RandomState(4)
    clips = [_clip(161, 300 + b, scale) for b in range(65)]
    draws = [(int(rng.randint(0, 15000)), int(ln), int(rng.randint(0, ln))) for ln in rng.randint(50, 400, 65)]
    levels = [float(np.float32(v)) for v in rng.uniform(0.05, 0.5, 65)]
    outs, coefs = _run(ops, bank_d, clips, draws, levels, scale)
    worst = (0.0, 0.0)
    for b in range(65):
        r = _ratios(outs[b], coefs[b], clips[b], bank_np, draws[b], levels[b], scale)
        assert r[0] <= 1.0 and r[1] <= 1.0, (b, r)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print('noise B=65 x 161 WORST: out %.3f coef %.3f' % worst)


# ------------------------------------------------------------------------------------------------ through the classes
@pytest.fixture()
def noise_dir(tmp_path):
    root = str(tmp_path / 'noise')
    files = noise_ref.write_noise_dir(root, lengths=(30000, 9000, 52000), amplitude=2500)
    return (root,) + noise_ref.bank_of(root, files)[:3]


def _pcm(n, seed):
    return (np.random.RandomState(seed).standard_normal(n) * 3277).clip(-32768, 32767).astype(np.int16)     # 0.1 x white noise


def test_batch_frontend_mixes_what_the_loader_drew(ops, noise_dir):
    from codes.transforms import BatchSpectrogram, NoiseInjection, PCMClip, RawAudioBatch
    root, bank_np, starts, lengths = noise_dir
    ni = NoiseInjection(root, prob=1.0)
    lens = [16000, 20500, 8000, 41000]
    assert lengths == [9000, 30000, 52000]
    draws = [(1, 0.3, 0.6), None, (0, 0.5, 0.999), (0, 0.25, 0.4)]    # a crop, none, a crop that ends at the recording's end, a wrap
    tempos, gains = [1.1, 0.9, 1.0, 0.87], [2.0, -3.0, 0.0, 5.5]
    clips = [PCMClip(torch.from_numpy(_pcm(n, 20 + i)), t, g, d) for i, (n, t, g, d) in enumerate(zip(lens, tempos, gains, draws))]
    batch = RawAudioBatch.from_clips(clips)
    assert batch.noise == draws
    front = BatchSpectrogram(noise=ni)
    inputs, pct = front(batch.to(DEV))
    # the same decode, then the float64 reference mix, then the float64 spectrogram
    flat, offs = ops.decode_augment(batch.pcm.to(DEV), batch.offsets, tempos, gains)
    flat = flat.cpu().numpy()
    mixed = []
    for b, d in enumerate(draws):
        x = flat[offs[b]:offs[b + 1]]
        if d is None:
            mixed.append(x.astype(np.float64))
            continue
        start = noise_ref.start_rule(d[2], lengths[d[0]], len(x))
        out, coef = noise_ref.mix_ref(x, bank_np, starts[d[0]], lengths[d[0]], start, d[1], SCALES['unit'])
        assert coef > 0
        mixed.append(out)
    assert lengths[0] < len(mixed[3]) and lengths[1] > len(mixed[0])   # one recording wraps, one is cropped
    t_max = inputs.shape[1]
    want = refs.batch_log_spectrogram64(mixed, t_max)
    err = float(np.abs(inputs.cpu().numpy() - want).max())
    print('noise through BatchSpectrogram: max spectrogram error %.3g (bound 2e-4)' % err)
    assert err <= 2e-4
    plain = refs.batch_log_spectrogram64([flat[offs[b]:offs[b + 1]] for b in range(4)], t_max)
    assert float(np.abs(want[0] - plain[0]).max()) > 0.05               # the noise is in there
    assert np.array_equal(pct.numpy(), np.asarray([(1 + len(m) // 160) / float(t_max) for m in mixed], np.float32))


def test_batch_without_draws_is_todays_path(noise_dir):
    from codes.transforms import BatchSpectrogram, NoiseInjection, PCMClip, RawAudioBatch
    ni = NoiseInjection(noise_dir[0])
    clips = [PCMClip(torch.from_numpy(_pcm(n, 40 + i)), 1.05, 1.5) for i, n in enumerate((16000, 9000))]
    batch = RawAudioBatch.from_clips(clips)
    assert batch.noise is None
    a, pa = BatchSpectrogram(noise=ni)(batch.to(DEV))
    b, pb = BatchSpectrogram()(batch.to(DEV))
    assert torch.equal(a, b) and torch.equal(pa, pb)
    assert ni._banks == {}                                               # and the bank was never uploaded
    with pytest.raises(RuntimeError, match='noise bank'):
        BatchSpectrogram()(RawAudioBatch.from_clips([PCMClip(clips[0].pcm, noise=(0, 0.2, 0.5))]).to(DEV))


def test_per_clip_call_equals_the_batched_result(ops, noise_dir):
    from codes.transforms import NoiseInjection
    root, bank_np, starts, lengths = noise_dir
    ni = NoiseInjection(root, prob=1.0)
    x = torch.from_numpy(_pcm(12000, 60).astype(np.float32) * np.float32(SCALES['unit']))
    np.random.seed(8)
    torch.manual_seed(8)
    draw = ni.draw()
    np.random.seed(8)
    torch.manual_seed(8)
    y = ni(x)
    assert y.device.type == 'cpu' and y.shape == x.shape and not torch.equal(y, x)
    other = torch.from_numpy(_clip(5000, 61, SCALES['unit']))
    flat = torch.cat([other, x]).to(DEV)
    ni.mix_batch(flat, [0, 5000, 17000], [None, draw], SCALES['unit'])
    assert torch.equal(flat[5000:].cpu(), y) and torch.equal(flat[:5000].cpu(), other)
    start = noise_ref.start_rule(draw[2], lengths[draw[0]], 12000)
    want, _ = noise_ref.mix_ref(x.numpy(), bank_np, starts[draw[0]], lengths[draw[0]], start, draw[1], SCALES['unit'])
    np.testing.assert_allclose(y.numpy(), want, rtol=0, atol=3e-7 * float(np.abs(want).max()))
    x_dev = x.to(DEV)
    np.random.seed(8)                                                    # the same draw once more
    torch.manual_seed(8)
    on_dev = ni(x_dev)                                                   # a device tensor stays there, and x is not written
    assert on_dev.is_cuda and torch.equal(on_dev.cpu(), y) and torch.equal(x_dev.cpu(), x)
    assert ni.prob == 1.0 and NoiseInjection(root, prob=0.0)(x) is x


# ------------------------------------------------------------------------------------------------ one training step
def _corpus(tmp_path, lens):
    rows = []
    for i, n in enumerate(lens):
        noise_ref.write_wav(str(tmp_path / ('u%d.wav' % i)), _pcm(n, 80 + i))
        (tmp_path / ('u%d.txt' % i)).write_text('HELLO WORLD %s' % ('AB' * (i + 1)))
        rows.append('u%d.wav,u%d.txt,%.3f' % (i, i, n / 16000.0))
    (tmp_path / 'm.csv').write_text('\n'.join(rows) + '\n')


def _one_step(tmp_path, noise_block, seed=5):
    from codes.data import AudioDataLoader, AudioDataset
    from codes.engine import Trainer
    from codes.model import DeepSpeech
    from codes.transforms import BatchSpectrogram, waveform_noise, waveform_scale
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    training = {'augment': True, 'batch_size': 3}
    if noise_block is not None:
        training['noise'] = AttrDict(noise_block)
    cfg = AttrDict({'model': AttrDict({'langs': ['en']}), 'training': AttrDict(training)})
    train_t, val_t, target_t = tu.get_default_transforms(os.path.join(ROOT, 'data'), cfg)
    assert waveform_noise(val_t) is None and (waveform_noise(train_t) is not None) == (noise_block is not None)
    ds = AudioDataset(str(tmp_path), str(tmp_path / 'm.csv'), train_t, target_t[0])
    loader = AudioDataLoader(ds, batch_size=3, num_workers=0, raw_audio=True)
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = DeepSpeech(rnn_hidden_size=32, num_rnn_layers=2, num_classes=29).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True)
    frontend = BatchSpectrogram(device=DEV, scale=waveform_scale(train_t), noise=waveform_noise(train_t))
    trainer = Trainer(model, opt, device=DEV, max_norm=400, frontend=frontend)
    batch = next(iter(loader))
    assert (batch[0].noise is not None) == (noise_block is not None)
    return float(trainer.update(batch))


def test_one_training_step_with_the_config_block(tmp_path, noise_dir):
    _corpus(tmp_path, [16000, 21000, 18500])
    block = {'path': noise_dir[0], 'noise_levels': [0.3, 0.5], 'prob': 1.0}
    with_noise, again, without = _one_step(tmp_path, block), _one_step(tmp_path, block), _one_step(tmp_path, None)
    print('one step: loss %.6f with noise, %.6f again, %.6f without' % (with_noise, again, without))
    assert np.isfinite(with_noise) and np.isfinite(without)
    assert with_noise == again
    assert with_noise != without
