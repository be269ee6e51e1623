"""Reverberation on the device (ds2_reverb) against tests/reverb_ref.py: exact on integer data at every tile and pass edge,
isolated from its neighbours, the same bits wherever a clip stands, the level gain, float data against float64, and the
training frontend against the stages called by hand.

Float, one run on an MI355X (profiles/reverb_errors.md): the hard bound (m + 1) 2^-24 S[n] is used to at most 0.16; the
rms of err / S is 0.28 .. 0.84 of the float32 tap-order chain's on the CPU (the assertion allows 4).  Every float test
prints its figures before it asserts (``pytest -s``)."""
import os

import numpy as np
import pytest
import torch

from tests import reverb_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = {'unit': 1.0 / 32768.0, 'int32': 65536.0}


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ops, clips, rirs, keep_level, lead=0, trail=0, outside=np.nan, bank_gap=0, bank_fill=np.nan, ws=None,
         sentinel=None):
    """clips: list of float32 arrays; rirs: list of float32 arrays or None (no draw).  Lays the clips out behind ``lead``
    samples of ``outside`` and the RIRs ``bank_gap`` + (odd) taps of ``bank_fill`` apart, runs one launch and returns
    (outs per clip, gains, whole out buffer, offsets)."""
    offs = [lead]
    for c in clips:
        offs.append(offs[-1] + len(c))
    flat = np.full(offs[-1] + trail, outside, np.float32)
    for c, o in zip(clips, offs):
        flat[o:o + len(c)] = c
    parts, lo, ln, pos = [np.full(bank_gap | 1, bank_fill, np.float32)], [], [], bank_gap | 1
    for h in rirs:
        if h is None:
            lo.append(0), ln.append(0)
            continue
        lo.append(pos), ln.append(len(h))
        parts += [np.asarray(h, np.float32), np.full(bank_gap + 1, bank_fill, np.float32)]
        pos += len(h) + bank_gap + 1
        if bank_gap and pos % 2 == 0:                                   # keep rir_lo odd
            parts.append(np.full(1, bank_fill, np.float32))
            pos += 1
    bank = torch.from_numpy(np.concatenate(parts)).to(DEV)
    wav = torch.from_numpy(flat).to(DEV)
    out = None if sentinel is None else torch.full_like(wav, sentinel)
    res, gain = ops.reverb(wav, offs, bank, lo, ln, keep_level, out=out, return_gain=True, ws=ws)
    assert torch.equal(wav.cpu().view(torch.int32), torch.from_numpy(flat).view(torch.int32))      # the input is not written
    whole = res.cpu().numpy()
    return [whole[offs[b]:offs[b + 1]] for b in range(len(clips))], gain.cpu().numpy(), whole, offs


# ------------------------------------------------------------------------------------------------ exact
def _lengths(ops):
    t = ops.REVERB_TILE
    return [1, 15, 16, 17, t - 1, t, t + 1, 2 * t + 7]


def _tap_groups(ops):
    s = ops.REVERB_TAPS_STEP
    return [[1, 2, 3], [4, 5, 15], [16, 17, s - 1], [s, s + 1, 2 * s + 3], [8000]]


def _int_clip(n, rng):
    return rng.randint(-64, 65, size=n).astype(np.float32)


def _int_rir(k, rng):
    h = rng.randint(-8, 9, size=k).astype(np.float32)
    h[0], h[-1] = rng.choice([-8, -3, 1, 8]), rng.choice([-5, 2, 7])    # neither end is zero (K is what it says)
    return h


@pytest.mark.parametrize('group', range(5))
def test_integer_data_is_exact_at_every_edge(ops, group):
    """Clips in +-64 and taps in +-8: every partial sum stays below 64 * 8 * 8000 < 2^24, so the float32 result equals the
    integer one in ANY summation order."""
    rng = np.random.RandomState(100 + group)
    taps = _tap_groups(ops)[group]
    clips, rirs = [], []
    for k in taps:
        for n in _lengths(ops):
            clips.append(_int_clip(n, rng)), rirs.append(_int_rir(k, rng))
    for at, n in ((3, 40), (11, 0), (17, ops.REVERB_TILE + 5), (len(clips), 0)):       # undrawn and empty clips mixed in
        clips.insert(at, _int_clip(n, rng)), rirs.insert(at, None)
    clips.insert(7, _int_clip(0, rng)), rirs.insert(7, _int_rir(taps[0], rng))         # an EMPTY clip with a draw
    assert len(clips) <= 32 and any(len(h) > len(c) for c, h in zip(clips, rirs) if h is not None)
    outs, gains, _, _ = _run(ops, clips, rirs, keep_level=False, lead=group)
    for b, (c, h, y) in enumerate(zip(clips, rirs, outs)):
        want = c if h is None else ref.conv_direct(c, h).astype(np.float32)
        assert np.array_equal(y, want), (b, len(c), None if h is None else len(h))
        assert gains[b] == 1.0


def test_isolation_from_neighbours_bank_and_untouched_samples(ops):
    t, s = ops.REVERB_TILE, ops.REVERB_TAPS_STEP
    rng = np.random.RandomState(7)
    nan_clip = np.full(300, np.nan, np.float32)
    odd = np.array([0x80000000, 0x7fc00001, 0xffc12345, 0x7f800000, 0x00000001, 0x7fa00000], np.uint32).view(np.float32)
    clips = [_int_clip(t + 9, rng), nan_clip, _int_clip(2 * t + 7, rng), odd, _int_clip(17, rng), _int_clip(0, rng),
             nan_clip.copy(), _int_clip(s + 40, rng)]
    rirs = [_int_rir(s + 1, rng), None, _int_rir(8000, rng), None, _int_rir(40, rng), None, None, _int_rir(2 * s + 3, rng)]
    sentinel = -12345.5
    outs, gains, whole, offs = _run(ops, clips, rirs, keep_level=False, lead=5, trail=77, bank_gap=24, sentinel=sentinel)
    assert offs[0] % 2 == 1
    for b, (c, h, y) in enumerate(zip(clips, rirs, outs)):
        if h is None:
            assert np.array_equal(_bits(y), _bits(c)), b                # bit for bit: -0.0 and NaN payloads included
        else:
            assert np.all(np.isfinite(y)), b                            # no NaN next door reached a product
            assert np.array_equal(y, ref.conv_direct(c, h).astype(np.float32)), b
    assert np.all(gains == 1.0)
    assert np.all(whole[:offs[0]] == np.float32(sentinel)) and np.all(whole[offs[-1]:] == np.float32(sentinel))
    assert len(whole) == offs[-1] + 77
    # keep_level on the same layout: the NaN neighbours do not reach the energy sums either
    outs, gains, whole, _ = _run(ops, clips, rirs, keep_level=True, lead=5, trail=77, bank_gap=24, sentinel=sentinel)
    assert all(np.all(np.isfinite(y)) for y, h in zip(outs, rirs) if h is not None) and np.all(np.isfinite(gains))
    assert np.all(whole[:offs[0]] == np.float32(sentinel)) and np.all(whole[offs[-1]:] == np.float32(sentinel))
    assert np.array_equal(_bits(outs[3]), _bits(odd)) and gains[3] == 1.0


# ------------------------------------------------------------------------------------------------ bits
def test_bits_do_not_depend_on_position_company_alignment_or_workspace(ops):
    from ds2hip import lib
    t, s = ops.REVERB_TILE, ops.REVERB_TAPS_STEP
    clip = ref.speech_like(2 * t + 7, 1)
    h = ref.synth_rir_taps(s + 1, 0.05, 2)
    rng = np.random.RandomState(3)
    others = [ref.speech_like(n, 10 + i) for i, n in enumerate((900, 3 * t + 1, 33))]
    other_h = [ref.synth_rir_taps(77, 0.01, 5), None, ref.synth_rir_taps(8000, 0.4, 6)]
    runs = {}
    for keep in (False, True):
        alone = _run(ops, [clip], [h], keep)
        moved = _run(ops, others + [clip, _int_clip(500, rng)], other_h + [h, ref.synth_rir_taps(9, 0.01, 8)], keep,
                     lead=3, trail=2, bank_gap=10)
        need = lib.query('ds2_reverb_ws_bytes', 1, len(clip))
        dirty = _run(ops, [clip], [h], keep, ws=torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV))
        large = _run(ops, [clip], [h], keep, ws=torch.full((2 * need,), 0xFF, dtype=torch.uint8, device=DEV))
        y, g = alone[0][0], alone[1][0]
        for name, (outs, gains, _, _), at in (('moved', moved, 3), ('dirty ws', dirty, 0), ('large ws', large, 0)):
            assert np.array_equal(_bits(outs[at]), _bits(y)), (keep, name)
            assert _bits(gains[at:at + 1])[0] == _bits([g])[0], (keep, name)
        runs[keep] = (y, g)
    (y0, g0), (y1, g1) = runs[False], runs[True]
    assert g0 == 1.0 and g1 != 1.0
    assert np.array_equal(_bits(y1), _bits(np.float32(g1) * y0))        # the scaled run convolved to the same unscaled y
    with pytest.raises(ValueError, match='workspace'):
        _run(ops, [clip], [h], True, ws=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))


def test_vector_alu_form_is_the_same_sum(ops, monkeypatch):
    """DS2_REVERB_FORM=valu (the timing baseline, read at every call): exact on integer data, and on finite float data the
    bits of the matrix form -- both add an output's taps from the last one down to h[0] in one fma chain."""
    t, s = ops.REVERB_TILE, ops.REVERB_TAPS_STEP
    rng = np.random.RandomState(9)
    lens = [1, 17, t - 1, t + 1, 2 * t + 7, 300]
    taps = [1, 5, s, s + 1, 2 * s + 3, 8000]
    clips = [_int_clip(n, rng) for n in lens] + [_int_clip(50, rng)]
    rirs = [_int_rir(k, rng) for k in taps] + [None]
    fclips = [ref.speech_like(n, 90 + i) for i, n in enumerate((2 * t + 7, 700))]
    frirs = [ref.synth_rir_taps(s + 9, 0.05, 3), ref.synth_rir_taps(8000, 0.4, 4)]
    mfma = _run(ops, fclips, frirs, True, lead=1)
    monkeypatch.setenv('DS2_REVERB_FORM', 'valu')
    outs, gains, _, _ = _run(ops, clips, rirs, keep_level=False, lead=3)
    valu = _run(ops, fclips, frirs, True, lead=1)
    monkeypatch.delenv('DS2_REVERB_FORM')
    for b, (c, h, y) in enumerate(zip(clips, rirs, outs)):
        want = c if h is None else ref.conv_direct(c, h).astype(np.float32)
        assert np.array_equal(y, want) and gains[b] == 1.0, b
    for b in range(2):
        assert np.array_equal(_bits(valu[0][b]), _bits(mfma[0][b])), b
    assert np.array_equal(_bits(valu[1]), _bits(mfma[1]))


# ------------------------------------------------------------------------------------------------ level
def test_level_gain_and_the_single_multiply(ops):
    t = ops.REVERB_TILE
    clips = [ref.speech_like(n, 20 + i, sc) for i, (n, sc) in enumerate(
        ((2 * t + 7, SCALES['unit']), (t, SCALES['int32']), (700, SCALES['unit']), (5 * t + 3, SCALES['int32'])))]
    clips += [np.zeros(t + 3, np.float32), ref.speech_like(300, 30)]
    rirs = [ref.synth_rir_taps(k, rt, 40 + i) for i, (k, rt) in enumerate(((800, 0.1), (8000, 0.5), (3, 0.01), (2000, 0.2)))]
    rirs += [ref.synth_rir_taps(100, 0.05, 50), None]
    y, g0, _, _ = _run(ops, clips, rirs, keep_level=False)
    out, gain, _, _ = _run(ops, clips, rirs, keep_level=True)
    assert np.all(g0 == 1.0)
    for b in range(4):
        g64 = ref.gain_ref(clips[b], y[b])                              # float64, from the kernel's own y
        rel = abs(float(gain[b]) - g64) / g64
        print('clip %d: gain %.9g, float64 %.12g, off by %.3f of 2^-24' % (b, gain[b], g64, rel * 2.0 ** 24))
        assert rel <= 1.001 * 2.0 ** -24
        assert gain[b] != 1.0 and 0.1 < gain[b] < 10.0
        assert np.array_equal(_bits(out[b]), _bits(np.float32(gain[b]) * y[b]))
        ey = float(np.dot(out[b].astype(np.float64), out[b].astype(np.float64)))
        ex = float(np.dot(clips[b].astype(np.float64), clips[b].astype(np.float64)))
        assert ey == pytest.approx(ex, rel=1e-6)                        # which is what the stage is for
    assert gain[4] == 1.0 and not np.any(out[4]) and not np.any(y[4])   # a drawn all-zero clip
    assert gain[5] == 1.0 and np.array_equal(_bits(out[5]), _bits(clips[5]))


# ------------------------------------------------------------------------------------------------ float against float64
FLOAT_CASES = [(800, 'short', 'unit'), (800, 'short', 'int32'), (8000, 'short', 'unit'), (8000, 'short', 'int32'),
               (8000, 'long', 'unit')]


@pytest.mark.parametrize('k,length,scale', FLOAT_CASES)
def test_float_data_against_float64(ops, k, length, scale):
    n = 2 * ops.REVERB_TILE + 7 if length == 'short' else 240000
    x = ref.speech_like(n, k + n % 97, SCALES[scale])
    h = ref.synth_rir_taps(k, 0.3 if k == 800 else 0.5, k)
    (y,), _, _, _ = _run(ops, [x], [h], keep_level=False)
    y64, s = ref.conv_ref(x, h), ref.abs_sum(x, h)
    m = np.minimum(np.arange(n) + 1, k)
    err = np.abs(y.astype(np.float64) - y64)
    live = s > 0
    assert np.all(err[~live] == 0)
    used = float(np.max(err[live] / ((m[live] + 1) * 2.0 ** -24 * s[live])))
    chain = np.abs(ref.chain32(x, h).astype(np.float64) - y64)          # the yardstick: computed here, never from the kernel
    rms = lambda e: float(np.sqrt(np.mean((e[live] / s[live]) ** 2)))   # noqa: E731
    ratio = rms(err) / rms(chain)
    print('reverb K=%d N=%d %s WORST: %.4f of the hard bound; rms err/S %.3e, float32 chain %.3e, ratio %.3f'
          % (k, n, scale, used, rms(err), rms(chain), ratio))
    assert used <= 1.001
    assert ratio <= 4.0


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture()
def banks(tmp_path):
    import importlib.util

    from tests.noise_ref import write_noise_dir
    spec = importlib.util.spec_from_file_location('ds2_make_rir', os.path.join(ROOT, 'tools', 'make_rir.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.write_set(str(tmp_path / 'rirs'), rt60s=(0.05, 0.2), count=2, seed=1)
    write_noise_dir(str(tmp_path / 'noise'))
    return str(tmp_path / 'rirs'), str(tmp_path / 'noise')


def _pcm(n, seed):
    return (np.random.RandomState(seed).standard_normal(n) * 3000).astype(np.int16)


def test_frontend_equals_the_stages_called_by_hand(ops, banks):
    from codes.transforms import BatchSpectrogram, NoiseInjection, PCMClip, RawAudioBatch, Reverb
    rv, nz = Reverb(banks[0], prob=1.0), NoiseInjection(banks[1], prob=1.0)
    rdraws = [1, None, 3, 0]
    ndraws = [(0, 0.3, 0.2), (1, 0.2, 0.7), None, (2, 0.4, 0.1)]
    clips = [PCMClip(torch.from_numpy(_pcm(n, 70 + i)), 1.0 + 0.03 * i, 1.5 - i, ndraws[i], None, rdraws[i])
             for i, n in enumerate((16000, 9000, 12345, 20000))]
    batch = RawAudioBatch.from_clips(clips)
    assert batch.reverb == rdraws and batch.noise == ndraws
    front = BatchSpectrogram(reverb=rv, noise=nz)
    inputs, pct = front(batch.to(DEV))
    # by hand
    flat, offs = ops.decode_augment(batch.pcm.to(DEV), batch.offsets, batch.tempos, batch.gains_db, scale=front.scale)
    dry = flat.clone()
    lo, ln = rv.params(rdraws)
    wet, gain = ops.reverb(flat, offs, rv.bank(DEV), lo, ln, True, return_gain=True)
    assert torch.equal(flat, dry) and wet.data_ptr() != flat.data_ptr()
    for b, d in enumerate(rdraws):
        same = torch.equal(wet[offs[b]:offs[b + 1]], dry[offs[b]:offs[b + 1]])
        assert same == (d is None) and (float(gain[b]) == 1.0) == (d is None)
    lens = [offs[i + 1] - offs[i] for i in range(4)]
    nlo, nln, nst, nlv = nz.params(ndraws, lens)
    mixed = ops.noise_mix(wet, offs, nz.bank(DEV), nlo, nln, nst, nlv, front.scale, out=wet)
    frames = [1 + n // 160 for n in lens]
    want = ops.spectrogram(mixed, torch.tensor(offs, dtype=torch.int64), max(frames), True, 1e-9)
    assert torch.equal(inputs, want)
    assert np.array_equal(pct.numpy(), np.asarray([f / float(max(frames)) for f in frames], np.float32))
    plain, _ = BatchSpectrogram(noise=nz)(RawAudioBatch.from_clips(
        [PCMClip(c.pcm, c.tempo, c.gain_db, c.noise) for c in clips]).to(DEV))
    assert torch.equal(plain[1], inputs[1]) and not torch.equal(plain[0], inputs[0])     # clip 1 drew no RIR
    # a batch that carries draws needs the bank; one without draws never touches it
    with pytest.raises(RuntimeError, match='RIR bank'):
        BatchSpectrogram(noise=nz)(batch.to(DEV))
    fresh = Reverb(banks[0])
    BatchSpectrogram(reverb=fresh)(RawAudioBatch.from_clips([PCMClip(clips[0].pcm, 1.05, 1.5)]).to(DEV))
    assert fresh._banks == {}


def test_per_clip_call_equals_the_batched_result(ops, banks):
    from codes.transforms import Reverb
    rv = Reverb(banks[0], prob=1.0)
    x = torch.from_numpy(_pcm(12000, 60).astype(np.float32) * np.float32(SCALES['unit']))
    np.random.seed(8)
    draw = rv.draw()
    np.random.seed(8)
    y = rv(x)
    assert y.device.type == 'cpu' and y.shape == x.shape and not torch.equal(y, x)
    other = torch.from_numpy(ref.speech_like(5000, 61))
    out = rv.apply_batch(torch.cat([other, x]).to(DEV), [0, 5000, 17000], [None, draw])
    assert torch.equal(out[5000:].cpu(), y) and torch.equal(out[:5000].cpu(), other)
    h = ref.rir_rule(_read16(rv.paths[draw]), rv.max_taps)
    assert torch.equal(rv.bank(DEV)[rv.starts[draw]:rv.starts[draw] + rv.lengths[draw]].cpu(), torch.from_numpy(h))
    y64 = ref.conv_ref(x.numpy(), h)
    want = y64 * np.sqrt(np.dot(x.numpy().astype(np.float64), x.numpy().astype(np.float64)) / np.dot(y64, y64))
    np.testing.assert_allclose(y.numpy(), want, rtol=0, atol=2e-5 * float(np.abs(want).max()))
    x_dev = x.to(DEV)
    np.random.seed(8)
    on_dev = rv(x_dev)                                                   # a device tensor stays there, and x is not written
    assert on_dev.is_cuda and torch.equal(on_dev.cpu(), y) and torch.equal(x_dev.cpu(), x)
    assert Reverb(banks[0], prob=0.0)(x) is x


def _read16(path):
    import wave
    with wave.open(path, 'rb') as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
