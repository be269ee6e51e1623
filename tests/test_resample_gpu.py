"""Sample-rate conversion on the device (ds2_resample) against tests/resample_ref.py, by EQUALITY on exactly summable data
(integer taps in +-8, samples in +-64: every partial sum stays below 8 * 64 * 1023 < 2^24, so the float32 result is the
integer one in any order) at every ratio, tap count and clip length at which the kernel takes another path; isolated from its
neighbours in the flat buffer; the same bits wherever a clip stands; and the designed filters against float64 within the fp32
chain's own bound.  The float test prints its figures before it asserts (``pytest -s``).

One run on an MI355X (profiles/resample_errors.md): of 90 880 outputs per rate, 3 937 .. 19 530 lie inside the margin and
24 .. 69 differ from rint(v64), each by one unit and each inside the margin."""
import numpy as np
import pytest
import torch

from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -21846                      # 0xAAAA: what the output buffer holds before a launch

RATIOS = [(1, 1), (2, 1), (1, 2), (1, 3), (2, 3), (3, 2), (160, 441), (640, 441), (1, 6)]
TAP_COUNTS = [1, 3, 5, 53, 141, 305, 1023]


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops
    return ops


def _int_taps(L, K, rng):
    """Integer taps in +-8, none of them zero: a leaked neighbour of +-32767 always changes the sum."""
    return (rng.randint(1, 9, size=(L, K)) * rng.choice([-1, 1], size=(L, K))).astype(np.float32)


def _int_clip(n_frames, channels, rng):
    return rng.randint(-64, 65, size=n_frames * channels).astype(np.int16)


def _len_for(target, L, M):
    """The shortest clip with at least ``target`` outputs."""
    n = target * M // L
    while ref.out_len(n, L, M) < target:
        n += 1
    return n


def _lengths(tile, L, M, K):
    ns = [0, 1, 2, M - 1, M, M + 1, (K - 1) // 2, K - 1] + [_len_for(x, L, M) for x in (tile - 1, tile, tile + 1, 2 * tile + 3)]
    return [n for n in ns if n >= 0]


def _raw(pcm, in_off, channels, L, M, taps_d, out, out_off):
    """One launch through the C ABI, nothing in between."""
    from ds2hip import lib, ops
    bsz = len(in_off) - 1
    meta = ops.upload_small(torch.from_numpy(np.concatenate([np.asarray(in_off, np.int64), np.asarray(out_off, np.int64)])), DEV)
    lib.call('ds2_resample', pcm, meta[:bsz + 1], bsz, channels, L, M, taps_d, int(taps_d.shape[1]), out, meta[bsz + 1:])


def _carved(clips, channels, L, M, taps, lead=3, fill=32767, seed=0):
    """The interleaved int16 ``clips`` carved out of a flat buffer whose other elements are +-``fill``: ``lead`` of them in
    front, 8 behind, and between any two clips a filler of two or three frames (so odd and even element offsets both occur).
    The ABI's clips stand back to back, so the fillers are clips of the batch too; their outputs go behind everyone else's.
    The clips' outputs stand in a buffer of SENTINEL with one to three elements between them.  ONE launch.
    Returns (outputs per clip, the whole output buffer, [(start, end) of every clip's output])."""
    rng = np.random.RandomState(seed + len(clips))
    parts, in_off, kinds, pos = [rng.choice([-1, 1], size=lead) * fill], [lead], [], lead
    for i, c in enumerate(clips):
        f = rng.choice([-1, 1], size=channels * (2 + (i & 1))) * fill
        for kind, a in (('fill', f), ('clip', np.asarray(c))):
            parts.append(a)
            pos += len(a)
            in_off.append(pos)
            kinds.append(kind)
    parts.append(rng.choice([-1, 1], size=8) * fill)
    flat = np.concatenate(parts).astype(np.int16)
    out_off, spans, pos = [0] * len(kinds), [], 1
    for b, kind in enumerate(kinds):
        if kind == 'clip':
            n_out = ref.out_len((in_off[b + 1] - in_off[b]) // channels, L, M)
            out_off[b] = pos
            spans.append((pos, pos + n_out))
            pos += n_out + 1 + (b % 3)
    junk = pos
    for b, kind in enumerate(kinds):
        if kind == 'fill':
            out_off[b] = pos
            pos += ref.out_len((in_off[b + 1] - in_off[b]) // channels, L, M)
    pcm = torch.from_numpy(flat).to(DEV)
    out = torch.full((pos + 8,), SENTINEL, dtype=torch.int16, device=DEV)
    taps_d = torch.from_numpy(np.ascontiguousarray(taps, np.float32)).to(DEV)
    _raw(pcm, in_off, channels, L, M, taps_d, out, out_off)
    assert np.array_equal(pcm.cpu().numpy(), flat)                                    # the input is not written
    whole = out.cpu().numpy()
    keep = np.ones(junk, bool)
    for a, e in spans:
        keep[a:e] = False
    assert (whole[:junk][keep] == SENTINEL).all(), 'an element outside every clip was written'
    assert (whole[pos:] == SENTINEL).all(), 'an element behind the last output was written'
    return [whole[a:e] for a, e in spans], whole, spans


def _check_exact(clips, channels, L, M, taps, **kw):
    outs, _, _ = _carved(clips, channels, L, M, taps, **kw)
    for c, got in zip(clips, outs):
        want = ref.resample(c, channels, L, M, taps)
        assert len(got) == len(want)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, 'L %d M %d K %d n %d: %d outputs differ, first at %d: %d != %d' % (
            L, M, taps.shape[1], len(c) // channels, bad.size, bad[0], got[bad[0]], want[bad[0]])
    return outs


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('ratio', RATIOS, ids=lambda r: '%d_%d' % r)
def test_integer_data_is_exact_at_every_ratio_tap_count_and_length(ops, ratio):
    """Every K of the list at this ratio, one launch each over clips of every length of the list, carved out of +-32767."""
    L, M = ratio
    rng = np.random.RandomState(1000 * L + M)
    for K in TAP_COUNTS:
        taps = _int_taps(L, K, rng)
        clips = [_int_clip(n, 1, rng) for n in _lengths(ops.RESAMPLE_TILE, L, M, K)]
        _check_exact(clips, 1, L, M, taps, seed=K)


@pytest.mark.parametrize('ratio,K', [((1, 12), 1023), ((1, 12), 5), ((3, 4096), 1023), ((1024, 4095), 3), ((1024, 1), 7)],
                         ids=lambda v: str(v).replace(', ', '_'))
def test_ratios_whose_tile_is_staged_in_several_passes_and_the_limits(ops, ratio, K):
    """Past M / L of about 7 the input span of a 1024-output tile no longer fits the staging buffer and a tile is produced in
    passes (down to two outputs per pass at 3 / 4096 with 1023 taps); 1024 and 4095 / 4096 are the limits of L and M."""
    L, M = ratio
    rng = np.random.RandomState(L + M + K)
    taps = _int_taps(L, K, rng)
    t = ops.RESAMPLE_TILE
    clips = [_int_clip(n, 2, rng) for n in (1, M + 1, _len_for(t - 1, L, M), _len_for(t + 1, L, M), _len_for(2 * t + 3, L, M))]
    _check_exact(clips, 2, L, M, taps * 2, seed=K)           # (even taps: the halved stereo sum stays an integer)


def test_identity_copies_bit_for_bit(ops):
    rng = np.random.RandomState(5)
    x = rng.randint(-32768, 32768, size=5000).astype(np.int16)
    x[:4] = [-32768, 32767, 0, -1]
    outs, _, _ = _carved([x, x[:1], x[:0]], 1, 1, 1, np.ones((1, 1), np.float32))
    assert np.array_equal(outs[0], x) and np.array_equal(outs[1], x[:1]) and len(outs[2]) == 0


@pytest.mark.parametrize('channels', [1, 2, 3, 8])
def test_downmix_rounds_halves_to_even(ops, channels):
    """taps = [1]: the output is the channel mean, one rounded multiply by float(1 / C).  Odd sums of two channels (and sums
    of eight that are 4 mod 8) are halves: they go to the even neighbour, below zero too."""
    rng = np.random.RandomState(channels)
    frames = rng.randint(-32768, 32768, size=(4000, channels)).astype(np.int16)
    if channels in (2, 8):
        for i, s in enumerate([1, 3, 5, -1, -3, -5, 7, -7, 65533, -65533, 65531, -65531]):
            frames[i, :channels // 2] = s // 2                                   # the channels sum to s * C / 2: the mean is
            frames[i, channels // 2:] = s - s // 2                               # s / 2, a half
    frames[-1], frames[-2] = 32767, -32768
    clip = frames.reshape(-1)
    outs = _check_exact([clip, clip[:channels], clip[:7 * channels]], channels, 1, 1, np.ones((1, 1), np.float32))
    if channels in (2, 8):
        assert outs[0][:12].tolist() == [0, 2, 2, 0, -2, -2, 4, -4, 32766, -32766, 32766, -32766]
    assert outs[0][-1] == 32767 and outs[0][-2] == -32768


def test_saturation_at_both_ends(ops):
    taps = np.array([[2, 4, 2]], np.float32)
    x = np.concatenate([np.full(40, 32767), np.full(40, -32767), [-32768] * 8, [100, -100, 5000, -5000]]).astype(np.int16)
    outs = _check_exact([x], 1, 1, 1, taps)
    assert outs[0][10] == 32767 and outs[0][60] == -32768 and outs[0][84] == -32768


# ------------------------------------------------------------------------------------------------ int64 positions
def _check_windows(pcm, n, L, M, taps, out, starts, width):
    h = (taps.shape[1] - 1) // 2
    for a in starts:
        ms = np.arange(a, min(a + width, len(out)), dtype=np.int64)
        lo = max(int(ms[0]) * M // L - h, 0)
        hi = min(int(ms[-1]) * M // L + h + 1, n)
        s = pcm[lo:hi].cpu().numpy().astype(np.float64)
        want = ref.quantise(ref.convolve(s, L, M, taps, ms=ms, origin=lo, n=n))[0]
        got = out[int(ms[0]):int(ms[-1]) + 1].cpu().numpy()
        assert np.array_equal(got, want), 'outputs from %d differ' % a


def test_positions_past_2_to_the_31_at_160_441(ops):
    """14.2 M frames at 160 / 441: t = m M reaches 2.27e9 > 2^31 in the last 5 % of the clip (28 MB of input)."""
    L, M, K = 160, 441, 5
    n = 14200000
    rng = np.random.RandomState(31)
    taps = _int_taps(L, K, rng)
    g = torch.Generator(device=DEV).manual_seed(31)
    pcm = torch.randint(-64, 65, (n,), dtype=torch.int16, device=DEV, generator=g)
    out, off = ops.resample(pcm, [0, n], 44100, taps=(L, M, taps))
    assert off == [0, ref.out_len(n, L, M)] and off[1] * M > 2 ** 31
    first_past = 2 ** 31 // M
    _check_windows(pcm, n, L, M, taps, out, [0, first_past - 1500, first_past - 3, first_past + 70000, off[1] - 3000], 3000)


def test_one_clip_of_400_million_samples_at_1_6(ops):
    """0.8 GB of input in one clip (skipped where the device has not that much to spare): 65 105 tiles, element offsets
    past 2^28 (byte offsets past 2^29), a sample of the outputs against the reference.  Its positions t = m M stay below
    2^31 (L = 1: t is the input index); the case that passes 2^31 is the one above."""
    n = 400 * 1000 * 1000
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * (2 * n):
        pytest.skip('needs %.1f GB of free device memory' % (3 * 2 * n / 1e9))
    L, M, K = 1, 6, 5
    rng = np.random.RandomState(6)
    taps = _int_taps(L, K, rng)
    g = torch.Generator(device=DEV).manual_seed(6)
    pcm = torch.randint(-64, 65, (n,), dtype=torch.int16, device=DEV, generator=g)
    out, off = ops.resample(pcm, [0, n], 96000, taps=(L, M, taps))
    assert off == [0, ref.out_len(n, L, M)]
    starts = [0, 2 ** 24 - 1000, 2 ** 25 + 12345, 2 ** 28 // M - 1000, 60000000, off[1] - 2000]
    _check_windows(pcm, n, L, M, taps, out, starts, 2000)
    del pcm, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ placement
def test_a_clip_has_the_same_bits_wherever_it_stands(ops):
    """Alone, first, last and in the middle of a batch, at odd and even element offsets, and among 65534 clips of one or two
    samples (one workgroup column then walks all of its tiles): always the bits of B = 1."""
    L, M, K = 160, 441, 141
    rng = np.random.RandomState(77)
    taps = _int_taps(L, K, rng)
    clip = _int_clip(_len_for(3 * ops.RESAMPLE_TILE + 17, L, M), 1, rng)
    other = [_int_clip(n, 1, rng) for n in (700, 1, 12000, 0, 3001)]
    want = ref.resample(clip, 1, L, M, taps)
    alone = _check_exact([clip], 1, L, M, taps, lead=0)[0]
    assert np.array_equal(alone, want)
    for lead, order in ((1, [clip] + other), (2, other + [clip]), (5, other[:2] + [clip] + other[2:]), (4, [clip, clip])):
        outs, _, _ = _carved(order, 1, L, M, taps, lead=lead)
        for c, got in zip(order, outs):
            if c is clip:
                assert np.array_equal(got, want), 'lead %d' % lead
    # B = 65535: the clip behind 30000 tiny ones and in front of 35534, through the wrapper
    tiny = rng.randint(-64, 65, size=98304).astype(np.int16)
    lens = np.ones(65535, np.int64)
    lens[::3] = 2
    lens[30000] = len(clip)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = np.resize(tiny, off[-1])
    flat[off[30000]:off[30001]] = clip
    out, out_off = ops.resample(torch.from_numpy(flat).to(DEV), off.tolist(), 44100, taps=(L, M, taps))
    got = out.cpu().numpy()
    assert np.array_equal(got[out_off[30000]:out_off[30001]], want)
    want_all, want_off = ref.resample_flat(flat[:off[200]], off[:201], 1, L, M, taps)
    assert np.array_equal(got[:out_off[200]], want_all) and out_off[:201] == want_off.tolist()
    assert out_off[-1] == sum(ref.out_len(int(v), L, M) for v in lens)


# ------------------------------------------------------------------------------------------------ designed filters
def _speech_like(n, rng):
    """Seeded int16 noise with a speech-like spectrum and envelope (a two-pole low-pass under a slow modulation)."""
    e = rng.randn(n)
    x = np.zeros(n)
    a1, a2 = 1.6, -0.68
    for i in range(2, n):
        x[i] = e[i] + a1 * x[i - 1] + a2 * x[i - 2]
    env = 0.55 + 0.45 * np.sin(2 * np.pi * np.arange(n) / n * 3.3 + rng.rand() * 6)
    x = x / np.abs(x).max() * env * 30000
    return np.rint(x).astype(np.int16)


@pytest.mark.parametrize('rate', ref.RATES)
def test_design_taps_against_float64(ops, rate):
    """Clips of about a second, mixed lengths, mono and stereo, through resample_design's table.  v64: the float64 sum over
    the SAME float32 taps, divided by C.  |out - rint(v64)| <= 1 everywhere; out == rint(v64) wherever v64 is farther from a
    rounding boundary than (K + 2) 2^-24 sum |taps s| / C: K fused multiply-adds, the rounding of 1 / C and the multiply, each
    at most half an ulp of a magnitude that sum bounds -- the fp32 chain's own bound."""
    L, M, taps = ops.resample_design(rate)
    rL, rM, rtaps = ref.design(rate)
    assert (L, M) == (rL, rM) and np.array_equal(taps, rtaps)
    K = taps.shape[1]
    rng = np.random.RandomState(rate)
    near = differ = total = 0
    worst = 0
    for channels in (1, 2):
        clips = [_speech_like(int(rate * sec) * channels, rng) for sec in (0.71, 1.0, 1.13)]
        off = np.concatenate([[0], np.cumsum([len(c) for c in clips])])
        out, out_off = ops.resample(torch.from_numpy(np.concatenate(clips)).to(DEV), off.tolist(), rate, channels=channels)
        got_all = out.cpu().numpy()
        for b, c in enumerate(clips):
            s = ref.downmix(c, channels)
            want, v = ref.quantise(ref.convolve(s, L, M, taps), channels)
            margin = (K + 2) * 2.0 ** -24 * ref.convolve(s, L, M, taps, absolute=True) / channels
            got = got_all[out_off[b]:out_off[b + 1]]
            assert len(got) == len(want) == ref.out_len(len(s), L, M)
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            clear = np.abs(v - np.floor(v) - 0.5) > margin                      # (distance to the nearest k + 1/2)
            inside = (v > -32768.5 + margin) & (v < 32767.5 - margin)
            near += int((~clear).sum())
            differ += int((d != 0).sum())
            total += len(got)
            worst = max(worst, int(d.max()))
            print('resample %6d Hz C=%d n=%7d: outputs %6d, inside the margin %4d, differ %3d, max |diff| %d, largest margin %.2e'
                  % (rate, channels, len(s), len(got), int((~clear).sum()), int((d != 0).sum()), int(d.max()), margin.max()))
            assert d.max() <= 1
            assert (d[clear & inside] == 0).all()
    print('resample %6d Hz total: outputs %d, inside the margin %d, differ %d, max |diff| %d' % (rate, total, near, differ, worst))


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_written(ops):
    from ds2hip import lib
    pcm = torch.randint(-64, 65, (4096,), dtype=torch.int16, device=DEV)
    out = torch.full((8192,), SENTINEL, dtype=torch.int16, device=DEV)
    one = torch.ones((4, 4), dtype=torch.float32, device=DEV)
    cases = [dict(K=2), dict(K=0), dict(K=1025), dict(L=0), dict(L=1025), dict(M=0), dict(M=4097), dict(channels=9),
             dict(channels=0), dict(channels=3, off=[0, 300, 1000]), dict(off=[0, 600, 500]), dict(B=0)]
    for kw in cases:
        off = kw.get('off', [0, 1000, 4096])
        bsz = kw.get('B', len(off) - 1)
        meta = ops.upload_small(torch.tensor(off + [0, 4096], dtype=torch.int64), DEV)
        with pytest.raises(lib.Ds2Error) as err:
            lib.call('ds2_resample', pcm, meta[:len(off)], bsz, kw.get('channels', 1), kw.get('L', 1), kw.get('M', 1),
                     one, kw.get('K', 3), out, meta[len(off):])
        assert err.value.code == lib.ERR_ARG, kw
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), kw
    assert lib.query('ds2_resample_out_len', 0, 160, 441) == 0 and lib.query('ds2_resample_out_len', 441, 160, 441) == 160
    assert lib.query('ds2_resample_out_len', 442, 160, 441) == 161
    assert lib.query('ds2_resample_out_len', 158760000 * 2, 160, 441) == 115200000     # two hours: n L passes 2^32
    # the wrapper refuses the same by name, before any launch
    for bad in (dict(channels=9), dict(channels=3), dict(taps=(1, 1, np.ones((1, 2), np.float32))),
                dict(taps=(0, 1, np.ones((0, 3), np.float32)))):
        with pytest.raises(ValueError, match='resample'):
            ops.resample(pcm[:1000], [0, 1000], 48000, **bad)
    with pytest.raises(ValueError, match='44056'):
        ops.resample(pcm, [0, 4096], 44056)
    with pytest.raises(RuntimeError):
        ops.resample(pcm.cpu(), [0, 4096], 48000)
