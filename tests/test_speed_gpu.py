"""Speed perturbation on the device (ds2_resample_var), held by EQUALITY throughout: against tests/resample_ref.py on exactly
summable data (integer taps in +-8, samples in +-64: every partial sum stays below 8 * 64 * 1023 < 2^24, so the float32 result
is the integer one in any order, as tests/test_resample_gpu.py argues) in ONE launch that mixes LDS-resident tables with a
table on the cache path; against ds2_resample on every clip alone with the designed tables; wherever a clip stands; the
refusals; and the stage in BatchSpectrogram against the clips converted one at a time."""
import numpy as np
import pytest
import torch

from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -21846                      # 0xAAAA: what the output buffer holds before a launch

# (L, M, K): the identity's shape, the two default factors', both octaves', a table past the LDS capacity (53 000 floats) and
# the tap limit
SHAPES = [(1, 1, 1), (10, 9, 53), (10, 11, 57), (2, 1, 53), (1, 2, 103), (1000, 937, 53), (3, 2, 1023)]


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops
    return ops


def _int_taps(L, K, rng):
    """Integer taps in +-8, none of them zero: a leaked neighbour of +-32767 always changes the sum."""
    return (rng.randint(1, 9, size=(L, K)) * rng.choice([-1, 1], size=(L, K))).astype(np.float32)


def _len_for(target, L, M):
    """The shortest clip with at least ``target`` outputs."""
    n = target * M // L
    while n > 0 and ref.out_len(n - 1, L, M) >= target:
        n -= 1
    while ref.out_len(n, L, M) < target:
        n += 1
    return n


def _rw(table):
    """A designed table with a writable copy of its (read-only, cached) taps, as ops.resample uploads them."""
    return table[0], table[1], np.array(table[2])


def _bank(tables):
    """(device tap bank, (T, 4) int32 host description) of a list of (L, M, taps)."""
    desc, pos = [], 0
    for L, M, taps in tables:
        desc.append((L, M, taps.shape[1], pos))
        pos += taps.size
    bank = torch.from_numpy(np.concatenate([np.ascontiguousarray(t[2], np.float32).reshape(-1) for t in tables])).to(DEV)
    return bank, np.asarray(desc, np.int32).reshape(-1, 4)


def _raw(pcm, in_off, out_off, ids, desc, bank, max_out, out, n_tables=None, bank_floats=None, B=None):
    """One launch through the C ABI, nothing in between."""
    from ds2hip import lib, ops
    bsz = len(in_off) - 1
    ids_pad = np.zeros(2 * ((bsz + 1) // 2), np.int32)
    ids_pad[:bsz] = ids
    meta = ops.upload_small(torch.from_numpy(np.concatenate([np.asarray(in_off, np.int64), np.asarray(out_off, np.int64),
                                                             ids_pad.view(np.int64)])), DEV)
    a = bsz + 1
    lib.call('ds2_resample_var', pcm, meta[:a], meta[a:2 * a], meta[2 * a:].view(torch.int32), bsz if B is None else B,
             desc.ctypes.data, len(desc) if n_tables is None else n_tables, bank,
             int(bank.numel()) if bank_floats is None else bank_floats, int(max_out), out)


def _carved(clips, ids, tables, lead=3, fill=32767, seed=0, extra_out=0):
    """The int16 ``clips`` (clip i through table ``ids[i]``) carved out of a flat buffer whose other elements are +-``fill``:
    ``lead`` of them in front, 8 behind, and between any two clips a filler of two or three samples (so odd and even element
    offsets both occur).  The ABI's clips stand back to back, so the fillers are clips of the batch too (through table 0); their
    outputs go behind everyone else's.  The clips' outputs stand in a buffer of SENTINEL with one to three elements between
    them.  ONE launch, ``max_out`` = the longest output + ``extra_out``.  Returns the outputs per clip."""
    rng = np.random.RandomState(seed + len(clips))
    parts, in_off, kinds, tid, pos = [rng.choice([-1, 1], size=lead) * fill], [lead], [], [], lead
    for i, c in enumerate(clips):
        f = rng.choice([-1, 1], size=2 + (i & 1)) * fill
        for kind, a, t in (('fill', f, 0), ('clip', np.asarray(c), ids[i])):
            parts.append(a)
            pos += len(a)
            in_off.append(pos)
            kinds.append(kind)
            tid.append(t)
    parts.append(rng.choice([-1, 1], size=8) * fill)
    flat = np.concatenate(parts).astype(np.int16)
    n_outs = [ref.out_len(in_off[b + 1] - in_off[b], tables[tid[b]][0], tables[tid[b]][1]) for b in range(len(kinds))]
    out_off, spans, pos = [0] * (len(kinds) + 1), [], 1
    for b, kind in enumerate(kinds):
        if kind == 'clip':
            out_off[b] = pos
            spans.append((pos, pos + n_outs[b]))
            pos += n_outs[b] + 1 + (b % 3)
    junk = pos
    for b, kind in enumerate(kinds):
        if kind == 'fill':
            out_off[b] = pos
            pos += n_outs[b]
    out_off[-1] = pos                                                                # (the last entry is not read)
    pcm = torch.from_numpy(flat).to(DEV)
    out = torch.full((pos + 8,), SENTINEL, dtype=torch.int16, device=DEV)
    bank, desc = _bank(tables)
    _raw(pcm, in_off, out_off, tid, desc, bank, max(n_outs) + extra_out, out)
    assert np.array_equal(pcm.cpu().numpy(), flat)                                    # the input is not written
    whole = out.cpu().numpy()
    keep = np.ones(junk, bool)
    for a, e in spans:
        keep[a:e] = False
    assert (whole[:junk][keep] == SENTINEL).all(), 'an element outside every clip was written'
    assert (whole[pos:] == SENTINEL).all(), 'an element behind the last output was written'
    return [whole[a:e] for a, e in spans]


# ------------------------------------------------------------------------------------------------ exact
@pytest.fixture(scope='module')
def exact_case(ops):
    """Every table of SHAPES with clips of 0, 1, 2, K - 1 samples and the shortest clips with tile - 1, tile, tile + 1 and
    2 tile + 3 outputs, shuffled; the references computed once."""
    rng = np.random.RandomState(950)
    tile = ops.RESAMPLE_TILE
    tables = [(L, M, _int_taps(L, K, rng)) for L, M, K in SHAPES]
    clips, ids = [], []
    for t, (L, M, K) in enumerate(SHAPES):
        for n in [0, 1, 2, K - 1] + [_len_for(x, L, M) for x in (tile - 1, tile, tile + 1, 2 * tile + 3)]:
            clips.append(rng.randint(-64, 65, size=n).astype(np.int16))
            ids.append(t)
    order = rng.permutation(len(clips))
    clips, ids = [clips[i] for i in order], [ids[i] for i in order]
    want = [ref.resample(c, 1, tables[t][0], tables[t][1], tables[t][2]) for c, t in zip(clips, ids)]
    return tables, clips, ids, want


def test_one_launch_over_every_table_and_length_is_exact(ops, exact_case):
    tables, clips, ids, want = exact_case
    assert tables[5][0] * tables[5][2].shape[1] > 24576 >= max(t[0] * t[2].shape[1] for i, t in enumerate(tables) if i != 5)
    outs = _carved(clips, ids, tables)
    seen = set()
    for c, t, got, w in zip(clips, ids, outs, want):
        L, M, taps = tables[t]
        assert len(got) == len(w) == ref.out_len(len(c), L, M)
        bad = np.nonzero(got != w)[0]
        assert bad.size == 0, 'L %d M %d K %d n %d: %d outputs differ, first at %d: %d != %d' % (
            L, M, taps.shape[1], len(c), bad.size, bad[0], got[bad[0]], w[bad[0]])
        seen.add((t, len(got)))
    tile = ops.RESAMPLE_TILE
    for t, (L, M, K) in enumerate(SHAPES):              # (at 2 / 1 the outputs come in pairs: the first count at or past each)
        for x in (tile - 1, tile, tile + 1, 2 * tile + 3):
            assert any(s == t and x <= y <= x + (L - 1) // M for s, y in seen), (L, M, x)


def test_identity_table_copies_bit_for_bit(ops):
    rng = np.random.RandomState(5)
    x = rng.randint(-32768, 32768, size=5000).astype(np.int16)
    x[:4] = [-32768, 32767, 0, -1]
    one = (1, 1, np.ones((1, 1), np.float32))
    outs = _carved([x, x[:1], x[:0]], [0, 0, 0], [one])
    assert np.array_equal(outs[0], x) and np.array_equal(outs[1], x[:1]) and len(outs[2]) == 0
    out, off = ops.resample_var(torch.from_numpy(x).to(DEV), [0, 5000], [0], [one])
    assert off == [0, 5000] and np.array_equal(out.cpu().numpy(), x)


# ------------------------------------------------------------------------------------------------ the parent's kernel
FACTORS = (0.9, 1.0, 1.1, 0.937)


@pytest.fixture(scope='module')
def designed(ops):
    """Full-range random clips, every one through every designed table, and ds2_resample's bits for each clip ALONE."""
    rng = np.random.RandomState(11)
    tables = [ops.speed_design(f) for f in FACTORS]
    lens = [16001, 3001, 1, 0, 40000, 2 * ops.RESAMPLE_TILE + 3]
    clips, ids = [], []
    for n in lens:
        for t in range(len(tables)):
            clips.append(rng.randint(-32768, 32768, size=n).astype(np.int16))
            ids.append(t)
    alone = []
    for c, t in zip(clips, ids):
        if len(c) == 0:
            alone.append(np.zeros(0, np.int16))
            continue
        out, off = ops.resample(torch.from_numpy(c).to(DEV), [0, len(c)], 16000, taps=_rw(tables[t]))
        assert off == [0, ref.out_len(len(c), tables[t][0], tables[t][1])]
        alone.append(out.cpu().numpy())
    return tables, clips, ids, alone


def test_every_clip_has_the_bits_of_ds2_resample_on_that_clip_alone(ops, designed):
    tables, clips, ids, alone = designed
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).tolist()
    out, out_off = ops.resample_var(torch.from_numpy(np.concatenate(clips)).to(DEV), off, ids, tables)
    got = out.cpu().numpy()
    assert out_off[-1] == len(got) == sum(len(a) for a in alone)
    for b, (c, t, a) in enumerate(zip(clips, ids, alone)):
        mine = got[out_off[b]:out_off[b + 1]]
        assert len(mine) == len(a) and np.array_equal(mine, a), 'clip %d (factor %s, %d samples)' % (b, FACTORS[t], len(c))
        if FACTORS[t] == 1.0:
            assert np.array_equal(mine, c)                                            # the 1.0 clips equal their input
    assert any(len(a) > 0 and not np.array_equal(a[:10], c[:10]) for a, c, t in zip(alone, clips, ids) if FACTORS[t] != 1.0)


# ------------------------------------------------------------------------------------------------ placement
def test_a_clip_has_the_same_bits_wherever_it_stands(ops, designed):
    """At B = 1 and in a batch of 300, first and last, beside any other tables, with max_out exact or larger: always the bits
    of ds2_resample on the clip alone."""
    tables, clips, ids, alone = designed
    rng = np.random.RandomState(300)
    for b in (4, 19):                                   # 3001 samples at 0.9 (LDS taps), 40000 samples at 0.937 (cache path)
        clip, t, want = clips[b], ids[b], alone[b]
        for extra in (0, 1, 5000):                      # B = 1, its own table only; max_out exact and larger than needed
            got = _carved([clip], [0], [tables[t]], lead=extra & 1, extra_out=extra)[0]
            assert np.array_equal(got, want), (b, extra)
        got = _carved([clip, clip], [t, t], tables, lead=2)                          # beside every other table
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        # first and last of 300, the 298 between them short clips through tables drawn at random
        other = [rng.randint(-32768, 32768, size=int(n)).astype(np.int16) for n in rng.randint(0, 400, size=298)]
        batch = [clip] + other + [clip]
        bids = [t] + [int(v) for v in rng.randint(0, len(tables), size=298)] + [t]
        off = np.concatenate([[0], np.cumsum([len(c) for c in batch])]).tolist()
        out, out_off = ops.resample_var(torch.from_numpy(np.concatenate(batch)).to(DEV), off, bids, tables)
        got = out.cpu().numpy()
        assert np.array_equal(got[:out_off[1]], want) and np.array_equal(got[out_off[299]:], want)
        mid = 150
        L, M, taps = tables[bids[mid]]
        assert out_off[mid + 1] - out_off[mid] == ref.out_len(len(batch[mid]), L, M)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_nothing_is_written(ops):
    from ds2hip import lib
    pcm = torch.randint(-64, 65, (4096,), dtype=torch.int16, device=DEV)
    out = torch.full((8192,), SENTINEL, dtype=torch.int16, device=DEV)
    good = (1, 1, np.ones((1, 3), np.float32))
    off, out_off = [0, 1000, 4096], [0, 1000, 4096]
    cases = {
        '17 tables': dict(tables=[good] * 17),
        'K even': dict(tables=[good, (1, 1, np.ones((1, 4), np.float32))]),
        'L = 1025': dict(tables=[good, (1025, 1, np.ones((1025, 1), np.float32))]),
        'a tap offset past the bank': dict(tables=[good, good], bank_floats=5),
        'B = 0': dict(tables=[good], B=0),
    }
    for name, kw in cases.items():
        bank, desc = _bank(kw['tables'])
        with pytest.raises(lib.Ds2Error) as err:
            _raw(pcm, off, out_off, [0, 0], desc, bank, 3096, out, bank_floats=kw.get('bank_floats'), B=kw.get('B'))
        assert err.value.code == lib.ERR_ARG and 'ds2_resample_var' in str(err.value), name
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), name


def test_a_table_id_outside_the_list_skips_that_clip_only(ops):
    rng = np.random.RandomState(8)
    tables = [(1, 1, _int_taps(1, 3, rng)), (2, 1, _int_taps(2, 5, rng))]
    clips = [rng.randint(-64, 65, size=n).astype(np.int16) for n in (700, 1500, 900, 40)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).tolist()
    pcm = torch.from_numpy(np.concatenate(clips)).to(DEV)
    bank, desc = _bank(tables)
    for bad in (2, -1, 2 ** 31 - 1):
        ids = [1, bad, 0, 1]
        n_out = [1400, 1500, 900, 80]                  # (the skipped clip's span is sized as if it went through table 0)
        out_off = np.concatenate([[0], np.cumsum(n_out)]).tolist()
        out = torch.full((out_off[-1] + 8,), SENTINEL, dtype=torch.int16, device=DEV)
        _raw(pcm, off, out_off, ids, desc, bank, 1500, out)
        got = out.cpu().numpy()
        assert (got[out_off[1]:out_off[2]] == SENTINEL).all() and (got[out_off[-1]:] == SENTINEL).all()
        for b in (0, 2, 3):
            L, M, taps = tables[ids[b]]
            assert np.array_equal(got[out_off[b]:out_off[b + 1]], ref.resample(clips[b], 1, L, M, taps)), (bad, b)
        if bad < 2 ** 31 - 1:
            with pytest.raises(ValueError, match='table %d' % bad):                  # the wrapper refuses it first
                ops.resample_var(pcm, off, ids, tables)
    with pytest.raises(ValueError, match='resample_var'):
        ops.resample_var(pcm, off, [0, 0, 0], tables)
    with pytest.raises(ValueError, match='resample_var'):
        ops.resample_var(pcm, [0, 700, 600, 3140], [0, 0, 0], tables)
    with pytest.raises(ValueError, match='resample_var'):
        ops.resample_var(pcm, off, [0, 0, 0, 0], [(1, 1, np.ones((1, 2), np.float32))])


def test_outputs_past_max_out_are_not_written(ops):
    rng = np.random.RandomState(9)
    tables = [(2, 1, _int_taps(2, 5, rng))]
    clip = rng.randint(-64, 65, size=1500).astype(np.int16)
    bank, desc = _bank(tables)
    out = torch.full((3008,), SENTINEL, dtype=torch.int16, device=DEV)
    _raw(torch.from_numpy(clip).to(DEV), [0, 1500], [0, 3000], [0], desc, bank, 1030, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:1030], ref.resample(clip, 1, 2, 1, tables[0][2])[:1030]) and (got[1030:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the stage
def _pcm(n, seed):
    rng = np.random.RandomState(seed)
    return (np.clip(rng.standard_normal(n) * 0.1, -1, 1) * 32767).astype(np.int16)


def test_frontend_stage_equals_the_clips_converted_one_at_a_time(ops):
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, SpeedPerturb
    sp = SpeedPerturb(factors=(0.9, 1.0, 1.1, 0.937))
    lens, draws = [16000, 9001, 12345, 8000, 20000], [0, None, 2, 1, 3]
    tempos, gains = [1.0, 1.1, 0.9, 1.05, 1.0], [0.0, 2.5, -3.0, 0.0, 6.0]
    pcms = [torch.from_numpy(_pcm(n, 60 + i)) for i, n in enumerate(lens)]
    batch = RawAudioBatch.from_clips([PCMClip(p, t, g, speed=d) for p, t, g, d in zip(pcms, tempos, gains, draws)])
    assert batch.speed == draws
    got, got_pct = BatchSpectrogram(speed=sp)(batch.to(DEV))
    conv = []
    for p, d in zip(pcms, draws):                       # one clip at a time through ds2_resample with the stage's table
        table = sp.tables()[sp.table_ids([d])[0]]
        out, _ = ops.resample(p.to(DEV), [0, p.numel()], 16000, taps=_rw(table))
        assert out.numel() == sp.out_len(p.numel(), d)
        conv.append(out.cpu())
    assert torch.equal(conv[1], pcms[1]) and torch.equal(conv[3], pcms[3])            # no draw, and the factor 1.0
    assert conv[0].numel() == 17778 and conv[2].numel() == ref.out_len(12345, 10, 11)
    want, want_pct = BatchSpectrogram()(RawAudioBatch.from_clips([PCMClip(p, t, g) for p, t, g in zip(conv, tempos, gains)])
                                        .to(DEV))
    assert got.shape == want.shape and torch.equal(got, want) and torch.equal(got_pct, want_pct)
    # pct and t_max follow the new lengths
    wav, offs = ops.decode_augment(torch.cat(conv).to(DEV), np.concatenate([[0], np.cumsum([c.numel() for c in conv])]).tolist(),
                                   tempos, gains)
    frames = [1 + (offs[i + 1] - offs[i]) // 160 for i in range(len(lens))]
    assert got.shape[1] == max(frames) and got_pct.tolist() == [np.float32(f / float(max(frames))) for f in frames]
    plain_frames = BatchSpectrogram()(RawAudioBatch.from_clips([PCMClip(p, t, g) for p, t, g in zip(pcms, tempos, gains)])
                                      .to(DEV))[0].shape[1]
    assert got.shape[1] != plain_frames
    with pytest.raises(RuntimeError, match='speed draws'):                            # draws but no speed=
        BatchSpectrogram()(batch.to(DEV))


def test_a_batch_without_draws_launches_nothing(ops, monkeypatch):
    from codes.transforms import BatchSpectrogram, PCMClip, RawAudioBatch, SpeedPerturb
    clips = [PCMClip(torch.from_numpy(_pcm(n, 40 + i)), 1.05, 1.5) for i, n in enumerate((16000, 9000))]
    batch = RawAudioBatch.from_clips(clips)
    assert batch.speed is None
    want, want_pct = BatchSpectrogram()(batch.to(DEV))

    def never(*a, **k):
        raise AssertionError('resample_var was launched for a batch without draws')
    monkeypatch.setattr(ops, 'resample_var', never)
    got, got_pct = BatchSpectrogram(speed=SpeedPerturb())(batch.to(DEV))
    assert torch.equal(got, want) and torch.equal(got_pct, want_pct)


def test_per_clip_call_runs_the_same_kernel(ops):
    from codes.transforms import SpeedPerturb
    x = torch.from_numpy(_pcm(5000, 3))
    sp = SpeedPerturb(factors=(1.1,), prob=1.0)
    y = sp(x)
    want, _ = ops.resample(x.to(DEV), [0, 5000], 16000, taps=_rw(ops.speed_design(1.1)))
    assert y.device == x.device and y.dtype == torch.int16 and torch.equal(y, want.cpu())
    assert SpeedPerturb(prob=0.0)(x) is x
