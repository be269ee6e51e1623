"""``ds2_vad_segment`` (csrc/vad.hip) against tests/vad_ref.py: the rule uses integers only, so ``segs`` and ``info`` must be
EQUAL.  Every case is a few thousand blocks at most, except the two that need their size (65537 blocks: a partial last
thread range of every scan; 60 000 blocks with max_len = 50: hundreds of splits)."""
import functools

import numpy as np
import pytest
import torch

from tests import vad_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# blocks: min_speech 5, min_silence 6, pad 2; threshold pinned at bin 40 (any block next to a loud one is speech)
RULE = dict(rank=0, margin_bins=0, min_bin=40, max_bin=40, min_speech=5, min_silence=6, pad=2, max_len=100)
ORDER = ('rank', 'margin_bins', 'min_bin', 'max_bin', 'min_speech', 'min_silence', 'pad', 'max_len')


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


def _check(ops, x, rule, want=None):
    """Run the wrapper on ``x`` and compare with the reference (returned, for further assertions on its masks)."""
    want = want or ref.vad_ref(x, **rule)
    segs, info = ops.vad_segment(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), **rule)
    assert segs.dtype == torch.int32 and tuple(segs.shape) == (len(want['segs']), 2)
    np.testing.assert_array_equal(segs.numpy(), want['segs'])
    assert [info[k] for k in ('n_seg', 'floor_bin', 'thr', 'speech_blocks', 'nb')] == want['info'][:5]
    return want


def _loud(nb, *spans):
    m = np.zeros(nb, np.int64)
    for s, e in spans:
        m[s:e] = 1
    return m


def _lengths(mask, value):
    return [e - s for s, e in ref.runs(mask, value)]


@pytest.mark.parametrize('fill', [0, 20000, -32768])
def test_tiny_lengths(ops, fill):
    """Around one, two and three blocks, and 30 blocks with max_len = 4 (every run is split); -32768 gives the largest sums a
    block can hold."""
    rule = dict(rank=0, margin_bins=16, min_bin=75, max_bin=115, min_speech=2, min_silence=3, pad=1, max_len=4)
    for n in (0, 1, 159, 160, 161, 319, 320, 321, 480, 4800):
        want = _check(ops, np.full(n, fill, np.int16), rule)
        if fill and n >= 320:
            assert want['info'][0] >= 1 and want['info'][3] == want['info'][4]
        if fill == -32768 and n == 4800:
            assert max(want['S']) == 3 * 160 * 2 ** 30 and max(want['bins']) == 155 and want['info'][0] > 7
        if not fill:
            assert want['info'][0] == 0


def test_six_clip_recording_through_the_segmenter():
    from codes.segment import Segmenter
    x, clips = ref.six_clip_recording()
    s = Segmenter()
    nb = -(-len(x) // 160)
    want = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    for pcm in (torch.from_numpy(x), torch.from_numpy(x).to(DEV)):              # from the host, or already on the device
        samples, stats = s.segment(pcm)
        np.testing.assert_array_equal(stats['blocks'], want['segs'])
        np.testing.assert_array_equal(samples, np.minimum(want['segs'].astype(np.int64) * 160, len(x)))
        assert len(samples) == 6 and stats['nb'] == nb
        for (a, b), (lo, hi) in zip(samples.tolist(), clips):
            assert 1760 <= lo - a <= 1900 and 1760 <= b - hi <= 1900
        assert stats['speech_seconds'] == want['info'][3] / 100.0
        assert -61.0 < stats['noise_floor_db'] <= -60.0 and -49.0 < stats['threshold_db'] < -48.0       # bins 75 and 91


@pytest.mark.parametrize('kind', ['noise', 'constant'])
def test_forced_splits_of_forty_seconds_of_speech(ops, kind):
    """max_bin binds (the noise floor IS the speech), so all 4000 blocks are one run that must be cut; in the constant case
    every argmin is a tie and the smallest index wins."""
    if kind == 'noise':
        x = (np.clip(0.1 * np.random.default_rng(3).standard_normal(640000), -1, 1) * 32767).astype(np.int16)
    else:
        x = np.full(640000, 3000, np.int16)
    rule = dict(rank=400, margin_bins=16, min_bin=75, max_bin=115, min_speech=25, min_silence=30, pad=10, max_len=1500)
    want = _check(ops, x, rule)
    assert want['info'][2] == 115 and want['info'][3] == 4000 and want['info'][0] >= 3
    assert all(750 <= e - s <= 1500 for s, e in want['segs'].tolist())
    if kind == 'constant':
        assert want['segs'].tolist() == [[0, 750], [750, 1500], [1500, 2250], [2250, 3000], [3000, 4000]]


def test_edge_length_patterns(ops):
    """Runs and gaps of exactly min_speech - 1, min_speech, min_silence - 1 and min_silence blocks, asserted on the
    reference's own masks: the three-block sum widens a loud run by one block on each side."""
    want = _check(ops, ref.pcm_from_blocks(_loud(40, (3, 13), (20, 30))), RULE)
    assert _lengths(want['m3'], 0)[1] == RULE['min_silence'] - 1 and want['info'][0] == 1
    want = _check(ops, ref.pcm_from_blocks(_loud(40, (3, 13), (21, 31))), RULE)
    assert _lengths(want['m3'], 0)[1] == RULE['min_silence'] and want['info'][0] == 2
    want = _check(ops, ref.pcm_from_blocks(_loud(30, (10, 12))), RULE)
    assert _lengths(want['m3'], 1) == [RULE['min_speech'] - 1] and want['info'][0] == 0
    want = _check(ops, ref.pcm_from_blocks(_loud(30, (10, 13))), RULE)
    assert _lengths(want['m3'], 1) == [RULE['min_speech']] and want['info'][0] == 1
    # a blip between two gaps of min_silence: dropped, and the gap it leaves is not closed afterwards
    want = _check(ops, ref.pcm_from_blocks(_loud(45, (3, 13), (21, 23), (31, 39))), RULE)
    assert _lengths(want['m4'], 1) == [12, 4, 10] and want['info'][0] == 2
    # a chain of short runs that only gap closing makes long enough; leading and trailing gaps shorter than min_silence
    want = _check(ops, ref.pcm_from_blocks(_loud(24, (4, 5), (9, 10), (14, 15), (19, 20)), last=1), RULE)
    assert _lengths(want['m3'], 1) == [3, 3, 3, 3] and _lengths(want['m3'], 0) == [3, 2, 2, 2, 3]
    assert want['segs'].tolist() == [[1, 23]]
    # pads clamp at 0 and nb
    want = _check(ops, ref.pcm_from_blocks(_loud(30, (0, 5), (25, 30)), last=7), RULE)
    assert want['segs'].tolist() == [[0, 8], [22, 30]]


@functools.lru_cache(maxsize=None)
def _random_case(nb, max_len, seed):
    """Quiet blocks of amplitude 3 .. 10 and loud ones of 300 .. 30000 in runs whose lengths straddle min_speech and
    min_silence, a few long enough to split; speech in block 0 and in the (partial) last block."""
    rng = np.random.default_rng(seed)
    # a blip between two long gaps, a run of three pieces, a gap that closes; then at random
    loud, state = [1] * 8 + [0] * 9 + [1] * 2 + [0] * 9 + [1] * (3 * max_len + 5) + [0] * 4, 1
    while len(loud) < nb:
        n = int(rng.integers(1, 13)) if rng.random() < 0.9 else int(rng.integers(max_len, 6 * max_len))
        loud += [state] * n
        state ^= 1
    loud = np.asarray(loud[:nb])
    loud[-8:] = 1
    amp = np.where(loud == 1, rng.integers(300, 30001, nb), rng.integers(3, 11, nb))
    x = ref.pcm_from_blocks(np.ones(nb, np.int64), amp, last=77)
    x = (x * rng.choice(np.array([-1, 1], np.int16), len(x))).astype(np.int16)
    rule = dict(rank=nb // 20, margin_bins=16, min_bin=20, max_bin=150, min_speech=5, min_silence=6, pad=2, max_len=max_len)
    return x, rule, ref.vad_ref(x, **rule)


@pytest.mark.parametrize('nb, max_len', [(1023, 40), (1024, 40), (1025, 40), (4097, 40), (65537, 40), (60000, 50)])
def test_random_patterns(ops, nb, max_len):
    x, rule, want = _random_case(nb, max_len, nb)
    assert len(x) == 160 * nb - 83 and want['m5'][0] == 1 and want['m5'][-1] == 1
    assert want['m4'] != want['m3'] and want['m5'] != want['m4']                 # gaps were closed and blips dropped
    assert 20 < want['info'][2] < 150                                             # neither clamp binds
    n_split = len(want['segs']) - len(ref.runs(want['m5'], 1))
    assert n_split >= (300 if nb == 60000 else 2)
    _check(ops, x, rule, want)


def test_threshold_clamps_and_rank_edges(ops):
    loud = _loud(50, (11, 50))
    x = ref.pcm_from_blocks(loud, amp=np.linspace(200, 9000, 50).astype(np.int64))
    base = dict(RULE, margin_bins=4, min_bin=0, max_bin=191)
    zero_s = sum(1 for s in ref.vad_ref(x, **base)['S'] if s == 0)
    assert zero_s == 10                                                           # hist[0] = 10: the cumulative count at bin 0
    at = _check(ops, x, dict(base, rank=zero_s - 1))
    past = _check(ops, x, dict(base, rank=zero_s))                               # equal to rank is not more than rank
    assert at['info'][1] == 0 and past['info'][1] == min(b for b in past['bins'] if b > 0) > 0
    top = _check(ops, x, dict(base, rank=49))
    assert top['info'][1] == max(top['bins']) and top['info'][2] == top['info'][1] + 4 and top['info'][0] == 0
    assert _check(ops, x, dict(base, rank=0))['info'][1] == 0
    low = _check(ops, x, dict(base, rank=20, min_bin=150))                        # min_bin binds
    assert low['info'][1] + 4 < 150 == low['info'][2] and low['info'][0] == 0
    high = _check(ops, x, dict(base, rank=20, max_bin=60))                        # max_bin binds
    assert high['info'][1] + 4 > 60 == high['info'][2] and high['info'][0] == 1
    both = _check(ops, x, dict(base, rank=20, min_bin=150, max_bin=60))           # the upper clamp is applied last
    assert both['info'][2] == 60


def _raw(lib, pcm, rule, ws, segs, seg_cap, info):
    lib.call('ds2_vad_segment', pcm.data_ptr(), pcm.numel(), *[rule[k] for k in ORDER], ws, ws.numel(), segs, seg_cap, info)


def test_memory_contract(ops):
    from ds2hip import lib
    x, rule, want = _random_case(1025, 40, 1025)
    n, n_seg = len(x), len(want['segs'])
    assert n % 8 and n_seg > 8
    ws_bytes = lib.query('ds2_vad_segment_ws_bytes', n)
    results = []
    for offset in (1, 4, 7, 8):                                                   # every kind of 16-byte misalignment
        big = torch.full((n + 64,), 32767, dtype=torch.int16, device=DEV)
        big[offset:offset + n] = torch.from_numpy(x).to(DEV)
        pcm = big[offset:offset + n]
        assert pcm.data_ptr() % 16 == (2 * offset) % 16
        for fill in (0xFF, 0x00):                                                 # what ws and segs held does not matter
            ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=DEV)
            segs = torch.full((n_seg + 3, 2), 12345 + fill, dtype=torch.int32, device=DEV)
            info = torch.full((8,), 777, dtype=torch.int32, device=DEV)
            _raw(lib, pcm, rule, ws, segs, n_seg + 2, info)
            results.append((segs.cpu().numpy(), info.cpu().numpy()))
            got, sentinel = results[-1][0], 12345 + fill
            np.testing.assert_array_equal(got[:n_seg], want['segs'])
            assert (got[n_seg:n_seg + 2] == -1).all() and (got[n_seg + 2] == sentinel).all()
            assert results[-1][1].tolist() == want['info']
        assert (big[:offset] == 32767).all() and (big[offset + n:] == 32767).all()
    for segs, info in results[1:]:                                                # bit-identical from run to run
        np.testing.assert_array_equal(segs[:n_seg + 2], results[0][0][:n_seg + 2])
        np.testing.assert_array_equal(info, results[0][1])
    # fewer rows than segments: the true count, seg_cap rows, nothing behind them
    pcm = torch.from_numpy(x).to(DEV)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    segs = torch.full((6, 2), 4242, dtype=torch.int32, device=DEV)
    info = torch.zeros(8, dtype=torch.int32, device=DEV)
    _raw(lib, pcm, rule, ws, segs, 5, info)
    assert int(info[0]) == n_seg
    np.testing.assert_array_equal(segs[:5].cpu().numpy(), want['segs'][:5])
    assert (segs[5] == 4242).all()
    with pytest.raises(RuntimeError, match='do not fit'):
        ops.vad_segment(pcm, seg_cap=5, **rule)
    # a caller's workspace, and the refusal of one that is too small or of another type
    got, _ = ops.vad_segment(pcm, ws=ws, **rule)
    np.testing.assert_array_equal(got.numpy(), want['segs'])
    with pytest.raises(ValueError, match='workspace'):
        ops.vad_segment(pcm, ws=ws[:ws_bytes - 1], **rule)
    for bad in (pcm.cpu(), pcm.float(), pcm.view(1, -1)):
        with pytest.raises(RuntimeError, match='1-D int16 tensor on the device'):
            ops.vad_segment(bad, **rule)


def test_argument_errors():
    from ds2hip import lib
    n = 1600                                                                      # nb = 10
    pcm = torch.zeros(n, dtype=torch.int16, device=DEV)
    ws_bytes = lib.query('ds2_vad_segment_ws_bytes', n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    segs = torch.full((4, 2), 99, dtype=torch.int32, device=DEV)
    info = torch.full((8,), 99, dtype=torch.int32, device=DEV)
    good = dict(RULE, rank=9)
    _raw(lib, pcm, good, ws, segs, 4, info)
    assert info.tolist() == [0, 0, 40, 0, 10, 0, 0, 0] and (segs == -1).all()
    segs.fill_(99), info.fill_(99)

    def refused(rule=good, pcm_arg=(pcm.data_ptr(), n), ws_arg=(ws.data_ptr(), ws_bytes), seg_cap=4):
        with pytest.raises(lib.Ds2Error) as e:
            lib.call('ds2_vad_segment', pcm_arg[0], pcm_arg[1], *[rule[k] for k in ORDER], ws_arg[0], ws_arg[1], segs,
                     seg_cap, info)
        assert e.value.code == lib.ERR_ARG, e.value

    refused(dict(good, min_speech=1))
    refused(dict(good, max_len=3))
    refused(dict(good, pad=-1))
    refused(dict(good, pad=3))                                                    # 2 pad == min_silence
    refused(dict(good, pad=4))
    refused(dict(good, rank=-1))
    refused(dict(good, rank=10))                                                  # nb - 1 is the last rank
    for key in ('margin_bins', 'min_bin', 'max_bin'):
        refused(dict(good, **{key: -1}))
        refused(dict(good, **{key: 192}))
    refused(pcm_arg=(pcm.data_ptr(), 2 ** 31))                                    # refused before anything is read
    refused(ws_arg=(ws.data_ptr(), ws_bytes - 1))
    refused(seg_cap=0)
    refused(dict(good, rank=1), pcm_arg=(pcm.data_ptr(), 0))                      # n = 0: only rank 0
    torch.cuda.synchronize()
    assert (segs == 99).all() and (info == 99).all()                              # no launch happened
    _raw(lib, pcm[:0], dict(good, rank=0), ws, segs, 4, info)                     # n = 0 itself is fine
    assert info.tolist() == [0] * 8 and (segs == -1).all()
