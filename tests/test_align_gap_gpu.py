"""``ds2_ctc_align_banded_gap`` on the GPU against the float64 host reference (tests/align_gap_ref.py).

Every input is a LOG input whose values are multiples of 1/4 of size at most 16 (or -inf), and every penalty a multiple of
1/4, so f[t] = m[t] - g is exact in fp32 and every path sum is a multiple of 1/4 below 2^18 in size at T <= 9000: exact in
fp64.  The tie rule and the band decide alone, and states, starts, ends, gap and the float64 score must EQUAL the reference.
Every launch reads probabilities that are NaN in every frame past an utterance's size and a band row that is garbage there,
works in a garbage-filled workspace and writes its outputs into the middle of larger sentinel-filled tensors."""
import numpy as np
import pytest
import torch

from tests import align_banded_ref as bref
from tests import align_gap_ref as gref

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = ('states', 'starts', 'ends', 'gap', 'score')
INF = float('inf')
SPACE = 1


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape), fill


def _i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32).reshape(-1), dtype=torch.int32, device='cuda')


def _launch(probs, sizes, labels_list, lo, w, g, space=SPACE, blank=0, lmax=None, ws=None, lens=None, ws_fill=0xA5):
    """One launch of the C entry point -> numpy (states, starts, ends, gap, score)."""
    from ds2hip import lib
    true_lens = [len(v) for v in labels_list]
    lmax = max(true_lens + [0]) if lmax is None else lmax
    offs = np.cumsum([0] + true_lens[:-1])
    flat = [x for v in labels_list for x in v]
    x = np.array(probs, dtype=np.float32)
    bsz, t, a = x.shape
    lo = np.array(lo, dtype=np.int64).reshape(bsz, t)
    for b in range(bsz):
        n = min(max(int(sizes[b]), 0), t)
        x[b, n:] = np.nan
        lo[b, n:] = -7 - b
    p = torch.from_numpy(x).cuda()
    lo_d = torch.from_numpy(lo.astype(np.int32)).cuda()
    if ws is None:
        ws = torch.full((max(lib.query('ds2_ctc_align_banded_gap_ws_bytes', bsz, t, w), 16),), ws_fill, dtype=torch.uint8,
                        device='cuda')
    outs = [_guarded((bsz, t), torch.int32, -777), _guarded((bsz, lmax), torch.int32, -778),
            _guarded((bsz, lmax), torch.int32, -779), _guarded((bsz, t), torch.uint8, 77),
            _guarded((bsz,), torch.float64, 12345.0)]
    lib.call('ds2_ctc_align_banded_gap', p, _i32(sizes), _i32(flat), _i32(offs), _i32(true_lens if lens is None else lens),
             lo_d, bsz, t, a, lmax, w, blank, space, float(g), 1, ws, ws.numel(), *[o[1] for o in outs])
    torch.cuda.synchronize()
    for (buf, view, fill), name in zip(outs, NAMES):
        n = view.numel()
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), name + ': written outside'
    return tuple(o[1].cpu().numpy() for o in outs)


def _assert_equal(got, want, what):
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and g.shape == x.shape, (what, name, g.dtype, x.dtype, g.shape, x.shape)
        assert np.array_equal(g, x), (what, name, g, x)


def _check(probs, sizes, labels_list, lo, w, g, what, space=SPACE, blank=0, **kw):
    want = gref.align_batch_banded_gap(probs, sizes, labels_list, lo, w, blank, space, g, True, kw.get('lmax'))
    got = _launch(probs, sizes, labels_list, lo, w, g, space, blank, **kw)
    _assert_equal(got, want, what)
    _check_invariants(probs, sizes, labels_list, got, g, space, blank, what)
    return got


def _check_invariants(probs, sizes, labels_list, got, g, space, blank, what):
    """gap only at eligible states; the gap frames' f[t] plus the other frames' path terms is the score, exactly."""
    states, _, _, gap, score = got
    for b, labels in enumerate(labels_list):
        n = min(max(int(sizes[b]), 0), states.shape[1])
        assert not gap[b, n:].any(), (what, b)
        if not np.isfinite(score[b]):
            assert not gap[b].any() and (states[b] == -1).all(), (what, b)
            continue
        lp, f, gapframe = gref.frame_values(np.asarray(probs)[b, :n], True, blank, g)
        st, gp = states[b, :n].astype(np.int64), gap[b, :n].astype(bool)
        assert gref.eligible(labels, space)[st][gp].all() and gapframe[gp].all(), (what, b)
        ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
        ext[1::2] = labels
        plain = lp[np.arange(n), ext[st]].astype(np.float64)
        assert f[gp].astype(np.float64).sum() + plain[~gp].sum() == score[b], (what, b)


def _quarters(rng, shape, lo=-40, hi=1, holes=0.0):
    x = (rng.integers(lo, hi, size=shape) / 4.0).astype(np.float32)
    if holes:
        x[rng.random(shape) < holes] = -np.inf
    return x


def _words(rng, n, a, every=5):
    """n labels without adjacent repeats, a space at every ``every``-th place (never first or last); a - 1 is never used."""
    out = []
    for i in range(n):
        if i % every == every - 1 and i < n - 1:
            out.append(SPACE)
            continue
        v = int(rng.integers(2, a - 1))
        while out and v == out[-1]:
            v = int(rng.integers(2, a - 1))
        out.append(v)
    return out


def _recording(rng, labels, t, a, n_ins=5):
    """A peaked recording of exactly t frames: every label one frame, blanks between them while frames last (spread evenly),
    the frame's own symbol at 0 and the rest between -10 and -3; blocks of ``n_ins`` frames of the foreign symbol a - 1 (the
    rest there below -3 too) before the first frame, after the blank that follows the middle space, and after the last frame.
    -> (x (t,a) float32, inserted (t,) bool).  Needs t >= len(labels) + 3 n_ins + 1."""
    n = len(labels)
    spaces = [i for i, v in enumerate(labels) if v == SPACE]
    mid = spaces[len(spaces) // 2] if spaces else -1
    spare = t - n - 3 * n_ins - (1 if mid >= 0 else 0)
    assert spare >= 0
    seq = [(a - 1, True)] * n_ins
    for i, v in enumerate(labels):
        seq.append((v, False))
        if i == mid:
            seq += [(0, False)] + [(a - 1, True)] * n_ins
        k = spare // (n - i)                                          # blanks after this label: the spare frames, spread
        seq += [(0, False)] * k
        spare -= k
    seq += [(a - 1, True)] * (n_ins if mid >= 0 else 2 * n_ins)
    assert len(seq) == t, (len(seq), t)
    x = _quarters(rng, (t, a), -40, -11)
    x[np.arange(t), [s for s, _ in seq]] = 0.0
    return x, np.array([f for _, f in seq], dtype=bool)


BANDS = (64, 128, 256, 512, 1024, 2048, 4096, 8192)


@pytest.mark.parametrize('form', ['full', 'slide'])
@pytest.mark.parametrize('w', BANDS)
def test_every_band_instantiation(w, form):
    """W >= S (every slot's state fixed) and S > W on the sliding diagonal band; a recording with uncovered blocks at the
    start, between two words and at the end, beside a random utterance of the same size.  g = 1."""
    rng = np.random.default_rng(w + (form == 'slide'))
    a = 29
    n = w // 2 - 3 if form == 'full' else min(w, 4500)
    t = 2 * n + 40 if form == 'full' else (2 * n + 2 * w if w < 4096 else 9000)
    s_n = 2 * n + 1
    assert (s_n <= w) == (form == 'full')
    big = w >= 4096
    labels = [_words(rng, n, a)] + ([] if big else [_words(rng, n, a, every=3)])
    x0, ins = _recording(rng, labels[0], t, a)
    x = np.stack([x0] + ([] if big else [_quarters(rng, (t, a))]))
    lo = np.stack([bref.diagonal(t, s_n, w)] * len(labels))
    sizes = [t] + ([] if big else [t - 1])
    states, starts, ends, gap, score = _check(x, sizes, labels, lo, w, 1.0, (w, form))
    assert np.isfinite(score).all()
    assert np.array_equal(gap[0].astype(bool), ins)                   # the uncovered frames, and only they
    first, mid = np.flatnonzero(ins)[0], np.flatnonzero(ins)[len(np.flatnonzero(ins)) // 2]
    assert first == 0 and ins[-1] and 0 < states[0][mid] < s_n - 1 and states[0][mid] % 2 == 0
    if form == 'slide':
        assert lo[0][-1] == s_n - w and lo[0][-1] > 0
    if not big:
        assert gap[1].any()


@pytest.mark.parametrize('a,frames', [(29, (31, 32, 33, 63, 64, 65, 128, 129)), (256, (3, 4, 5, 9))])
def test_frame_counts_around_the_staging_chunk_and_the_back_trace_window(a, frames):
    """A chunk is 32 frames at A = 29 and 4 at A = 256; a back-trace window is 64 frames.  W = 64 with S below and above it."""
    rng = np.random.default_rng(a)
    for t in frames:
        lens = [0, min(t // 2, 3), min(max(t // 2 - 1, 0), 50)]
        labels = [_words(rng, n, a, every=3) for n in lens]
        x = _quarters(rng, (3, t, a), holes=0.02)
        lo = np.stack([bref.diagonal(t, 2 * n + 1, 64) for n in lens])
        for g in (0.5, 3.0):
            got = _check(x, [t, t, t - 1 if lens[2] < t // 2 else t], labels, lo, 64, g, (a, t, g))
            assert np.isfinite(got[4][:2]).all()
    assert 2 * lens[2] + 1 > 64 or a == 256


def test_sliding_band_hands_slots_to_eligible_and_other_blanks():
    """W = 64 over 301 states in irregular steps: a slot is taken over by end blanks, blanks beside a space and blanks inside
    words in turn; with g = 1/2 on random inputs the path absorbs frames in inner eligible blanks."""
    rng = np.random.default_rng(17)
    a, w, n, t = 12, 64, 150, 330
    labels = [_words(rng, n, a, every=2), _words(rng, n, a, every=3), _words(rng, n, a, every=150)]
    s_n = 2 * n + 1
    x = _quarters(rng, (3, t, a), -24, 1)
    lo = np.stack([bref.diagonal(t, s_n, w), np.minimum(bref.staircase(t, (0, 1, 2, 0, 3, 0)), s_n - w),
                   bref.diagonal(t, s_n, w)])
    states, _, _, gap, score = _check(x, [t, t, t - 2], labels, lo, w, 0.5, 'slide')
    assert np.isfinite(score).all()
    for b in range(2):
        inner = states[b][gap[b] == 1]
        assert ((inner > 0) & (inner < s_n - 1)).sum() >= 5
    el = gref.eligible(labels[1], SPACE)                            # (a period of 6 states against 64 slots)
    slots = {(int(s) % w, bool(el[s])) for s in range(0, s_n, 2)}
    assert any((k, True) in slots and (k, False) in slots for k in range(w))


def test_transcripts_without_an_eligible_inner_state():
    """Leading, trailing and doubled spaces, no space at all, and space = -1."""
    rng = np.random.default_rng(23)
    a, t, w = 8, 40, 64
    labels = [[1, 2, 3, 4], [2, 3, 4, 1], [2, 1, 1, 3], [2, 3, 4, 5], [1], [1, 1]]
    x = _quarters(rng, (len(labels), t, a), -24, 1)
    lo = np.zeros((len(labels), t))
    for g in (0.25, 2.0):
        got = _check(x, [t] * len(labels), labels, lo, w, g, ('space', g))
        none = _check(x, [t] * len(labels), labels, lo, w, g, ('no space', g), space=-1)
        inner = (none[0] > 0) & (none[0] < 2 * np.array([len(v) for v in labels])[:, None])
        assert not (none[3].astype(bool) & inner).any()
        assert (got[4] >= none[4]).all() and (got[4][[0, 1, 2]] > none[4][[0, 1, 2]]).any()
    assert np.array_equal(got[0][3], none[0][3]) and got[4][3] == none[4][3]       # no space in the transcript: the same


def test_empty_transcript():
    rng = np.random.default_rng(29)
    a, t = 29, 70
    x = _quarters(rng, (2, t, a), -40, -3)
    x[:, :, 5] = 0.0
    x[:, :, 0] = -8.0
    lo = np.zeros((2, t))
    got = _check(x, [t, t - 3], [[], []], lo, 64, 1.0, 'L = 0', lmax=0)
    assert got[3][0].all() and got[3][1][:t - 3].all() and (got[0][0] == 0).all()
    assert got[4][0] == -1.0 * t and got[4][1] == -1.0 * (t - 3)
    got = _check(x, [t, t - 3], [[], []], lo, 64, INF, 'L = 0, no gaps', lmax=0)
    assert not got[3].any() and got[4][0] == -8.0 * t
    got = _check(x, [0, t], [[], [2]], lo, 64, 1.0, 'no frames', lmax=1)
    assert got[4][0] == 0.0 and not got[3][0].any()


def test_frames_without_a_finite_value():
    """m[t] = -inf: f[t] = -inf, no gap there, and no path through the frame.  A frame whose blank alone is -inf is absorbed."""
    rng = np.random.default_rng(31)
    a, t = 6, 34
    labels = [[2, 1, 3]] * 3
    x = _quarters(rng, (3, t, a), -24, 1)
    x[0, 33] = -np.inf                                              # the chunk's second frame
    x[1, :4, 0] = -np.inf
    x[1, :4, 2:4] = -np.inf                                         # only a gap in state 0 gets through the opening
    x[2, 10] = np.nan                                               # NaN counts as -inf
    got = _check(x, [t] * 3, labels, np.zeros((3, t)), 64, 1.0, 'holes')
    assert got[4][0] == -np.inf and got[4][2] == -np.inf and np.isfinite(got[4][1]) and got[3][1][:4].all()


@pytest.mark.parametrize('g', [0.0, INF])
def test_penalty_zero_and_infinite(g):
    """g = 0: every eligible state takes the frame's best symbol for free.  g = inf: the bits of ``ops.ctc_align_banded`` on
    the same input, and no gap."""
    from ds2hip import ops
    rng = np.random.default_rng(37)
    a, t, w, n = 29, 200, 64, 70
    labels = [_words(rng, n, a), _words(rng, 9, a, every=3), []]
    x = _quarters(rng, (3, t, a), holes=0.02)
    lo = np.stack([bref.diagonal(t, 2 * len(v) + 1, w) for v in labels])
    sizes = [t, t - 5, t]
    got = _check(x, sizes, labels, lo, w, g, g)
    if g == 0.0:
        assert got[3].any()
        _, f, _ = gref.frame_values(x[2], True, 0, 0.0)
        assert got[4][2] == f.astype(np.float64).sum()
        return
    assert not got[3].any()
    xs = x.copy()
    for b, size in enumerate(sizes):
        xs[b, size:] = np.nan
    lens = [len(v) for v in labels]
    plain = ops.ctc_align_banded(torch.from_numpy(xs).cuda(), _i32(sizes), _i32([v for lab in labels for v in lab]),
                                 _i32(np.cumsum([0] + lens[:-1])), _i32(lens), max(lens),
                                 torch.from_numpy(lo.astype(np.int32)).cuda(), w, 0, True)
    for k, name in zip((0, 1, 2, 4), ('states', 'starts', 'ends', 'score')):
        p = plain[min(k, 3)].cpu().numpy()
        assert p.dtype == got[k].dtype and p.tobytes() == got[k].tobytes(), name
    via_ops = ops.ctc_align_banded_gap(torch.from_numpy(xs).cuda(), _i32(sizes), _i32([v for lab in labels for v in lab]),
                                       _i32(np.cumsum([0] + lens[:-1])), _i32(lens), max(lens),
                                       torch.from_numpy(lo.astype(np.int32)).cuda(), w, SPACE, 1.0, 0, True)
    _assert_equal(tuple(v.cpu().numpy() for v in via_ops), _launch(x, sizes, labels, lo, w, 1.0), 'ops')


def test_an_utterance_does_not_depend_on_its_company_or_the_workspace():
    rng = np.random.default_rng(41)
    a, t, w, n = 29, 150, 64, 60
    labels = _words(rng, n, a)
    x, _ = _recording(rng, labels, t, a)
    x[rng.random(x.shape) < 0.3] = -2.0                             # ties
    lo = bref.diagonal(t, 2 * n + 1, w)
    alone = _launch(x[None], [t], [labels], lo[None], w, 1.0)
    assert np.isfinite(alone[4][0]) and alone[3].any()
    others = [_words(rng, m, a) for m in (3, 70, 0, 20)]
    xo = _quarters(rng, (4, t, a))
    for pos in (0, 4):
        lab = others[:pos] + [labels] + others[pos:]
        xb = np.concatenate([xo[:pos], x[None], xo[pos:]])
        lob = np.stack([bref.diagonal(t, 2 * len(v) + 1, w) for v in lab])
        for fill in (0xFF, 0x00, 0xFF):                            # (0xFF: NaN patterns wherever the workspace were read)
            got = _launch(xb, [t - 1] * pos + [t] + [t - 2] * (4 - pos), lab, lob, w, 1.0, ws_fill=fill)
            for k, name in enumerate(NAMES):
                mine, want = np.atleast_1d(got[k][pos]), np.atleast_1d(alone[k][0])
                assert mine[:want.shape[0]].tobytes() == want.tobytes(), (pos, fill, name)


def test_no_alignment():
    """Bad bands, bad labels and infeasible inputs: score -inf, -1 everywhere, gap zero -- for that utterance alone."""
    rng = np.random.default_rng(43)
    a, t, w = 8, 40, 64
    good = [2, 1, 3]
    labels = [good, good, good, [2, 0, 3], [2, a, 3], [2] * 30, good, good]
    x = _quarters(rng, (len(labels), t, a), -24, 1)
    lo = np.zeros((len(labels), t), dtype=np.int64)
    lo[1, 5] = -1
    lo[2, 7:] = 3
    lo[2, 20:] = 2                                                  # a decrease
    lo[6, 10:] = 64                                                 # a step of W
    got = _check(x, [t] * len(labels), labels, lo, w, 0.5, 'failures')
    assert np.isfinite(got[4][[0, 7]]).all() and (got[4][1:7] == -np.inf).all()
    assert (got[0][1:7] == -1).all() and (got[1][1:7] == -1).all() and (got[2][1:7] == -1).all() and not got[3][1:7].any()
    got = _check(x, [t] * len(labels), labels, lo, w, 0.5, 'a label count past max_label_len', lmax=5)
    assert got[4][5] == -np.inf
    # a diagonal band too narrow for an opening the transcript does not cover: "no alignment" or a clipped path, as the
    # reference has it
    many = _words(rng, 100, a)
    xr, _ = _recording(rng, many, 400, a, n_ins=60)
    _check(xr[None], [400], [many], bref.diagonal(400, 201, w)[None], w, 1.0, 'clipped')


def test_refusals():
    from ds2hip import lib
    x, lo = np.zeros((1, 4, 3), dtype=np.float32), np.zeros((1, 4))
    for kw, word in ((dict(g=-0.25), 'gap_penalty'), (dict(g=float('nan')), 'gap_penalty'), (dict(g=-INF), 'gap_penalty'),
                     (dict(space=0), 'space'), (dict(space=3), 'space'), (dict(space=-2), 'space'),
                     (dict(space=2, blank=2), 'space')):
        args = dict(g=1.0, space=1, blank=0)
        args.update(kw)
        with pytest.raises(lib.Ds2Error) as e:
            _launch(x, [4], [[1]], lo, 64, args['g'], args['space'], args['blank'])
        assert e.value.code == lib.ERR_ARG and word in str(e.value) and 'ds2_ctc_align_banded_gap' in str(e.value), kw
    for band in (0, 32, 96, 16384):
        with pytest.raises(lib.Ds2Error) as e:
            _launch(x, [4], [[2]], lo, band, 1.0, ws=torch.zeros(1 << 16, dtype=torch.uint8, device='cuda'))
        assert e.value.code == lib.ERR_ARG and 'band %d' % band in str(e.value)
    with pytest.raises(lib.Ds2Error) as e:
        _launch(x, [4], [[2]], lo, 64, 1.0, ws=torch.zeros(8, dtype=torch.uint8, device='cuda'))
    assert e.value.code == lib.ERR_ARG and 'workspace' in str(e.value)
    with pytest.raises(lib.Ds2Error) as e:
        _launch(x, [4], [[2]], lo, 64, 1.0, blank=3)
    assert e.value.code == lib.ERR_ARG
    with pytest.raises(lib.Ds2Error) as e:
        _launch(np.zeros((1, 4, 257), dtype=np.float32), [4], [[2]], lo, 64, 1.0)
    assert e.value.code == lib.ERR_ARG and 'alphabet' in str(e.value)
    ws, f64 = torch.zeros(1 << 12, dtype=torch.uint8, device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda')
    u8 = torch.zeros(4, dtype=torch.uint8, device='cuda')
    with pytest.raises(lib.Ds2Error) as e:
        lib.call('ds2_ctc_align_banded_gap', torch.zeros((1, 4, 3), device='cuda'), _i32(4), _i32(1), _i32(0), _i32(1),
                 _i32([0, 0, 0, 0]), 1, 4, 3, 1 << 30, 64, 0, 1, 1.0, 1, ws, ws.numel(), _i32([0, 0, 0, 0]), _i32(0), _i32(0),
                 u8, f64)
    assert e.value.code == lib.ERR_ARG and 'max_label_len' in str(e.value)
    assert lib.query('ds2_ctc_align_banded_gap_ws_bytes', 2, 100, 64) == lib.query('ds2_ctc_align_banded_ws_bytes', 2, 100, 64)
    with pytest.raises(RuntimeError):
        from ds2hip import ops
        ops.ctc_align_banded_gap(torch.zeros((1, 4, 3), device='cuda'), _i32(4), _i32(1), _i32(0), _i32(1), 1,
                                 torch.zeros((1, 3), dtype=torch.int32, device='cuda'), 64, 1, 1.0)
