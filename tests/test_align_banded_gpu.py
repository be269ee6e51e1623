"""``ds2_ctc_align_banded`` on the GPU against the float64 host reference (tests/align_banded_ref.py).

Exact cases: log inputs k/64 with integer |k| <= 2048 and some -inf, as in tests/test_align_gpu.py; every path sum is a
multiple of 1/64 below 2^21 in size up to T = 45 000, so it is exact in fp64 and the tie rule and the band decide alone:
states, starts, ends and the float64 score must EQUAL the reference.  Rounded cases judge the path (valid, inside the band,
within the rounding bound of the banded optimum), not its identity.  Every launch writes its outputs into the middle of larger
sentinel-filled tensors, reads probabilities that are NaN in every frame past an utterance's size and a band row that is
garbage there."""
import numpy as np
import pytest
import torch

from tests import align_banded_ref as bref
from tests import align_ref
from tests.test_align_gpu import FRAMES, _activations, _dyadic, _labels, _softmax

pytestmark = pytest.mark.gpu

GUARD = 64                                           # sentinel elements on either side of every output
NAMES = ('states', 'starts', 'ends', 'score')


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape), fill


def _launch(probs, sizes, labels_list, lo, w, blank=0, log_input=True, lmax=None, ws=None, lens=None):
    """One launch of the C entry point -> numpy (states, starts, ends, score).  ``lens``: label_lens as passed, where they
    differ from the lists' lengths."""
    from ds2hip import lib
    dev = 'cuda'
    true_lens = [len(v) for v in labels_list]
    lmax = max(true_lens + [0]) if lmax is None else lmax
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32).reshape(-1), dtype=torch.int32, device=dev)   # noqa: E731
    offs = np.cumsum([0] + true_lens[:-1])
    flat = [x for v in labels_list for x in v]
    x = np.array(probs, dtype=np.float32)
    bsz, t, a = x.shape
    lo = np.array(lo, dtype=np.int64).reshape(bsz, t)
    for b in range(bsz):
        n = min(max(int(sizes[b]), 0), t)
        x[b, n:] = np.nan
        lo[b, n:] = -7 - b
    p = torch.from_numpy(x).to(dev)
    lo_d = torch.from_numpy(lo.astype(np.int32)).to(dev)
    if ws is None:
        ws = torch.empty(max(lib.query('ds2_ctc_align_banded_ws_bytes', bsz, t, w), 16), dtype=torch.uint8, device=dev)
    outs = [_guarded((bsz, t), torch.int32, -777), _guarded((bsz, lmax), torch.int32, -778),
            _guarded((bsz, lmax), torch.int32, -779), _guarded((bsz,), torch.float64, 12345.0)]
    lib.call('ds2_ctc_align_banded', p, i32(sizes), i32(flat), i32(offs), i32(true_lens if lens is None else lens), lo_d,
             bsz, t, a, lmax, w, blank, int(log_input), ws, ws.numel(), *[o[1] for o in outs])
    torch.cuda.synchronize()
    for (buf, view, fill), name in zip(outs, NAMES):
        n = view.numel()
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), name + ': written outside'
    return tuple(o[1].cpu().numpy() for o in outs)


def _assert_equal(got, want, what):
    for g, x, name in zip(got, want, NAMES):
        assert g.dtype == x.dtype and g.shape == x.shape, (what, name, g.dtype, x.dtype, g.shape, x.shape)
        assert np.array_equal(g, x), (what, name, g, x)            # (-inf == -inf; there is no NaN on either side)


def _check_exact(probs, sizes, labels_list, lo, w, what, blank=0, **kw):
    want = bref.align_batch_banded(probs, sizes, labels_list, lo, w, blank, True, kw.get('lmax'))
    got = _launch(probs, sizes, labels_list, lo, w, blank, True, **kw)
    _assert_equal(got, want, what)
    return want


def _band(t, s_n, w, steps=None):
    """The diagonal band, or a staircase that stops where the band reaches the last state."""
    if steps is None:
        return bref.diagonal(t, s_n, w)
    return np.minimum(bref.staircase(t, steps), max(s_n - w, 0))


def _held(lo, at, step):
    """``lo`` held at lo[at] until it can catch up in one step of at least ``step`` states."""
    lo = lo.copy()
    lo[at:int(np.searchsorted(lo, lo[at] + step))] = lo[at]
    return lo


@pytest.mark.parametrize('w', [64, 1024])
def test_full_band_equals_the_unbanded_kernel(w):
    """lo = 0 and W >= S: the result is ``ds2_ctc_align``'s, bit for bit (its float score is the double's rounding)."""
    from ds2hip import ops
    rng = np.random.default_rng(w)
    lens = [n for n in (0, 1, 2, 31, 511) if 2 * n + 1 <= w]
    a, feasible = 29, 0
    for t in FRAMES + [700]:
        labels = [_labels(rng, n, a) for n in lens]
        x = _dyadic(rng, (len(lens), t, a))
        x[1::2][rng.random(x[1::2].shape) < 0.05] = -np.inf
        x[:, :, 0][rng.random(x[:, :, 0].shape) < 0.3] = 0.0        # (blank frames that tie with each other)
        sizes = [t] * (len(lens) - 1) + [max(t - 1, 0)]
        got = _launch(x, sizes, labels, np.zeros((len(lens), t)), w)
        i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32).reshape(-1), dtype=torch.int32, device='cuda')   # noqa: E731
        old = ops.ctc_align(torch.from_numpy(x).cuda(), i32(sizes),
                            i32([v for lab in labels for v in lab]), i32(np.cumsum([0] + lens[:-1])), i32(lens), max(lens),
                            0, True)
        old = [o.cpu().numpy() for o in old]
        for g, o, name in zip(got[:3], old[:3], NAMES):
            assert np.array_equal(g, o), (w, t, name)
        assert got[3].dtype == np.float64 and np.array_equal(got[3].astype(np.float32), old[3]), (w, t, got[3], old[3])
        _assert_equal(got, align_ref_as_banded(x, sizes, labels), (w, t))
        feasible += int(np.isfinite(got[3]).sum())
    assert feasible >= 2 * len(FRAMES) - 3          # the empty transcript always aligns, two labels from three frames on
    if w == 1024:
        assert np.isfinite(got[3][4])                               # 511 labels in 700 frames


def align_ref_as_banded(x, sizes, labels):
    st, sa, en, sc = align_ref.align_batch(x, sizes, labels, 0, True)
    # (the float reference rounds its score; recompute it in float64)
    score = np.array([align_ref.viterbi(align_ref.frame_terms(x[b, :min(max(n, 0), x.shape[1])], True), labels[b])[0]
                      for b, n in enumerate(sizes)], dtype=np.float64)
    return st, sa, en, score


@pytest.mark.parametrize('a', [2, 29, 43, 128])
def test_the_band_moves(a):
    """W = 64 against 121 to 401 states: the band slides over the whole row, on the diagonal and in irregular steps, at frame
    counts around the staging chunk and the back-trace window."""
    rng = np.random.default_rng(a)
    w, feasible = 64, 0
    for t in (63, 64, 65, 127, 128, 129, 300):
        n = int(min(200, max(60, (t * 2) // 3)))                    # S = 2 n + 1 in 121 .. 401
        if a == 2:
            n = 60                                                  # one label repeated: 2 n - 1 = 119 frames at least
        labels = [_labels(rng, n, a) for _ in range(3)]
        x = _dyadic(rng, (3, t, a))
        x[2][rng.random(x[2].shape) < 0.03] = -np.inf
        s_n = 2 * n + 1
        lo = np.stack([_band(t, s_n, w), _band(t, s_n, w, (0, 1, 2, 3)), _held(_band(t, s_n, w), t // 3, 40)])
        assert 40 <= np.diff(lo[2]).max() < w
        want = _check_exact(x, [t, t, t - 1], labels, lo, w, (a, t))
        feasible += int(np.isfinite(want[3]).sum())
        print('a=%d T=%d S=%d scores %s' % (a, t, s_n, want[3]))
    assert feasible >= 4


@pytest.mark.parametrize('t', [3, 4, 5, 9])
def test_every_staging_slot_in_use(t):
    """A = 256, the largest alphabet: a staging chunk is 4 frames of 256 floats, so every slot of the buffer and every load
    of a staging thread is in use; frame counts below, at and above one chunk and just above two.  Bands that admit
    everything, that climb with the path, and one that leaves the first states behind."""
    rng = np.random.default_rng(256 + t)
    a, w = 256, 64
    lens = [0, min(t, 2), t // 2, t // 2]
    labels = [_labels(rng, n, a) for n in lens]
    x = _dyadic(rng, (len(lens), t, a))
    x[1::2][rng.random(x[1::2].shape) < 0.05] = -np.inf             # -inf holes for rows 1 and 3
    lo = np.zeros((len(lens), t), dtype=np.int64)
    lo[2] = np.minimum(bref.staircase(t, (0, 1)), 2 * lens[2])
    lo[3] = np.minimum(bref.staircase(t, (1, 2)), 2 * lens[3])
    want = _check_exact(x, [t, t, t, t - 1], labels, lo, w, (a, t))
    assert np.isfinite(want[3][0]) and np.isfinite(want[3][2])     # (no holes; row 2's band follows the path of one state per frame)
    print('T=%d scores %s' % (t, want[3]))


def _raised_blank(rng, t, a, side):
    x = _dyadic(rng, (t, a))
    half = slice(0, t // 2) if side == 'late' else slice(t // 2, t)
    x[half, 0] += 64.0
    return x


@pytest.mark.parametrize('t,n,w', [(300, 100, 64), (129, 60, 64), (2000, 800, 256)])
@pytest.mark.parametrize('side', ['late', 'early'])
def test_the_band_binds(t, n, w, side):
    """The blank is worth 64 more in one half of the frames, so the free optimum waits there and leaves the diagonal band:
    the banded optimum is strictly worse, runs along the band's edge, and the kernel finds exactly it."""
    from codes.align import band_margin
    # (the margin of the REFERENCE's path is 0 or 1 with these seeds; other seeds give 0 to 5: it is a property of the input)
    rng = np.random.default_rng(2000 + t + (side == 'late'))
    a = 29
    labels = _labels(rng, n, a)
    x = _raised_blank(rng, t, a, side)
    lo = bref.diagonal(t, 2 * n + 1, w)
    want = _check_exact(x[None], [t], [labels], lo[None], w, (t, n, w, side))
    free = align_ref.viterbi(x.astype(np.float64), labels)[0]
    margin = band_margin(want[0][0], lo, w, 2 * n + 1)
    print('T=%d L=%d W=%d %s: banded %.2f free %.2f margin %s' % (t, n, w, side, want[3][0], free, margin))
    assert np.isfinite(want[3][0]) and want[3][0] < free
    assert margin is not None and margin <= 3


def test_all_emissions_equal():
    """Every path ties: the tie rule and the band alone name the path."""
    t, n, w = 300, 100, 64
    labels = _labels(np.random.default_rng(4), n, 29)
    lo = bref.diagonal(t, 2 * n + 1, w)
    want = _check_exact(np.full((1, t, 29), -1.0, dtype=np.float32), [t], [labels], lo[None], w, 'all equal')
    assert want[3][0] == -300.0
    on_upper_edge = int((want[0][0] == lo + w - 1).sum())
    print('frames on the upper edge: %d' % on_upper_edge)
    assert on_upper_edge >= 100


def _band_max():
    from ds2hip import lib
    return lib.ALIGN_BAND_MAX


@pytest.mark.parametrize('case', ['below', 'above', 'far'])
@pytest.mark.parametrize('w', [2048, 4096, 'max'])
def test_several_states_per_thread(w, case):
    """2, 4 and W / 1024 states per thread; S just below W, just above it, and well above it (there the band is a staircase
    that climbs 7 states in 4 frames, which the path has to follow).  At T = 200 no transcript of this length can be spelled:
    no alignment; the frame counts beside it are the shortest that leave the paths some room."""
    w = _band_max() if w == 'max' else w
    rng = np.random.default_rng(w)
    a = 29
    long_n = 10000 if w == 2048 else 6000
    for n, steps in ({'below': (w // 2 - 1, (0,)), 'above': (w // 2, (0, 0, 1)), 'far': (long_n, (2, 2, 2, 1))}[case],):
        s_n = 2 * n + 1
        labels = _labels(rng, n, a)
        for t in (200, n + n // 8):
            x = _dyadic(rng, (1, t, a))
            lo = _band(t, s_n, w, steps)
            if case == 'far':                                       # (the staircase half a band late: the path has room below)
                lo = np.minimum(np.maximum(bref.staircase(t, steps) - w // 2, 0), s_n - w)
            want = _check_exact(x, [t], [labels], lo[None], w, (w, n, t))
            print('W=%d S=%d T=%d score %s' % (w, s_n, t, want[3][0]))
            assert np.isfinite(want[3][0]) == (t > 200)
            if t > 200 and s_n > w:
                assert lo[-1] == s_n - w and want[0][0][-1] >= s_n - 2


def test_indices_past_16_bits():
    """40 000 labels in 45 000 frames through 64 states: state and frame indices pass 2^16, the pointer bytes 2^21."""
    rng = np.random.default_rng(16)
    t, n, w, a = 45000, 40000, 64, 29
    labels = _labels(rng, n, a)
    x = _dyadic(rng, (1, t, a))
    lo = bref.diagonal(t, 2 * n + 1, w)
    assert int(np.diff(lo).max()) == 2
    want = _check_exact(x, [t], [labels], lo[None], w, 'long')
    assert np.isfinite(want[3][0]) and want[0][0][-1] >= 2 * n - 1 and want[1][0][-1] > 2 ** 15


def test_batch_company_and_workspace_contents_do_not_matter():
    from ds2hip import lib
    rng = np.random.default_rng(11)
    t, a, w = 150, 29, 64
    lens = [80, 0, 100]                                             # 100 labels in 90 frames: no alignment
    sizes = [150, 120, 90]
    labels = [_labels(rng, n, a) for n in lens]
    x = rng.integers(-2, 1, size=(3, t, a)).astype(np.float32)      # three levels: many ties
    lo = np.stack([np.resize(_band(sizes[0], 161, w), t), np.zeros(t, dtype=np.int64),
                   np.resize(_band(sizes[2], 201, w, (1, 2)), t)])
    alone = []
    for b in range(3):
        alone.append(_check_exact(x[b:b + 1], sizes[b:b + 1], labels[b:b + 1], lo[b:b + 1], w, ('alone', b), lmax=100))
    assert np.isfinite(alone[0][3][0]) and alone[1][3][0] < 0 and alone[2][3][0] == -np.inf
    ws = torch.empty(lib.query('ds2_ctc_align_banded_ws_bytes', 3, t, w), dtype=torch.uint8, device='cuda')
    for shift, fill in ((0, 0xFF), (1, 0x01), (2, None)):           # (None: the workspace as the last launch left it)
        order = [(b + shift) % 3 for b in range(3)]
        if fill is not None:
            ws.fill_(fill)
        got = _launch(x[order], [sizes[b] for b in order], [labels[b] for b in order], lo[order], w, ws=ws, lmax=100)
        for pos, b in enumerate(order):
            for g, x1, name in zip(got, alone[b], NAMES):
                assert g[pos].tobytes() == x1[0].tobytes(), (shift, pos, b, name)


def test_bad_input_on_the_device_costs_its_utterance_only():
    rng = np.random.default_rng(5)
    t, a, w, n = 120, 29, 64, 70
    good_lo = bref.diagonal(t, 2 * n + 1, w)
    base = _labels(rng, n, a)
    cases = [('good', good_lo, base, None),
             ('decreasing', np.r_[good_lo[:50], good_lo[49] - 1, good_lo[51:]], base, None),
             ('negative', np.r_[-1, good_lo[1:]], base, None),
             ('jump of W', np.r_[good_lo[:60], good_lo[60:] + (w - (good_lo[60] - good_lo[59]))], base, None),
             ('jump past W', np.r_[good_lo[:60], np.full(t - 60, good_lo[59] + w + 9)], base, None),
             ('blank as a label', good_lo, base[:30] + [0] + base[31:], None),
             ('label = A', good_lo, base[:69] + [a], None),
             ('label < 0', good_lo, [-5] + base[1:], None),
             ('label far outside', good_lo, base[:10] + [10 ** 6] + base[11:], None),
             ('length > max', good_lo, base, n + 1),
             ('length < 0', good_lo, base, -1),
             ('good again', good_lo, base, None)]
    x = np.repeat(_dyadic(rng, (1, t, a)), len(cases), axis=0)
    lo = np.stack([c[1] for c in cases])
    labels = [c[2] for c in cases]
    lens = [len(c[2]) if c[3] is None else c[3] for c in cases]
    # the reference's view of a bad label_lens: a transcript that cannot be aligned
    ref_labels = [c[2] if c[3] is None else [0] for c in cases]
    want = bref.align_batch_banded(x, [t] * len(cases), ref_labels, lo, w, 0, True, n)
    got = _launch(x, [t] * len(cases), labels, lo, w, lmax=n, lens=lens)
    _assert_equal(got, want, 'bad input')
    for b, c in enumerate(cases):
        bad = not c[0].startswith('good')
        assert (want[3][b] == -np.inf) == bad, c[0]
        assert bool((want[0][b] == -1).all()) == bad and bool((want[1][b] == -1).all()) == bad, c[0]
    assert want[3][0] == want[3][-1] and np.array_equal(want[0][0], want[0][-1])


def test_refusals():
    from ds2hip import lib
    x = np.zeros((1, 4, 3), dtype=np.float32)
    lo = np.zeros((1, 4))
    for band in (0, 63, 96, 2 * lib.ALIGN_BAND_MAX):
        with pytest.raises(lib.Ds2Error) as e:
            _launch(x, [4], [[1]], lo, band, ws=torch.zeros(1 << 16, dtype=torch.uint8, device='cuda'))
        assert e.value.code == lib.ERR_ARG and 'band %d' % band in str(e.value)
    with pytest.raises(lib.Ds2Error) as e:
        _launch(x, [4], [[1]], lo, 64, ws=torch.zeros(8, dtype=torch.uint8, device='cuda'))
    assert e.value.code == lib.ERR_ARG and 'workspace' in str(e.value)
    # 2 L + 1 states must fit an int32 (the outputs are never touched: the call is refused first)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device='cuda')       # noqa: E731
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device='cuda')
    f64 = torch.zeros(1, dtype=torch.float64, device='cuda')
    with pytest.raises(lib.Ds2Error) as e:
        lib.call('ds2_ctc_align_banded', torch.zeros((1, 4, 3), device='cuda'), i32(4), i32(1), i32(0), i32(1),
                 i32(0, 0, 0, 0), 1, 4, 3, 1 << 30, 64, 0, 1, ws, ws.numel(), i32(0, 0, 0, 0), i32(0), i32(0), f64)
    assert e.value.code == lib.ERR_ARG and 'max_label_len' in str(e.value)
    # a good call still works after the refusals
    _check_exact(x, [4], [[1]], lo, 64, 'after the refusals')


@pytest.mark.parametrize('t,n,w', [(2000, 800, 256), (746, 300, 1024)])
def test_rounded_probabilities(t, n, w):
    rng = np.random.default_rng(t)
    a = 29
    kinds = ('peaked', 'blank', 'random')
    labels = [_labels(rng, n, a) for _ in kinds]
    probs = np.stack([_softmax(_activations(rng, kind, t, a, lab)) for kind, lab in zip(kinds, labels)])
    sizes = [t, t, t - 3]
    s_n = 2 * n + 1
    lo = np.stack([np.resize(bref.diagonal(sz, s_n, w), t) for sz in sizes])
    got = _launch(probs, sizes, labels, lo, w, log_input=False)
    for b, lab in enumerate(labels):
        sz = sizes[b]
        logp = align_ref.frame_terms(probs[b, :sz], False)
        v_star, ref_states = bref.windowed(logp, lab, lo[b, :sz], w)
        assert np.isfinite(v_star)
        states = got[0][b]
        assert (states[sz:] == -1).all()
        assert align_ref.is_valid_path(states[:sz], n, lab), b
        assert bref.in_band(states[:sz], lo[b, :sz], w)
        assert align_ref.collapse(states[:sz], lab) == lab
        v_pi, abs_pi = align_ref.path_score(logp, states[:sz], lab)
        _, abs_ref = align_ref.path_score(logp, ref_states, lab)
        tol = 2.0 ** -21 * (abs_pi + abs_ref)                       # 4 fp32 ulp per frame term, on both paths
        print('b=%d T=%d L=%d W=%d V*=%.6f V(pi)=%.6f score=%.6f tol=%.3g same_path=%s' % (
            b, sz, n, w, v_star, v_pi, got[3][b], tol, np.array_equal(states[:sz], ref_states)))
        assert v_pi >= v_star - tol
        assert abs(float(got[3][b]) - v_pi) <= tol
        want_starts, want_ends = align_ref.spans(states[:sz], n)
        assert np.array_equal(got[1][b, :n], want_starts) and np.array_equal(got[2][b, :n], want_ends)


def drifting_path(n, t):
    """A state path that spells n labels in t frames at a speaking rate that drifts by +-25 % (piecewise linear in the label
    index, two periods): label l is spoken in ONE frame and followed by blanks up to the next label's frame.  -> (states (t,), label start frames (n,))."""
    l = np.arange(n)
    tri = 2.0 * np.abs(2.0 * ((2.0 * l / n) % 1.0) - 1.0) - 1.0    # 1 -> -1 -> 1, twice
    dur = 1.0 + 0.25 * tri
    at = np.floor(np.cumsum(dur) / dur.sum() * (t - 20)).astype(np.int64) + 5
    assert (np.diff(at) >= 1).all() and at[0] >= 1 and at[-1] < t - 1
    states = np.zeros(t, dtype=np.int64)
    for k in range(n):
        states[at[k]] = 2 * k + 1
        states[at[k] + 1:(at[k + 1] if k + 1 < n else t)] = 2 * k + 2
    return states, at


def path_probs(states, labels, a):
    sym = np.where(states & 1, np.asarray(labels)[np.minimum(states >> 1, len(labels) - 1)], 0)
    p = np.full((len(states), a), 0.1 / (a - 1), dtype=np.float32)
    p[np.arange(len(states)), sym] = 0.9
    return p


def test_long_aligner_widens_its_band_until_the_path_has_room():
    from codes.align import LongAligner, band_margin
    rng = np.random.default_rng(8)
    n, t, a = 3000, 8000, 29
    alphabet = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]
    labels = _labels(rng, n, a)
    for k in range(1, n):                                           # no adjacent repeats: a label may follow the last at once
        if labels[k] == labels[k - 1]:
            labels[k] = labels[k] % (a - 1) + 1
    states, at = drifting_path(n, t)
    probs = path_probs(states, labels, a)
    s_n = 2 * n + 1
    res = LongAligner(alphabet, band_states=64, band_margin=16).align(torch.from_numpy(probs).cuda(), labels)
    w = res['band_states']
    print('band_states %d margin %s score %.3f' % (w, res['band_margin'], res['score']))
    assert [s for _, s, _ in res['chars']] == at.tolist()           # every label starts where it was spoken
    assert np.array_equal(res['states'].cpu().numpy(), states) and res['states'].dtype == torch.int32
    assert 64 < w < s_n and w & (w - 1) == 0
    lo = bref.diagonal(t, s_n, w)
    assert res['band_margin'] == band_margin(states, lo, w, s_n) and res['band_margin'] >= 16
    # one width down the path had no room (that is why the aligner went on) ...
    narrow = band_margin(states, bref.diagonal(t, s_n, w // 2), w // 2, s_n)
    assert narrow is None or narrow < 16
    # ... and at the final width the banded optimum is the free one
    logp = align_ref.frame_terms(probs, False)
    banded, free = bref.windowed(logp, labels, lo, w), align_ref.viterbi(logp, labels)
    assert banded[0] == free[0] and np.array_equal(banded[1], free[1]) and np.array_equal(free[1], states)
    assert res['score'] == pytest.approx(free[0], rel=1e-6) and res['score_per_frame'] == pytest.approx(free[0] / t, rel=1e-6)
    assert ''.join(c for c, _, _ in res['chars']) == ''.join(alphabet[k] for k in labels)
    assert ' '.join(wd for wd, _, _ in res['words']) == ' '.join(''.join(alphabet[k] for k in labels).split())
