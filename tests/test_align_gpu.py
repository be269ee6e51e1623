"""``ds2_ctc_align`` on the GPU against the float64 host reference (tests/align_ref.py).

Exact cases: log inputs k/64 with integer |k| <= 2048 and some -inf, so every path sum is exact in fp32 and fp64 and the tie
rule decides alone: states, starts, ends and score must EQUAL the reference.  Rounded cases: probabilities, whose fp32 log
may legitimately pick another near-optimal path, so the path is judged (valid, within the rounding bound of the optimum),
not its identity.  The kernel stages emissions min(32, 1024 / A) frames at a time and walks its back-pointers 64 frames at
a time; the frame counts below sit on and around those lengths."""
import numpy as np
import pytest
import torch

from tests import align_ref

pytestmark = pytest.mark.gpu

CHUNK = {2: 32, 29: 32, 43: 23, 128: 8}          # frames per emission staging chunk, by alphabet size
BT_FRAMES = 64                                    # frames per back-trace window


def _launch(probs, sizes, labels_list, blank=0, log_input=True, lmax=None, ws=None):
    """One launch through ``ops.ctc_align`` (or, with ``ws``, through the C entry point on that workspace) -> numpy."""
    from ds2hip import lib, ops
    dev = 'cuda'
    lens = [len(v) for v in labels_list]
    lmax = max(lens + [0]) if lmax is None else lmax
    i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32).reshape(-1), dtype=torch.int32, device=dev)   # noqa: E731
    offs = np.cumsum([0] + lens[:-1])
    flat = [x for v in labels_list for x in v]
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).to(dev)
    args = (p, i32(sizes), i32(flat), i32(offs), i32(lens))
    if ws is None:
        out = ops.ctc_align(*args, lmax, blank, log_input)
    else:
        bsz, t, a = p.shape
        out = (torch.empty((bsz, t), dtype=torch.int32, device=dev), torch.empty((bsz, lmax), dtype=torch.int32, device=dev),
               torch.empty((bsz, lmax), dtype=torch.int32, device=dev), torch.empty((bsz,), device=dev))
        lib.call('ds2_ctc_align', *args, bsz, t, a, lmax, blank, int(log_input), ws, ws.numel(), *out)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ('states', 'starts', 'ends', 'score')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, g, w)           # (-inf == -inf; there is no NaN on either side)


def _dyadic(rng, shape, holes=0.0):
    x = (rng.integers(-2048, 2049, size=shape) / 64.0).astype(np.float32)
    if holes:
        x[rng.random(shape) < holes] = -np.inf
    return x


def _labels(rng, n, a, blank=0):
    ids = [k for k in range(a) if k != blank]
    return [int(v) for v in rng.choice(ids, size=n)]


def _repeats(labels):
    return sum(1 for x, y in zip(labels, labels[1:]) if x == y)


def _check_exact(probs, sizes, labels_list, what, blank=0, **kw):
    want = align_ref.align_batch(probs, sizes, labels_list, blank, True, kw.get('lmax'))
    got = _launch(probs, sizes, labels_list, blank, True, **kw)
    _assert_equal(got, want, what)
    return want


FRAMES = sorted({1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 22, 23, 24, 7, 8, 9, 127, 128, 129})


@pytest.mark.parametrize('a', [2, 29, 43, 128])
def test_exact_over_frame_counts(a):
    """Every frame count around the staging chunk (32, 23 or 8 frames) and the back-trace window (64), B = 4 of mixed
    transcript lengths; A = 2 has one label, so its transcripts are one repeated label."""
    rng = np.random.default_rng(a)
    assert {CHUNK[a] - 1, CHUNK[a], CHUNK[a] + 1, BT_FRAMES - 1, BT_FRAMES, BT_FRAMES + 1} <= set(FRAMES)
    feasible = 0
    for t in FRAMES:
        lens = [0, 1, min(t, 2), int(rng.integers(0, t // 2 + 2))]
        labels = [_labels(rng, n, a) for n in lens]
        x = _dyadic(rng, (4, t, a))
        if t > 3:                                                   # -inf holes for the second and the last utterance
            x[1::2][rng.random(x[1::2].shape) < 0.05] = -np.inf
        want = _check_exact(x, [t, t, t, t], labels, (a, t))
        feasible += int(np.isfinite(want[3]).sum())
    # without holes the empty transcript always aligns, and two labels (at worst one repeated) do from three frames on
    assert feasible >= 2 * len(FRAMES) - 2


@pytest.mark.parametrize('t', [3, 4, 5, 9])
def test_exact_with_every_staging_slot_in_use(t):
    """A = 256, the largest alphabet: a staging chunk is 4 frames of 256 floats, so every slot of the buffer and every load
    of a staging thread is in use; frame counts below, at and above one chunk and just above two.  B = 4 as in
    ``test_exact_over_frame_counts``."""
    a = 256
    rng = np.random.default_rng(a + t)
    lens = [0, 1, min(t, 2), int(rng.integers(0, t // 2 + 2))]
    labels = [_labels(rng, n, a) for n in lens]
    x = _dyadic(rng, (4, t, a))
    x[1::2][rng.random(x[1::2].shape) < 0.05] = -np.inf            # -inf holes for the second and the last utterance
    want = _check_exact(x, [t, t, t, t], labels, (a, t))
    assert np.isfinite(want[3][0])                                  # without holes the empty transcript always aligns


@pytest.mark.parametrize('n', [0, 1, 2, 127, 128, 255, 256, 511])
def test_exact_at_the_tightest_frame_count(n):
    """L labels need L + repeats frames: exactly that many (one path), one more, one fewer (no alignment), and a looser
    one with -inf holes.  L = 127 | 128, 255 | 256 and 511 sit on the 256 / 512 / 1024-thread instantiations' edges."""
    rng = np.random.default_rng(1000 + n)
    a = 43 if n % 2 else 29
    labels = _labels(rng, n, a)
    if n >= 2:
        labels[1] = labels[0]                                       # at least one adjacent repeat
    tight = n + _repeats(labels)
    loose = tight + n // 2 + 7
    x = _dyadic(rng, (4, loose, a))
    x[3][rng.random(x[3].shape) < 0.05] = -np.inf
    x[:, :, 0][rng.random(x[:, :, 0].shape) < 0.5] = 0.0            # (blank frames that tie with each other)
    sizes = [tight, tight + 1, tight - 1, loose]
    want = _check_exact(x, sizes, [labels] * 4, n)
    assert np.isfinite(want[3][0]) and np.isfinite(want[3][1])
    if n > 0:
        assert want[3][2] == -np.inf and (want[0][2] == -1).all() and (want[1][2] == -1).all()
    if n in (2, 128):                                               # one repeated label, at the tightest count and looser
        rep = [5] * n
        xs = _dyadic(rng, (3, 2 * n + 3, a))
        want = _check_exact(xs, [2 * n - 1, 2 * n - 2, 2 * n + 3], [rep] * 3, ('repeated', n))
        assert np.isfinite(want[3][0]) and want[3][1] == -np.inf


def test_longer_transcripts_and_small_workspaces_are_refused():
    from ds2hip import lib
    x = np.zeros((1, 4, 3), dtype=np.float32)
    with pytest.raises(lib.Ds2Error) as e:
        _launch(x, [4], [[1]], lmax=512)
    assert e.value.code == lib.ERR_ARG and '511' in str(e.value)
    with pytest.raises(lib.Ds2Error) as e:
        _launch(x, [4], [[1]], ws=torch.zeros(8, dtype=torch.uint8, device='cuda'))
    assert e.value.code == lib.ERR_ARG and 'workspace' in str(e.value)


def test_bad_label_ids_are_infeasible_not_read():
    """A label outside [0, A), or the blank, makes ITS utterance infeasible; the batch's others are untouched."""
    rng = np.random.default_rng(5)
    x = _dyadic(rng, (5, 20, 29))
    labels = [[3, 4, 5], [3, 29, 5], [3, -1, 5], [3, 0, 5], [3, 10 ** 6, 5]]
    want = _check_exact(x, [20] * 5, labels, 'bad labels')
    assert np.isfinite(want[3][0]) and (want[3][1:] == -np.inf).all() and (want[0][1:] == -1).all()
    _check_exact(x, [20] * 5, [[3, 4, 5], [3, 2, 5], [2], [], [7, 7]], 'blank 2', blank=2)


def test_exact_mixed_batch_with_nan_padding():
    """B = 17, sizes from 0 to T (and beyond: clamped), every frame past an utterance's size filled with NaN."""
    rng = np.random.default_rng(17)
    b, t, a = 17, 100, 29
    sizes = [0, 1, 2, 100, 120, -3] + [int(v) for v in rng.integers(3, 100, size=b - 6)]
    labels = [[], [4], [4, 4], _labels(rng, 40, a), _labels(rng, 50, a), [1]] + \
             [_labels(rng, int(rng.integers(0, 41)), a) for _ in range(b - 6)]
    x = _dyadic(rng, (b, t, a), holes=0.05)
    x[3][rng.random((t, a)) < 0.02] = np.nan                        # a NaN inside a valid frame counts as -inf
    for i, n in enumerate(sizes):
        x[i, min(max(n, 0), t):] = np.nan
    want = _check_exact(x, sizes, labels, 'mixed', lmax=60)
    assert np.isfinite(want[3]).sum() >= 8 and (want[3] == -np.inf).sum() >= 2


def test_exact_ties_everywhere():
    """All-equal emissions (every path of a transcript ties) and three-level ones (many ties): the tie rule alone names
    the path."""
    rng = np.random.default_rng(3)
    a, t = 29, 100
    labels = [[], [7], [7, 7, 7], _labels(rng, 20, a), _labels(rng, 49, a), [1, 2] * 25]
    flat = np.full((len(labels), t, a), -1.0, dtype=np.float32)
    want = _check_exact(flat, [t, t, t, t, 99, 100], labels, 'all equal')
    assert (want[3][:4] == np.float32([-100.0] * 4)).all()
    assert want[0][3][-1] == 40 and want[0][3][-21] == 40 and want[0][3][0] in (0, 1)       # final blank held to the end
    levels = rng.integers(-2, 1, size=flat.shape).astype(np.float32)
    _check_exact(levels, [t, t, t, 64, 65, 33], labels, 'levels')


def test_bitwise_independent_of_batch_company_and_workspace_contents():
    from ds2hip import lib
    rng = np.random.default_rng(11)
    t, a, n = 100, 29, 30
    mine, labels = rng.integers(-2, 1, size=(t, a)).astype(np.float32), _labels(rng, n, a)
    alone = _launch(mine[None], [t], [labels])
    _assert_equal(alone, align_ref.align_batch(mine[None], [t], [labels], 0, True), 'alone')
    others = _dyadic(rng, (5, t, a), holes=0.05)
    other_labels = [_labels(rng, k, a) for k in (0, 45, 3, 60, 50)]
    other_sizes = [100, 90, 2, 100, 0]
    for pos in range(5):
        x, lab, sz = others.copy(), list(other_labels), list(other_sizes)
        x[pos], lab[pos], sz[pos] = mine, labels, t
        st, sa, en, sc = _launch(x, sz, lab)
        assert np.array_equal(st[pos], alone[0][0]) and np.array_equal(sa[pos, :n], alone[1][0]) and \
            np.array_equal(en[pos, :n], alone[2][0]) and sc[pos].tobytes() == alone[3][0].tobytes(), pos
        assert (sa[pos, n:] == -1).all() and (en[pos, n:] == -1).all()
    # a second launch on a workspace full of other values (every byte the back-trace reads was written by this launch)
    ws = torch.empty(lib.query('ds2_ctc_align_ws_bytes', 1, t, n), dtype=torch.uint8, device='cuda')
    for fill in (0xFF, 0x01):
        ws.fill_(fill)
        _assert_equal(_launch(mine[None], [t], [labels], ws=ws), alone, 'workspace %#x' % fill)
    _assert_equal(_launch(mine[None], [t], [labels], ws=ws), alone, 'workspace reused')


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _activations(rng, kind, t, a, labels):
    x = rng.standard_normal((t, a))
    if kind == 'blank':                                             # early training: the blank dominates everywhere
        x[:, 0] += 6.0
    if kind == 'peaked':                                            # a trained model: the transcript spelled out, spread over T
        x *= 0.5
        x[:, 0] += 5.0
        at = np.sort(rng.choice(t, size=len(labels), replace=False)) if len(labels) <= t else []
        for f, k in zip(at, labels):
            x[f, k] += 9.0
    return x


def _check_rounded(probs, sizes, labels_list):
    got = _launch(probs, sizes, labels_list, log_input=False)
    for b, labels in enumerate(labels_list):
        n, k = int(sizes[b]), len(labels)
        logp = align_ref.frame_terms(probs[b, :n], False)
        v_star, ref_states = align_ref.viterbi(logp, labels)
        assert np.isfinite(v_star)
        states = got[0][b]
        assert (states[n:] == -1).all()
        assert align_ref.is_valid_path(states[:n], k, labels), b
        assert align_ref.collapse(states[:n], labels) == labels
        v_pi, abs_pi = align_ref.path_score(logp, states[:n], labels)
        _, abs_ref = align_ref.path_score(logp, ref_states, labels)
        tol = 2.0 ** -21 * (abs_pi + abs_ref)                       # 4 fp32 ulp per frame term, on both paths
        print('b=%d T=%d L=%d V*=%.6f V(pi)=%.6f score=%.6f tol=%.3g same_path=%s' % (
            b, n, k, v_star, v_pi, got[3][b], tol, np.array_equal(states[:n], ref_states)))
        assert v_pi >= v_star - tol
        assert abs(float(got[3][b]) - v_pi) <= tol + 2.0 ** -23 * abs(v_pi)
        want_starts, want_ends = align_ref.spans(states[:n], k)
        assert np.array_equal(got[1][b, :k], want_starts) and np.array_equal(got[2][b, :k], want_ends)
        assert (got[1][b, k:] == -1).all() and (got[2][b, k:] == -1).all()


def test_rounded_probabilities_t100():
    rng = np.random.default_rng(21)
    t, a = 100, 29
    kinds = ['random', 'blank', 'peaked'] * 2
    lens = [10, 10, 10, 45, 45, 45]
    labels = [_labels(rng, n, a) for n in lens]
    probs = np.stack([_softmax(_activations(rng, kind, t, a, lab)) for kind, lab in zip(kinds, labels)])
    _check_rounded(probs, [t, t, t, t, 97, 100], labels)


def test_rounded_probabilities_t746():
    rng = np.random.default_rng(22)
    t, a, n = 746, 29, 300
    labels = [_labels(rng, n, a) for _ in range(2)]
    probs = np.stack([_softmax(_activations(rng, kind, t, a, lab)) for kind, lab in zip(('peaked', 'random'), labels)])
    _check_rounded(probs, [t, t], labels)


def test_alignment_to_the_greedy_transcript_gives_the_greedy_offsets():
    """The greedy path is the best of ALL paths, so it is the best one that spells its own labelling: aligned to what
    ``GreedyDecoder.decode`` returns, every label starts at its greedy offset, and between one label's end and the next
    one's start the model wrote blanks only.  Zeros among the probabilities (log 0) leave no NaN."""
    from codes.align import ForcedAligner
    from codes.decoder import GreedyDecoder
    rng = np.random.default_rng(31)
    b, t, a = 4, 100, 29
    alphabet = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]
    x = rng.standard_normal((b, t, a))
    peak = np.where(rng.random((b, t)) < 0.6, 0, rng.integers(1, a, size=(b, t)))
    np.put_along_axis(x, peak[..., None], 8.0 + rng.random((b, t, 1)), axis=-1)
    probs = _softmax(x)
    probs[rng.random(probs.shape) < 0.1] = 0.0
    np.put_along_axis(probs, peak[..., None], np.take_along_axis(_softmax(x), peak[..., None], -1), axis=-1)
    sizes = [100, 100, 77, 64]
    dev = torch.from_numpy(probs).cuda()
    dec = GreedyDecoder(alphabet)
    strings, offsets = dec.decode(dev, torch.tensor(sizes, dtype=torch.int32))
    labels = [[int(v) for v in np.atleast_1d(dec.label_encoder.transform(list(s[0])))] if s[0] else [] for s in strings]
    assert min(len(v) for v in labels) > 10
    states, starts, ends, score = _launch(probs, sizes, labels, log_input=False)
    assert np.isfinite(score).all()
    best = probs.argmax(-1)
    for i, lab in enumerate(labels):
        k = len(lab)
        assert starts[i, :k].tolist() == offsets[i][0].tolist()
        assert (ends[i, :k] >= starts[i, :k]).all()
        for j in range(k - 1):
            assert (best[i, ends[i, j] + 1:starts[i, j + 1]] == 0).all()
            assert (states[i, ends[i, j] + 1:starts[i, j + 1]] == 2 * j + 2).all()
    # and through the aligner's own surface
    res = ForcedAligner(alphabet).align(dev, torch.tensor(sizes), torch.tensor([v for lab in labels for v in lab]),
                                        torch.tensor([len(v) for v in labels]))
    for i, r in enumerate(res):
        assert ''.join(c for c, _, _ in r['chars']) == strings[i][0]
        assert [s for _, s, _ in r['chars']] == offsets[i][0].tolist()
        assert ' '.join(w for w, _, _ in r['words']) == ' '.join(strings[i][0].split())
        assert r['score'] == pytest.approx(float(score[i])) and r['score_per_frame'] == pytest.approx(score[i] / sizes[i])
