"""N-best lists on the device (ds2_ctc_beam_search_nbest, csrc/ctc_beam.hip) against tests/nbest_ref.py: every row of every
utterance over the alphabet sizes, widths, N and blanks, spelled inputs with LMs and a context graph; exact ties in the final
ranking; row 0 and nbest = 1 bit for bit against the 1-best entries; fewer valid entries than N; the edges of the
back-trace and the launch; the ABI called directly; the decoder.  Every comparison with the reference asserts that the
reference's smallest gap over the cuts and the ranks exceeds TIE_GAP: the seeds were picked so that it does."""
import numpy as np
import pytest
import torch

from tests import beam_ref, bias_ref, nbest_ref
from tests.test_beam_edges_gpu import LABELS, TIE_GAP, _close, _make_lm, _softmax, _spell, _tie_probs

pytestmark = pytest.mark.gpu
SENT_I = -12345


def _graph(phrases, a, blank=0):
    from codes.bias import ContextGraph
    g = ContextGraph(phrases, a, blank)
    return g.trans, g.final


def _device(probs, sizes, w, n, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1, trans=None, final=None,
            weight=0.0):
    """ops.ctc_beam_search_nbest -> the seven outputs as numpy arrays (bias None without a graph)."""
    from ds2hip import ops
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    out = ops.ctc_beam_search_nbest(p, s, w, n, blank, log_input, lm, alpha, beta, space_id, dev(trans), dev(final), weight)
    torch.cuda.synchronize()
    return [None if x is None else x.cpu().numpy() for x in out]


def _reference(probs, sizes, w, n, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1, trans=None,
               final=None, weight=0.0, ties=None):
    """nbest_ref per utterance -> [(rows, count)], with the assertion every comparison makes: no near-tie at a cut or a rank,
    and (``ties`` None) no exact tie; a list collects the exact ties per utterance instead."""
    refs = []
    for b, size in enumerate(sizes):
        t = min(max(size, 0), probs.shape[1])
        stats = {}
        refs.append(nbest_ref.beam_search_nbest(beam_ref.frame_log_probs(probs[b, :t], log_input), blank, w, n, trans, final,
                                                weight, lm, alpha, beta, space_id, stats=stats))
        marks = stats['cut'] + stats['rank']
        assert min([gap for _, gap in marks], default=np.inf) > TIE_GAP, (b, 'a near-tie: the case does not decide the rule')
        if ties is None:
            assert not any(tie for tie, _ in marks), (b, 'an exact tie')
        else:
            ties.append(sum(tie for tie, _ in stats['rank']))
    return refs


def _compare(out, refs, n):
    """Every row of every utterance: labels, offsets, length, bias and count with ==, scores with _close, zeros past every
    length, and the rows past the count empty at -inf."""
    labels, offsets, lens, score, ctc, bias, count = out
    assert labels.shape[:2] == offsets.shape[:2] == lens.shape == score.shape == ctc.shape == (len(refs), n)
    for b, (rows, cnt) in enumerate(refs):
        assert count[b] == cnt, (b, int(count[b]), cnt)
        for r in range(n):
            m = lens[b, r]
            assert not labels[b, r, m:].any() and not offsets[b, r, m:].any(), (b, r)
            if r >= cnt:
                assert m == 0 and np.isneginf(score[b, r]) and np.isneginf(ctc[b, r]), (b, r)
                assert bias is None or bias[b, r] == 0
                continue
            ref = rows[r]
            assert labels[b, r, :m].tolist() == ref[0], (b, r)
            assert offsets[b, r, :m].tolist() == ref[1], (b, r)
            assert bias is None or bias[b, r] == ref[4], (b, r)
            assert _close(score[b, r], ref[2]) and _close(ctc[b, r], ref[3]), (b, r, float(score[b, r]), ref[2])


# ------------------------------------------------------------------------------------------ 1. against the reference
RANDOM_CASES = [(5, 2, 2, 4), (5, 16, 16, 0), (5, 128, 128, 2), (29, 16, 4, 14), (29, 128, 65, 0), (128, 16, 16, 0),
                (128, 128, 5, 64)]


def random_case(a, w, blank):
    """Random frames and random phrases over the alphabet (the shapes of test_bias_gpu.random_case): T = 24 / 12 / 7,
    sizes [T, T-3, 1] -> (probs, sizes, phrases, weight)."""
    rng = np.random.default_rng(1000 * a + 10 * w + blank)
    t = 24 if w * a <= 512 else (12 if w * a <= 4096 else 7)
    labels = [c for c in range(a) if c != blank]
    phrases = set()
    while len(phrases) < 6:
        phrases.add(tuple(int(c) for c in rng.choice(labels[:6], size=rng.integers(1, 5))))
    x = rng.standard_normal((3, t, a)) * 2.0
    if a > 6:
        x[..., labels[:6] + [blank]] += 3.0
    return _softmax(x), [t, t - 3, 1], sorted(phrases), 0.75


@pytest.mark.parametrize('boost', [False, True])
@pytest.mark.parametrize('a, w, n, blank', RANDOM_CASES)
def test_random_inputs_against_the_reference(a, w, n, blank, boost):
    probs, sizes, phrases, weight = random_case(a, w, blank)
    kw = dict(blank=blank)
    if boost:
        trans, final = _graph(phrases, a, blank)
        kw.update(trans=trans, final=final, weight=weight)
    refs = _reference(probs, sizes, w, n, **kw)
    out = _device(probs, sizes, w, n, **kw)
    _compare(out, refs, n)
    assert (out[5] is not None) == boost
    if boost:
        assert any(row[4] > 0 for rows, _ in refs for row in rows)
    if w >= 16:
        assert refs[0][1] == n                                             # the list is full where the beam is


SPELLED = ['THE CAT SEES A BIRD', 'ABC DOG ABCD', 'THE CATS RUN', 'A BIR DOG CA']
SPELLED_PHRASES = ['CAT', 'CATS', 'BIRDS', 'AB', 'BC', 'THE', 'THE CAT', ' A ', 'DOGS']
SPELLED_SIZES = [48, 48, 41, 30]


def spelled_case(seed):
    rng = np.random.default_rng(seed)
    probs = np.stack([_spell(rng, s, 48, 29, noise=0.6) for s in SPELLED])
    return probs, SPELLED_SIZES, [[LABELS.index(c) for c in p] for p in SPELLED_PHRASES]


@pytest.fixture(scope='module')
def lms(tmp_path_factory):
    d = tmp_path_factory.mktemp('nbest_lm')
    return {'char': _make_lm(d, 3, 'char')[0], 'word': _make_lm(d, 2, 'word')[0]}


SPELLED_KINDS = ['char', 'word', 'graph']


def spelled_kw(kind, lms, phrases):
    if kind == 'graph':
        trans, final = _graph(phrases, 29)
        return dict(trans=trans, final=final, weight=1.25)
    return dict(lm=lms[kind], alpha=0.6, beta=0.9, space_id=1)


@pytest.mark.parametrize('kind', SPELLED_KINDS)
def test_spelled_inputs_against_the_reference(lms, kind):
    probs, sizes, phrases = spelled_case(23)
    kw = spelled_kw(kind, lms, phrases)
    refs = _reference(probs, sizes, 16, 16, **kw)
    _compare(_device(probs, sizes, 16, 16, **kw), refs, 16)
    assert all(cnt == 16 for _, cnt in refs)
    if kind == 'graph':
        assert refs[0][0][0][4] >= 3                                        # CAT at the least


# ---------------------------------------------------------------------------------------- 2. exact ties in the ranking
@pytest.mark.parametrize('w', [4, 16, 64])
def test_exact_ties_in_the_final_ranking(w):
    rng = np.random.default_rng(w + 3)
    probs = _tie_probs(rng, 3, 30, 29, [[4, 5], [8, 9, 10]], 0.0)
    sizes = [30, 30, 17]
    ties = []
    refs = _reference(probs, sizes, w, w, ties=ties)
    assert sum(ties) >= 3, ties
    out = _device(probs, sizes, w, w)
    _compare(out, refs, w)                                                  # the tied rows in slot order, as the reference
    for b, (rows, cnt) in enumerate(refs):
        for r in range(cnt - 1):
            if rows[r][2] == rows[r + 1][2]:
                assert out[3][b, r] == out[3][b, r + 1] and out[4][b, r] == out[4][b, r + 1], (b, r)
                assert out[0][b, r].tolist() != out[0][b, r + 1].tolist()
    again = _device(probs, sizes, w, w)
    for x, y in zip(out, again):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8))


# --------------------------------------------------------------------------------- 3. row 0 against the 1-best entries
@pytest.mark.parametrize('unit', [None, 'char', 'word'])
@pytest.mark.parametrize('boost', [False, True])
def test_row_0_and_nbest_1_are_the_shipped_entries(lms, unit, boost):
    from ds2hip import ops
    probs, sizes, phrases = spelled_case(3)
    probs = np.concatenate([probs, np.zeros_like(probs[:1])])               # and an impossible utterance
    sizes = sizes + [20]
    p = torch.from_numpy(probs).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    lm_kw = (lms[unit], 0.6, 0.9, 1) if unit else (None, 0.0, 0.0, -1)
    trans = final = None
    if boost:
        trans, final = [torch.from_numpy(x).cuda() for x in _graph(phrases, 29)]
        want = ops.ctc_beam_search_bias(p, s, 16, trans, final, 1.25, 0, False, *lm_kw)
    else:
        want = ops.ctc_beam_search(p, s, 16, 0, False, *lm_kw)
    for n in (1, 16):
        got = ops.ctc_beam_search_nbest(p, s, 16, n, 0, False, *lm_kw, trans, final, 1.25)
        assert got[0].shape == (5, n, 48) and got[2].shape == (5, n) and got[6].shape == (5,)
        for k, x in enumerate(want):
            assert x.dtype == got[k].dtype and torch.equal(got[k][:, 0].contiguous().view(torch.int32), x.view(torch.int32)), (n, k)
        assert (got[5] is None) == (not boost)
        assert got[6].tolist() == [n] * 4 + [0]


# ------------------------------------------------------------------------------------------ 4. fewer valid than N
def test_fewer_valid_entries_than_n():
    rng = np.random.default_rng(12)
    probs = _softmax(rng.standard_normal((3, 4, 3)) * 1.5)
    probs[2, 2] = 0.0                                                       # an all-zero frame: nothing is possible
    sizes = [1, 0, 4]
    refs = _reference(probs, sizes, 16, 16)
    out = _device(probs, sizes, 16, 16)
    _compare(out, refs, 16)
    assert 1 <= out[6][0] <= 3 and out[6][0] == refs[0][1] == 3
    assert out[6][1] == 1 and out[2][1, 0] == 0 and out[3][1, 0] == 0.0 and out[4][1, 0] == 0.0     # the empty labelling at 0
    assert out[6][2] == 0 and np.isneginf(out[3][2]).all() and np.isneginf(out[4][2]).all() and not out[2][2].any()


def test_sizes_are_clamped():
    rng = np.random.default_rng(4)
    probs = _softmax(rng.standard_normal((4, 20, 29)) * 2.0)
    out = _device(probs, [25, -3, 20, 1 << 30], 16, 8)
    want = _device(probs, [20, 0, 20, 20], 16, 8)
    for x, y in zip(out, want):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert out[6].tolist() == [8, 1, 8, 8]
    _compare(want, _reference(probs, [20, 0, 20, 20], 16, 8), 8)


# ---------------------------------------------------------------------------- 5. edges of the back-trace and the launch
def test_one_label_per_frame_pair():
    t = 48
    text = 'THE CAT SEES A BIRD RUNS'                                       # 24 labels, one per frame pair
    rng = np.random.default_rng(48)
    probs = _spell(rng, text, t, 29, noise=0.3)[None]
    refs = _reference(probs, [t], 16, 16)
    assert len(refs[0][0][0][0]) == 24 and refs[0][0][0][1][-1] == 46          # the chain is as long as it can be at this T
    _compare(_device(probs, [t], 16, 16), refs, 16)


@pytest.mark.parametrize('n', [65, 128])
def test_the_second_wave_traces(n):
    rng = np.random.default_rng(n)
    probs = _softmax(rng.standard_normal((2, 12, 9)) * 1.5)
    sizes = [12, 9]
    refs = _reference(probs, sizes, 128, n)
    assert all(cnt == n for _, cnt in refs) and max(len(r[0]) for r in refs[0][0][64:]) >= 3
    _compare(_device(probs, sizes, 128, n), refs, n)


def test_three_hundred_utterances():
    rng = np.random.default_rng(300)
    probs = _softmax(rng.standard_normal((300, 6, 5)) * 2.0)
    sizes = [6 - (b % 4) for b in range(300)]
    _compare(_device(probs, sizes, 4, 4), _reference(probs, sizes, 4, 4), 4)


def test_a_long_utterance():
    rng = np.random.default_rng(746)
    probs = _softmax(rng.standard_normal((1, 746, 29)) * 2.5)
    refs = _reference(probs, [746], 16, 16)
    assert refs[0][1] == 16 and len(refs[0][0][0][0]) > 200
    _compare(_device(probs, [746], 16, 16), refs, 16)


# ------------------------------------------------------------------------------------------------ 6. the ABI, directly
def _abi_call(probs, sizes, w, n, lm=None, alpha=0.0, beta=0.0, space_id=-1, trans=None, final=None, weight=0.0, pad=64,
              ws_fill=0):
    """ds2_ctc_beam_search_nbest called directly.  Every output is ``pad`` elements longer than it needs to be and
    pre-filled with a sentinel, the workspace with ``ws_fill``.  -> the seven outputs (bias all sentinel without a graph),
    their tails checked."""
    from ds2hip import lib
    from tests.test_bias_gpu import _lm_args
    b, t, a = probs.shape
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda() if b else torch.zeros(1, dtype=torch.int32).cuda()
    ints = [torch.full((m + pad,), SENT_I, dtype=torch.int32, device='cuda') for m in (b * n * t, b * n * t, b * n, b * n, b)]
    flts = [torch.full((b * n + pad,), float('nan'), dtype=torch.float32, device='cuda') for _ in range(2)]
    ws_bytes = lib.query('ds2_ctc_beam_ws_bytes', b, t, w)
    ws = torch.full((ws_bytes + 16,), ws_fill, dtype=torch.uint8, device='cuda')
    lm_args, keep = _lm_args(lm, p.device, alpha, beta, space_id)
    if trans is None:
        bias_args = (None, None, 0, float(weight))
    else:
        tabs = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in (trans, final)]
        bias_args = (tabs[0], tabs[1], len(final), float(weight))
    lib.call('ds2_ctc_beam_search_nbest', p if p.numel() else torch.zeros(1, device='cuda'), s, b, t, a, 0, w, 0, *lm_args,
             *bias_args, n, ws, ws_bytes, ints[0], ints[1], ints[2], flts[0], flts[1], ints[3], ints[4])
    torch.cuda.synchronize()
    labels, offsets, lens, bias, count = [x.cpu().numpy() for x in ints]
    score, ctc = [x.cpu().numpy() for x in flts]
    assert all((x[m:] == SENT_I).all() for x, m in ((labels, b * n * t), (offsets, b * n * t), (lens, b * n), (bias, b * n),
                                                    (count, b))), 'written past'
    assert np.isnan(score[b * n:]).all() and np.isnan(ctc[b * n:]).all(), 'written past (B,N)'
    return (labels[:b * n * t].reshape(b, n, t), offsets[:b * n * t].reshape(b, n, t), lens[:b * n].reshape(b, n),
            score[:b * n].reshape(b, n), ctc[:b * n].reshape(b, n), bias[:b * n].reshape(b, n), count[:b])


@pytest.mark.parametrize('kind', [None, 'word', 'graph'])
def test_a_row_does_not_depend_on_its_company(lms, kind):
    rng = np.random.default_rng(5)
    sizes = [40, 1, 0, 48, 23, 48, 9]
    texts = ['THE CAT SEES', 'A', '', 'ABC THE CATS BIRD', 'DOGS RUN', 'A BIRD SEES THE CAT', 'CAT']
    probs = np.full((len(sizes), 48, 29), np.nan, np.float32)                # NaN past sizes[b]: never read
    for b, m in enumerate(sizes):
        probs[b, :m] = _spell(rng, texts[b], 48, 29, noise=1.2)[:m]
    phrases = [[LABELS.index(c) for c in p] for p in SPELLED_PHRASES]
    kw = spelled_kw(kind, lms, phrases) if kind else {}
    n = 8
    batch = _abi_call(probs, sizes, 16, n, **kw)
    if kind == 'graph':
        assert batch[5].any() and (batch[5] != SENT_I).all()
    else:
        assert (batch[5] == SENT_I).all()                                    # no graph: out_bias is not written
    assert batch[6][2] == 1 and batch[2][2, 0] == 0 and batch[4][2, 0] == 0.0
    moved = _abi_call(probs, sizes, 16, n, ws_fill=255, **kw)                # another workspace content: the same bits
    for x, y in zip(batch, moved):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for b, m in enumerate(sizes):                                            # alone, with T cut to its own length
        alone = _abi_call(probs[b:b + 1, :m], [m], 16, n, ws_fill=170, **kw)
        assert alone[6][0] == batch[6][b] and np.array_equal(alone[2][0], batch[2][b])
        assert np.array_equal(alone[0][0], batch[0][b, :, :m]) and np.array_equal(alone[1][0], batch[1][b, :, :m])
        for k in (3, 4, 5):
            assert np.array_equal(alone[k][0].view(np.uint32), batch[k][b].view(np.uint32)), (b, k)
    out = list(batch)
    if kind != 'graph':
        out[5] = None
    _compare(out, _reference(np.nan_to_num(probs, nan=0.0), sizes, 16, n, **kw), n)
    none = _abi_call(probs[:0], [], 16, n, **kw)                             # B = 0: nothing is written
    assert all(x.size == 0 for x in none)


# --------------------------------------------------------------------------------------------- 7. decoder, integration
def test_decoder_nbest(lms):
    from codes.bias import PhraseBooster
    from codes.decoder import DeviceBeamCTCDecoder
    probs, sizes, _ = spelled_case(3)
    probs = np.concatenate([probs, np.zeros_like(probs[:1])])               # an impossible input keeps its one empty string
    p = torch.from_numpy(probs).cuda()
    s = torch.tensor(sizes + [20], dtype=torch.int32)
    for kw in (dict(), dict(lm=lms['word'], alpha=0.6, beta=0.9), dict(booster=PhraseBooster(LABELS, ['CAT', 'THE']))):
        one = DeviceBeamCTCDecoder(LABELS, beam_width=16, **kw)
        four = DeviceBeamCTCDecoder(LABELS, beam_width=16, nbest=4, **kw)
        want, want_off = one.decode(p, s)
        got, got_off = four.decode(p, s)
        assert one.last_nbest_scores is None and one.last_nbest_posteriors is None
        assert [len(g) for g in got] == [4, 4, 4, 4, 1] and got[4] == [''] == want[4]
        for b in range(5):
            assert got[b][0] == want[b][0] and got_off[b][0].tolist() == want_off[b][0].tolist()
            assert len(set(got[b])) == len(got[b])
            assert all(len(o) == len(t_) for o, t_ in zip(got_off[b], got[b]))
            fields = [four.last_nbest_scores[b], four.last_nbest_ctc_log_probs[b], four.last_nbest_posteriors[b]]
            if 'booster' in kw:
                fields.append(four.last_nbest_bias_counts[b])
                assert four.last_bias_counts[b] == four.last_nbest_bias_counts[b][0]
            assert all(len(f) == len(got[b]) for f in fields)
            sc = four.last_nbest_scores[b]
            assert all(x >= y for x, y in zip(sc, sc[1:]))
            post = four.last_nbest_posteriors[b]
            if b < 4:
                assert abs(sum(post) - 1.0) <= 1e-12 and all(x >= y for x, y in zip(post, post[1:])) and post[-1] > 0.0
                assert post == DeviceBeamCTCDecoder.nbest_posteriors(sc)
            else:
                assert post == [0.0] and sc == [float('-inf')]
        assert four.last_scores == one.last_scores and four.last_ctc_log_probs == one.last_ctc_log_probs
        assert four.last_bias_counts == one.last_bias_counts
        if 'booster' not in kw:
            assert four.last_nbest_bias_counts is None


def test_decode_labels_nbest_through_edit_stats(lms):
    from codes.decoder import DeviceBeamCTCDecoder
    from ds2hip import ops
    probs, sizes, _ = spelled_case(3)
    probs = np.concatenate([probs, np.zeros_like(probs[:1])])
    p = torch.from_numpy(probs).cuda()
    s = torch.tensor(sizes + [20], dtype=torch.int32)
    refs = ['THE CAT SEES A BIRD', 'ABC DOGS', 'THE CAT RUNS', 'A BIRD', 'CAT']
    n, bsz = 4, 5
    dec = DeviceBeamCTCDecoder(LABELS, beam_width=16, lm=lms['word'], alpha=0.6, beta=0.9, nbest=n)
    labels, lens, count = dec.decode_labels_nbest(p, s)
    assert dec.last_scores is None and dec.last_nbest_scores is None         # no last_* field is touched
    assert labels.is_cuda and labels.shape == (bsz, n, 48) and lens.shape == (bsz, n) and count.shape == (bsz,)
    assert labels.dtype == lens.dtype == count.dtype == torch.int32
    flat = torch.tensor([LABELS.index(c) for r in refs for c in r], dtype=torch.int32).cuda()
    rl = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    offs = (torch.cumsum(rl, 0) - rl).int().cuda()
    ref_index = (torch.arange(bsz * n, dtype=torch.int32) // n).int().cuda()
    stats = ops.edit_stats(labels.view(bsz * n, 48), lens.view(bsz * n), flat, offs, rl.cuda(), int(rl.max()), 1,
                           ref_index=ref_index).view(bsz, n, 10)
    big = torch.iinfo(torch.int32).max
    live = torch.arange(n, device='cuda')[None, :] < count.clamp(min=1)[:, None]     # row 0 stands for an empty list
    char_min = torch.where(live, stats[..., 0], big).min(1).values.cpu().tolist()
    word_min = torch.where(live, stats[..., 5], big).min(1).values.cpu().tolist()
    strings, _ = dec.decode(p, s)
    assert [len(x) for x in strings] == count.clamp(min=1).cpu().tolist()
    assert word_min == [min(dec.wer(h, r) for h in strings[b]) for b, r in enumerate(refs)]
    assert char_min == [min(dec.cer(h, r) for h in strings[b]) for b, r in enumerate(refs)]
    assert sum(word_min) <= sum(dec.wer(strings[b][0], r) for b, r in enumerate(refs))
