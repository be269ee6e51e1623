"""Phrase boosting on the device (ds2_ctc_beam_search_bias, csrc/ctc_beam.hip) against tests/bias_ref.py: random and spelled
inputs over the alphabet sizes, beam widths, blanks and LM kinds; exactly summable inputs whose fused scores are compared
with ==; every labelling enumerated; graphs that must change nothing; independence of a row from its company, from the
workspace and from where the tables stand; and a table whose next states point outside it.  Every comparison with the
reference asserts that the reference's smallest gap exceeds TIE_GAP: the seeds were picked so that it does."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import beam_ref, bias_ref
from tests.test_beam_edges_gpu import LABELS, TIE_GAP, _close, _make_lm, _moved_blank, _softmax, _spell

pytestmark = pytest.mark.gpu


def _graph(phrases, a, blank=0):
    from codes.bias import ContextGraph
    g = ContextGraph(phrases, a, blank)
    return g.trans, g.final


def _lm_args(lm, device, alpha, beta, space_id):
    if lm is None:
        return (None, 0, None, 0, 1, 0, -1, -1, -1, -1, 0.0, 0.0, 0.0), {}
    tabs = lm.to(device)
    word = tabs.get('word')
    return (tabs['ngram'], tabs['ngram'].shape[0], word, 0 if word is None else word.shape[0], lm.order,
            1 if lm.unit == 'char' else 2, lm.bos_id, lm.eos_id, lm.hist_unk_id, space_id, float(alpha), float(beta),
            float(lm.oov_logp)), tabs


def _device(probs, sizes, w, trans, final, weight, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    from ds2hip import ops
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    out = ops.ctc_beam_search_bias(p, s, w, torch.from_numpy(np.ascontiguousarray(trans)).cuda(),
                                   torch.from_numpy(np.ascontiguousarray(final)).cuda(), weight, blank, log_input, lm,
                                   alpha, beta, space_id)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _reference(probs, sizes, w, trans, final, weight, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    """bias_ref per utterance, with the assertion every comparison makes: no exact tie and no near-tie at a cut or pick."""
    refs = []
    for b, size in enumerate(sizes):
        n = min(max(size, 0), probs.shape[1])
        stats = {}
        refs.append(bias_ref.beam_search_bias(beam_ref.frame_log_probs(probs[b, :n], log_input), blank, w, trans, final,
                                              weight, lm, alpha, beta, space_id, stats=stats))
        marks = stats['cut'] + [stats['pick']]
        assert min(gap for _, gap in marks) > TIE_GAP, (b, 'a near-tie: the case does not decide the rule')
        assert not any(tie for tie, _ in marks), (b, 'an exact tie')
    return refs


def _compare(out, refs, exact_scores=False):
    labels, offsets, lens, score, ctc, bias = out
    for b, ref in enumerate(refs):
        assert labels[b, :lens[b]].tolist() == ref[0], b
        assert offsets[b, :lens[b]].tolist() == ref[1], b
        assert bias[b] == ref[4], (b, int(bias[b]), ref[4])
        if exact_scores:
            assert float(score[b]) == float(np.float32(ref[2])) and float(ctc[b]) == float(np.float32(ref[3])), b
        assert _close(score[b], ref[2]) and _close(ctc[b], ref[3]), (b, float(score[b]), ref[2], float(ctc[b]), ref[3])
        assert not labels[b, lens[b]:].any() and not offsets[b, lens[b]:].any()


# ------------------------------------------------------------------------------------------ 1. against the reference
def random_case(a, w, blank):
    """Random frames and random phrases over the alphabet: (probs, sizes, phrases, weight)."""
    rng = np.random.default_rng(1000 * a + 10 * w + blank)
    t = 24 if w * a <= 512 else (12 if w * a <= 4096 else 7)
    bsz = 3 if w * a <= 4096 else 2
    labels = [c for c in range(a) if c != blank]
    phrases = set()
    while len(phrases) < 6:
        phrases.add(tuple(int(c) for c in rng.choice(labels[:6], size=rng.integers(1, 5))))
    x = rng.standard_normal((bsz, t, a)) * 2.0
    if a > 6:
        x[..., labels[:6] + [blank]] += 3.0                      # the phrases' labels are likely enough to be spelled
    return _softmax(x), [t, t - 3, 1][:bsz], sorted(phrases), 0.75


RANDOM_CASES = [(5, 1, 0), (5, 2, 4), (5, 16, 0), (5, 128, 2), (29, 1, 0), (29, 2, 28), (29, 16, 14), (29, 128, 0),
                (128, 2, 127), (128, 16, 0), (128, 128, 64)]


@pytest.mark.parametrize('a, w, blank', RANDOM_CASES)
def test_random_inputs_against_the_reference(a, w, blank):
    probs, sizes, phrases, weight = random_case(a, w, blank)
    trans, final = _graph(phrases, a, blank)
    refs = _reference(probs, sizes, w, trans, final, weight, blank)
    assert any(r[4] > 0 for r in refs)
    _compare(_device(probs, sizes, w, trans, final, weight, blank), refs)


SPELLED = ['THE CAT SEES A BIRD', 'ABC DOG ABCD', 'THE CATS RUN', 'A BIR DOG CA']
SPELLED_PHRASES = ['CAT', 'CATS', 'BIRDS', 'AB', 'BC', 'THE', 'THE CAT', ' A ', 'DOGS']       # whole, partly, overlapping, nested


def spelled_case(labels, blank, seed):
    rng = np.random.default_rng(seed)
    probs = np.stack([_spell(rng, s, 48, 29, noise=0.6, labels=labels, blank=blank) for s in SPELLED])
    phrases = [[labels.index(c) for c in p] for p in SPELLED_PHRASES]
    return probs, [48, 48, 41, 30], phrases


@pytest.fixture(scope='module')
def lms(tmp_path_factory):
    return make_lms(tmp_path_factory.mktemp('bias_lm'), tmp_path_factory.mktemp('bias_lm_moved'))


def make_lms(d, d_moved):
    """A char 3-gram and a word 2-gram over LABELS, and the char 3-gram for the alphabet with the blank at 14."""
    return {('char', 0): _make_lm(d, 3, 'char')[0], ('word', 0): _make_lm(d, 2, 'word')[0],
            ('char', 14): _make_lm(d_moved, 3, 'char', _moved_blank(14), blank=14)[0]}


@pytest.mark.parametrize('unit, blank', [(None, 0), ('char', 0), ('word', 0), (None, 14), ('char', 14)])
@pytest.mark.parametrize('w', [2, 16])
def test_spelled_inputs_against_the_reference(lms, unit, blank, w):
    labels = _moved_blank(blank) if blank else LABELS
    lm = lms[(unit, blank)] if unit else None
    probs, sizes, phrases = spelled_case(labels, blank, 7 + w)
    trans, final = _graph(phrases, 29, blank)
    kw = dict(blank=blank, lm=lm, alpha=0.6, beta=0.9, space_id=labels.index(' '))
    refs = _reference(probs, sizes, w, trans, final, 1.25, **kw)
    _compare(_device(probs, sizes, w, trans, final, 1.25, **kw), refs)
    if w == 16:
        plain = [beam_ref.beam_search(beam_ref.frame_log_probs(probs[b, :n], False), blank, w, lm, 0.6, 0.9,
                                      labels.index(' ')) for b, n in enumerate(sizes)]
        assert any(p[0] != r[0] for p, r in zip(plain, refs))               # the boost does change a transcript
        assert refs[0][4] >= 7 and refs[1][4] >= 2                          # THE CAT, and AB of ABC


# ------------------------------------------------------------------------------------- 2. exactly summable log-inputs
def _summable():
    """blank C A B T S; four frames, every labelling with ONE alignment (the rest is -inf), log-probs multiples of 2^-10."""
    blank, C, A, B, T, S = range(6)
    lp = np.full((1, 4, 6), -np.inf, np.float32)
    lp[0, 0, C], lp[0, 1, A], lp[0, 2, T], lp[0, 2, B], lp[0, 3, blank] = -0.125, -0.25, -0.5, -1.0, -37.0 / 1024
    return lp, (C, A, B, T, S)


@pytest.mark.parametrize('w', [1, 2, 16, 128])
def test_exactly_summable_inputs(w):
    lp, (C, A, B, T, S) = _summable()
    base = -0.125 - 0.25 - 37.0 / 1024
    cat, cab = [C, A, T], [C, A, B]
    for phrases, weight, want, want_bias, want_score in (
            ([[S]], 0.75, cat, 0, base - 0.5),                               # nothing boosted that occurs: CAT
            ([cab], 0.25, cab, 3, base - 1.0 + 0.75),                        # CAB boosted past the gap of 0.5
            ([cab], 0.125, cat, 0, base - 0.5),                              # ... and not past it
            ([cab + [S]], 0.25, cat, 0, base - 0.5),                         # the partial credit of CABS is revoked
            ([cab + [S], [C]], 0.375, cat, 1, base - 0.5 + 0.375)):          # ... down to the complete C
        trans, final = _graph(phrases, 6)
        if w == 1 and phrases[0] == cab + [S]:
            # a beam of one follows the pending credit and cannot come back: CAB with what F leaves of it
            want, want_score = cab, base - 1.0 + weight * want_bias
        refs = _reference(lp, [4], w, trans, final, weight, log_input=True)
        out = _device(lp, [4], w, trans, final, weight, log_input=True)
        _compare(out, refs, exact_scores=True)
        assert refs[0][0] == want and refs[0][4] == want_bias and refs[0][2] == want_score, (phrases, weight, refs[0])
        assert float(out[3][0]) == want_score and int(out[5][0]) == want_bias


# -------------------------------------------------------------------------------------------------- 3. exhaustive
def _ctc_of_every_labelling(lp, blank):
    """{labelling: log p} over every path, fp64."""
    t, a = len(lp), len(lp[0])
    tot = {}
    for path in itertools.product(range(a), repeat=t):
        y = tuple(c for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1]))
        tot[y] = beam_ref.log_add(tot.get(y, beam_ref.NEG_INF), sum(lp[k][c] for k, c in enumerate(path)))
    return tot


def exhaustive_case(t, a):
    rng = np.random.default_rng(50 * t + a)
    probs = _softmax(rng.standard_normal((4, t, a)) * 1.5)
    phrases = [[1, 2], [2, 1, 1], [a - 1]] if a > 3 else [[1, 2], [2, 1, 1]]
    return probs, phrases, 1.5


@pytest.mark.parametrize('t, a', [(4, 3), (4, 4), (5, 3), (5, 4)])
def test_the_best_labelling_of_all(t, a):
    probs, phrases, weight = exhaustive_case(t, a)
    trans, final = _graph(phrases, a)
    out = _device(probs, [t] * 4, 128, trans, final, weight)
    _compare(out, _reference(probs, [t] * 4, 128, trans, final, weight))
    boosted = 0
    for b in range(4):
        every = _ctc_of_every_labelling(beam_ref.frame_log_probs(probs[b], False), 0)
        ranked = sorted(((lp + weight * bias_ref.F(y, phrases), y) for y, lp in every.items()), reverse=True)
        assert ranked[0][0] - ranked[1][0] >= 1e-6, b
        got = tuple(out[0][b, :out[2][b]].tolist())
        assert got == ranked[0][1], (b, got, ranked[:2])
        assert _close(out[3][b], ranked[0][0]) and out[5][b] == bias_ref.F(got, phrases)
        boosted += got != max(every, key=every.get)
    assert boosted >= 1                                              # the boost decides at least one of the four


# -------------------------------------------------------------------------------------------------- 4. no-op graphs
@pytest.mark.parametrize('unit', [None, 'char', 'word'])
def test_graphs_that_change_nothing(lms, unit):
    from ds2hip import ops
    lm = lms[(unit, 0)] if unit else None
    probs, sizes, phrases = spelled_case(LABELS, 0, 3)
    p = torch.from_numpy(probs).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    want = [x.cpu().numpy() for x in ops.ctc_beam_search(p, s, 16, 0, False, lm, 0.6, 0.9, 1)]
    root = np.zeros((1, 29), np.int32), np.zeros(1, np.int32)
    real = _graph(phrases, 29)
    for (trans, final), weight in ((root, 2.0), (real, 0.0)):
        got = _device(probs, sizes, 16, trans, final, weight, lm=lm, alpha=0.6, beta=0.9, space_id=1)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32))
    assert not _device(probs, sizes, 16, root[0], root[1], 2.0)[5].any()
    counts = _device(probs, sizes, 16, real[0], real[1], 0.0, lm=lm, alpha=0.6, beta=0.9, space_id=1)[5]
    assert counts.tolist() == [bias_ref.F(want[0][b, :want[2][b]].tolist(), phrases) for b in range(4)] and counts.any()


# -------------------------------------------------------------------------------------------------- 5. independence
SENT_I = -12345


def _abi_call(probs, sizes, w, trans, final, weight, lm=None, alpha=0.0, beta=0.0, space_id=-1, pad=64, ws_fill=0,
              table_offset=0, n_states=None, table_tail=0, tail_fill=0):
    """ds2_ctc_beam_search_bias called directly.  Every output is ``pad`` elements longer than it needs to be and pre-filled
    with a sentinel; the workspace is pre-filled with ``ws_fill``; the tables stand ``table_offset`` int32 into their
    allocations, which go on for ``table_tail`` more int32 of ``tail_fill``.  -> the six outputs, their tails checked."""
    from ds2hip import lib
    b, t, a = probs.shape
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda() if b else torch.zeros(1, dtype=torch.int32).cuda()
    ints = [torch.full((n + pad,), SENT_I, dtype=torch.int32, device='cuda') for n in (b * t, b * t, b, b)]
    flts = [torch.full((b + pad,), float('nan'), dtype=torch.float32, device='cuda') for _ in range(2)]
    ws_bytes = lib.query('ds2_ctc_beam_ws_bytes', b, t, w)
    ws = torch.full((ws_bytes + 16,), ws_fill, dtype=torch.uint8, device='cuda')
    n_states = len(final) if n_states is None else n_states
    tabs = []
    for x in (np.asarray(trans, np.int32).reshape(-1), np.asarray(final, np.int32)):
        buf = np.full(table_offset + len(x) + table_tail, tail_fill, np.int32)
        buf[table_offset:table_offset + len(x)] = x
        tabs.append(torch.from_numpy(buf).cuda())
    lm_args, keep = _lm_args(lm, p.device, alpha, beta, space_id)
    lib.call('ds2_ctc_beam_search_bias', p if p.numel() else torch.zeros(1, device='cuda'), s, b, t, a, 0, w, 0, *lm_args,
             tabs[0].data_ptr() + 4 * table_offset, tabs[1].data_ptr() + 4 * table_offset, n_states, float(weight), ws,
             ws_bytes, ints[0], ints[1], ints[2], flts[0], flts[1], ints[3])
    torch.cuda.synchronize()
    labels, offsets, lens, bias = [x.cpu().numpy() for x in ints]
    score, ctc = [x.cpu().numpy() for x in flts]
    assert all((x[n:] == SENT_I).all() for x, n in ((labels, b * t), (offsets, b * t), (lens, b), (bias, b))), 'written past'
    assert np.isnan(score[b:]).all() and np.isnan(ctc[b:]).all(), 'written past (B,)'
    return labels[:b * t].reshape(b, t), offsets[:b * t].reshape(b, t), lens[:b], score[:b], ctc[:b], bias[:b]


@pytest.mark.parametrize('unit', [None, 'word'])
def test_a_row_does_not_depend_on_its_company(lms, unit):
    lm = lms[(unit, 0)] if unit else None
    kw = dict(lm=lm, alpha=0.6, beta=0.9, space_id=1)
    rng = np.random.default_rng(5)
    sizes = [40, 1, 0, 48, 23, 48, 9]
    texts = ['THE CAT SEES', 'A', '', 'ABC THE CATS BIRD', 'DOGS RUN', 'A BIRD SEES THE CAT', 'CAT']
    probs = np.full((len(sizes), 48, 29), np.nan, np.float32)                # NaN past sizes[b]: never read
    for b, n in enumerate(sizes):
        probs[b, :n] = _spell(rng, texts[b], 48, 29, noise=1.2)[:n]
    phrases = [[LABELS.index(c) for c in p] for p in SPELLED_PHRASES]
    trans, final = _graph(phrases, 29)
    batch = _abi_call(probs, sizes, 16, trans, final, 1.25, **kw)
    assert batch[2][2] == 0 and batch[4][2] == 0.0 and batch[5][2] == 0 and batch[5].any()     # sizes[2] = 0: nothing said
    assert unit or batch[3][2] == 0.0                                        # (with an LM the empty labelling pays for </s>)
    # another workspace content and tables that stand elsewhere in memory: the same bits
    moved = _abi_call(probs, sizes, 16, trans, final, 1.25, ws_fill=255, table_offset=13, table_tail=5, tail_fill=-1, **kw)
    for x, y in zip(batch, moved):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for b, n in enumerate(sizes):                                        # alone, with T cut to its own length
        alone = _abi_call(probs[b:b + 1, :n], [n], 16, trans, final, 1.25, ws_fill=170, **kw)
        m = alone[2][0]
        assert m == batch[2][b] and alone[5][0] == batch[5][b]
        assert np.array_equal(alone[0][0, :m], batch[0][b, :m]) and np.array_equal(alone[1][0, :m], batch[1][b, :m])
        for k in (3, 4):
            assert alone[k][0].view(np.uint32) == batch[k][b].view(np.uint32)
    _compare(batch, _reference(np.nan_to_num(probs, nan=0.0), sizes, 16, trans, final, 1.25, **kw))
    none = _abi_call(probs[:0], [], 16, trans, final, 1.25, **kw)            # B = 0: nothing is written
    assert all(x.size == 0 for x in none)


# ------------------------------------------------------------------------------------- 6. next states outside the table
def test_a_next_state_outside_the_table_is_the_root():
    a, w = 5, 16
    rng = np.random.default_rng(77)
    probs = _softmax(rng.standard_normal((3, 30, a)) * 2.0)
    sizes = [30, 22, 30]
    phrases = [[1, 2], [2, 3, 1], [4]]
    trans, final = _graph(phrases, a)
    n = len(final)
    bad = trans.copy()
    leaves = (bad & 0xFFFF) == 0                          # every return to the root: to a node past the table instead
    where = np.argwhere(leaves & (np.arange(a)[None, :] != 0))
    assert len(where) >= 6
    for k, (s_, c) in enumerate(where):
        bad[s_, c] = (int(bad[s_, c]) & ~0xFFFF) | (n + (k * 9973) % (65536 - n))
    assert ((bad & 0xFFFF) >= n).sum() == len(where) and int((bad & 0xFFFF).max()) > 30000
    clean = bias_ref.sanitised(bad, n)
    assert np.array_equal(clean, trans)
    refs = _reference(probs, sizes, w, clean, final, 0.75)
    # the allocation goes on past the table with entries that would earn a label each: an unguarded walk reads them
    tail = 65536 * a
    out = _abi_call(probs, sizes, w, bad, final, 0.75, table_tail=tail, tail_fill=(1 << 16) | 1)
    _compare(out, refs)
    good = _abi_call(probs, sizes, w, trans, final, 0.75)
    for x, y in zip(out, good):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert any(r[4] > 0 for r in refs) and math.isfinite(refs[0][2])
