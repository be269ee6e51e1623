"""Device CTC beam search (ds2_ctc_beam_search_batch, csrc/ctc_beam.hip) where it is hardest to get right: exact ties at
the W-th key and at the final pick, a blank other than 0, the beam-width / alphabet limits (dynamic LDS above 64 KB),
LM orders 5-8, long utterances, and inputs at the edges (-inf log-probs, all-zero frames, out-of-range sizes, padding).
Every case is compared with the fp64 Python contract tests/beam_ref.py; cases without an LM and without ties also with
the host search ds2_ctc_beam_search."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_ref
from tests.test_beam_ref_cpu import HAND_TIES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]
WORDS = ['CAT', 'DOG', 'A', 'THE', 'BIRD', 'SEES', 'RUNS']
TIE_GAP = 1e-9        # a non-tied score this close (relative) to the cut could be ordered differently by two libms


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _device(probs, sizes, w, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    from ds2hip import ops
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    out = ops.ctc_beam_search(p, s, w, blank, log_input, lm, alpha, beta, space_id)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _host(probs, n, w, blank=0, log_input=False):
    from ds2hip import lib
    a = probs.shape[-1]
    ids, offs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    length, lp = ctypes.c_int(0), ctypes.c_float(0)
    lib.host_call('ds2_ctc_beam_search', np.ascontiguousarray(probs[:n]), n, a, blank, w, int(log_input), ids, offs,
                  len(ids), length, lp)
    return ids[:length.value].tolist(), lp.value


def _close(x, y):
    if not np.isfinite(y):
        return x == y
    return abs(float(x) - y) <= 1e-6 * max(1.0, abs(y))


def _check(out, probs, sizes, w, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1, host=None,
           ties=None):
    """Compare every utterance of a device result with beam_ref (and with the host search if ``host``).  ``ties``:
    None = the inputs must have no exact tie at a cut or pick; a list = collects the number of tied cuts/picks per
    utterance.  Either way every non-tied score stays TIE_GAP away from the cut."""
    labels, offsets, lens, score, ctc = out
    t = probs.shape[1]
    for b, size in enumerate(sizes):
        n = min(max(size, 0), t)
        stats = {}
        ref = beam_ref.beam_search(beam_ref.frame_log_probs(probs[b, :n], log_input), blank, w, lm, alpha, beta,
                                   space_id, stats=stats)
        marks = stats['cut'] + [stats['pick']]
        assert min(gap for _, gap in marks) > TIE_GAP, (b, 'a near-tie: the case does not decide the rule')
        n_ties = sum(tie for tie, _ in marks)
        if ties is None:
            assert n_ties == 0, b
        else:
            ties.append(n_ties)
        got = labels[b, :lens[b]].tolist()
        assert got == ref[0], (b, n, w)
        assert offsets[b, :lens[b]].tolist() == ref[1], (b, n, w)
        assert _close(score[b], ref[2]) and _close(ctc[b], ref[3]), (b, float(score[b]), ref[2], float(ctc[b]), ref[3])
        assert not labels[b, lens[b]:].any() and not offsets[b, lens[b]:].any()
        if host:
            want, want_lp = _host(probs[b], n, w, blank, log_input)
            assert got == want, (b, n, w)
            assert abs(float(ctc[b]) - want_lp) <= 1e-6 * max(1.0, abs(want_lp))


def _make_lm(tmp_path, order, unit, labels=LABELS, sents=None, blank=0):
    from codes.lm import NGramLM
    if sents is None:
        rng = np.random.default_rng(order)
        sents = [' '.join(rng.choice(WORDS, size=rng.integers(2, 7))) for _ in range(80)]
    txt = tmp_path / ('c_%s%d.txt' % (unit, order))
    txt.write_text('\n'.join(sents) + '\n')
    out = str(tmp_path / ('lm_%s%d.arpa' % (unit, order)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_lm.py'), '--order', str(order), '--unit', unit,
                        '--text', str(txt), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return NGramLM.from_arpa(out, labels, unit=unit, blank_index=blank), sents, out


def _spell(rng, text, t, a, noise=1.5, labels=LABELS, blank=0):
    """(t, a) probabilities spelling ``text`` (one frame per character, then a blank-leaning frame), noise after."""
    x = rng.standard_normal((t, a)) * noise
    fr = 0
    for ch in text:
        if fr + 1 >= t:
            break
        x[fr, labels.index(ch)] += 3.0
        x[fr + 1, blank] += 2.0
        fr += 2
    return _softmax(x)


def lookup_orders(lm, labels, space_id):
    """The order of the n-gram each LM lookup along ``labels`` finds (0 = out of vocabulary), end of utterance included:
    what the device's backoff walk must reach."""
    def hit(hist, w):
        if w is None or (w,) not in lm.ngrams:
            return 0
        hist = tuple(hist)[max(0, len(hist) - (lm.order - 1)):] if lm.order > 1 else ()
        for k in range(len(hist), 0, -1):
            if hist[len(hist) - k:] + (w,) in lm.ngrams:
                return k + 1
        return 1

    ctx, word, orders = (lm.bos_id,) if lm.order > 1 else (), [], []

    def score(w):
        nonlocal ctx
        orders.append(hit(ctx, w))
        _, tok = lm.log_prob_ids(ctx, w)
        ctx = (ctx + (tok,))[-(lm.order - 1):] if lm.order > 1 else ()

    for c in list(labels) + ([space_id] if lm.unit == 'word' else []):
        if lm.unit == 'char':
            score(c)
        elif c == space_id:
            if word:
                score(lm.word_id(word))
            word = []
        else:
            word.append(c)
    orders.append(hit(ctx, lm.eos_id))
    return orders


# ----------------------------------------------------------------------------------------------------------- 1. ties
def _tie_probs(rng, b, t, a, dup_cols, uniform_rows, boost=0.0):
    """Structural ties: the columns in each group of ``dup_cols`` carry identical values (raised by ``boost`` logits),
    and a fraction ``uniform_rows`` of the frames is exactly uniform.  Symmetric prefixes are then scored by the same operations on the
    same values, in beam_ref and on the device alike."""
    x = rng.standard_normal((b, t, a)) * 2.0
    for group in dup_cols:
        x[..., group] = x[..., group[:1]] + boost
    p = _softmax(x)
    p[rng.random((b, t)) < uniform_rows] = np.float32(1.0 / a)
    return p


@pytest.mark.parametrize('kind', ['dup', 'dup_uniform'])
@pytest.mark.parametrize('w', [4, 16, 64, 128])
def test_exact_ties_no_lm(kind, w):
    rng = np.random.default_rng(w + len(kind))
    probs = _tie_probs(rng, 3, 30, 29, [[4, 5], [8, 9, 10]], 0.0 if kind == 'dup' else 0.3)
    sizes = [30, 30, 17]
    ties = []
    _check(_device(probs, sizes, w), probs, sizes, w, ties=ties)
    assert sum(ties) >= 3, ties


@pytest.fixture(scope='module')
def corpus_lms(tmp_path_factory):
    d = tmp_path_factory.mktemp('lm')
    return {unit: _make_lm(d, 3, unit)[0] for unit in ('char', 'word')}


@pytest.mark.parametrize('unit', ['char', 'word'])
@pytest.mark.parametrize('w', [4, 16, 64, 128])
def test_exact_ties_with_lm(corpus_lms, unit, w):
    # J K and Q X Z spell no corpus word: in either unit the LM scores them alike (out of vocabulary)
    lm = corpus_lms[unit]
    cols = [[LABELS.index(c) for c in 'JK'], [LABELS.index(c) for c in 'QXZ']]
    rng = np.random.default_rng(w * 3 + len(unit))
    probs = _tie_probs(rng, 3, 30, 29, cols, 0.3, boost=2.5)
    sizes = [30, 24, 30]
    ties = []
    _check(_device(probs, sizes, w, lm=lm, alpha=0.5, beta=1.0, space_id=1), probs, sizes, w, lm=lm, alpha=0.5,
           beta=1.0, space_id=1, ties=ties)
    assert sum(ties) >= 1, ties


@pytest.mark.parametrize('case', HAND_TIES, ids=[c[0] for c in HAND_TIES])
def test_hand_derived_ties(case):
    _, probs, blank, w, labels, offsets = case
    out = _device(np.float32([probs]), [len(probs)], w, blank)
    assert out[0][0, :out[2][0]].tolist() == labels and out[1][0, :out[2][0]].tolist() == offsets


def test_tie_inputs_repeat_bit_identically(corpus_lms):
    rng = np.random.default_rng(99)
    cols = [[LABELS.index(c) for c in 'JK'], [LABELS.index(c) for c in 'QXZ'], [4, 5]]
    probs = _tie_probs(rng, 8, 40, 29, cols, 0.4)
    sizes = [40, 39, 1, 0, 25, 40, 33, 12]
    for lm in (None, corpus_lms['char']):
        first = _device(probs, sizes, 64, lm=lm, alpha=0.5, beta=1.0, space_id=1)
        for _ in range(2):
            again = _device(probs, sizes, 64, lm=lm, alpha=0.5, beta=1.0, space_id=1)
            for x, y in zip(first, again):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------------------------------------------- 2. blank != 0
@pytest.mark.parametrize('a', [29, 43])
@pytest.mark.parametrize('where', ['last', 'middle'])
@pytest.mark.parametrize('w', [1, 16, 128])
def test_nonzero_blank_no_lm(a, where, w):
    blank = a - 1 if where == 'last' else a // 2
    rng = np.random.default_rng(a * w + blank)
    t = 30 if w < 128 else 16
    x = rng.standard_normal((4, t, a)) * 2.5
    x[..., blank] += 1.0
    probs = _softmax(x)
    sizes = [t, t - 5, 1, t]
    _check(_device(probs, sizes, w, blank), probs, sizes, w, blank, host=True)


def _moved_blank(blank):
    """LABELS with the blank moved to index ``blank`` (the other labels keep their order)."""
    rest = LABELS[1:]
    return rest[:blank] + ['_'] + rest[blank:]


@pytest.mark.parametrize('unit', ['char', 'word'])
@pytest.mark.parametrize('where', ['last', 'middle'])
@pytest.mark.parametrize('w', [1, 16, 128])
def test_nonzero_blank_with_lm(tmp_path, unit, where, w):
    blank = 28 if where == 'last' else 14
    labels = _moved_blank(blank)
    lm, sents, _ = _make_lm(tmp_path, 3, unit, labels, blank=blank)
    space = labels.index(' ')
    rng = np.random.default_rng(w + blank + len(unit))
    t = 40 if w < 128 else 24
    probs = np.stack([_spell(rng, ' '.join(sents[i:i + 3]), t, 29, labels=labels, blank=blank) for i in range(3)])
    sizes = [t, t - 7, 2]
    _check(_device(probs, sizes, w, blank, lm=lm, alpha=0.7, beta=1.2, space_id=space), probs, sizes, w, blank,
           lm=lm, alpha=0.7, beta=1.2, space_id=space)


@pytest.mark.parametrize('unit', [None, 'char', 'word'])
def test_alphabet_permutation(tmp_path, unit):
    from codes.lm import NGramLM
    rng = np.random.default_rng(17)
    perm = rng.permutation(29)                      # new column j holds old column perm[j]
    inv = np.argsort(perm)
    plabels = [LABELS[k] for k in perm]
    blank, space = int(inv[0]), int(inv[1])
    lm = plm = None
    if unit:
        lm, sents, path = _make_lm(tmp_path, 4, unit)
        plm = NGramLM.from_arpa(path, plabels, unit=unit, blank_index=blank)
        probs = np.stack([_spell(rng, ' '.join(sents[i:i + 3]), 40, 29) for i in range(3)])
    else:
        probs = _softmax(rng.standard_normal((3, 40, 29)) * 2.5)
    sizes = [40, 31, 40]
    w = 16
    base = _device(probs, sizes, w, 0, lm=lm, alpha=0.6, beta=0.9, space_id=1)
    _check(base, probs, sizes, w, 0, lm=lm, alpha=0.6, beta=0.9, space_id=1, host=unit is None)
    moved = _device(probs[..., perm], sizes, w, blank, lm=plm, alpha=0.6, beta=0.9, space_id=space)
    for b in range(3):
        n = base[2][b]
        assert moved[2][b] == n
        assert moved[0][b, :n].tolist() == inv[base[0][b, :n]].tolist()
        assert np.array_equal(moved[1][b], base[1][b])
    for k in (3, 4):
        assert np.array_equal(moved[k].view(np.uint32), base[k].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------- 3. limits
@pytest.mark.parametrize('w, a', [(128, 48), (128, 64), (100, 128), (128, 128)])
def test_beam_and_alphabet_limits(w, a):
    # 8*W*A bytes of candidate keys: 48 KB .. 128 KB of dynamic LDS, on top of the static beam state
    rng = np.random.default_rng(w + a)
    probs = _softmax(rng.standard_normal((3, 10, a)) * 3.0)
    sizes = [10, 7, 10]
    _check(_device(probs, sizes, w), probs, sizes, w, host=True)
    blank = a - 1
    _check(_device(probs, sizes, w, blank), probs, sizes, w, blank, host=True)


@pytest.mark.parametrize('a', [1, 2])
@pytest.mark.parametrize('w', [5, 37, 127])
def test_tiny_alphabets_and_odd_widths(a, w):
    rng = np.random.default_rng(a * 1000 + w)
    probs = _softmax(rng.standard_normal((3, 25, a)) * 2.0)
    sizes = [25, 12, 1]
    for blank in range(a):
        _check(_device(probs, sizes, w, blank), probs, sizes, w, blank, host=True)


@pytest.mark.parametrize('w', [5, 37, 127])
def test_odd_widths(w):
    rng = np.random.default_rng(w)
    probs = _softmax(rng.standard_normal((2, 20, 29)) * 2.5)
    _check(_device(probs, [20, 15], w), probs, [20, 15], w, host=True)


def test_grid_larger_than_the_device():
    rng = np.random.default_rng(300)
    b, t = 300, 6
    probs = _softmax(rng.standard_normal((b, t, 29)) * 2.5)
    sizes = [int(x) for x in rng.integers(0, t + 1, size=b)]
    labels, _, lens, _, ctc = _device(probs, sizes, 16)
    for i in range(b):
        want, want_lp = _host(probs[i], sizes[i], 16)
        assert labels[i, :lens[i]].tolist() == want, i
        assert abs(float(ctc[i]) - want_lp) <= 1e-6 * max(1.0, abs(want_lp))


# --------------------------------------------------------------------------------------------------- 4. LM orders 5-8
@pytest.mark.parametrize('unit, order', [('char', 5), ('char', 6), ('char', 8), ('word', 5)])
def test_high_order_lm(tmp_path, unit, order):
    lm, sents, _ = _make_lm(tmp_path, order, unit)
    assert lm.order == order
    rng = np.random.default_rng(order)
    t = 120
    probs = np.stack([_spell(rng, ' '.join(sents[3 * i:3 * i + 8]), t, 29, noise=0.7) for i in range(2)])
    sizes = [t, 101]
    out = _device(probs, sizes, 16, lm=lm, alpha=0.4, beta=1.0, space_id=1)
    _check(out, probs, sizes, 16, lm=lm, alpha=0.4, beta=1.0, space_id=1)
    orders = [lookup_orders(lm, out[0][b, :out[2][b]].tolist(), 1) for b in range(2)]
    assert sum(o.count(order) for o in orders) >= 3, orders     # full-length histories decided some of the scores


def _write_arpa(path, grams):
    """grams: {n: [(log10 p, tokens str, log10 backoff or None)]}"""
    lines = ['\\data\\'] + ['ngram %d=%d' % (n, len(grams[n])) for n in sorted(grams)]
    for n in sorted(grams):
        lines += ['', '\\%d-grams:' % n]
        lines += ['%g\t%s' % (p, toks) + ('' if bo is None else '\t%g' % bo) for p, toks, bo in grams[n]]
    path.write_text('\n'.join(lines + ['', '\\end\\', '']))
    return str(path)


def test_hand_written_8gram(tmp_path):
    """After B C D E F G H the frames cannot tell J from K (identical columns).  P(J | BCDEFGH) is only reachable by
    backing off through all seven contexts (-0.2 + 6 * -0.15 = -1.1), P(K | BCDEFGH) is a present 8-gram (-1.0): with
    the whole 7-token history K wins; a history cut short, or a backoff weight dropped, makes J win."""
    from codes.lm import NGramLM
    seq = 'BCDEFGH'
    grams = {1: [(-99, '<s>', -0.5), (-1.0, '</s>', None)] + [(-1.5, c, -0.1) for c in seq] + [(-1.2, 'J', None),
                                                                                               (-2.0, 'K', None)],
             2: [(-0.2, 'H J', None), (-0.3, '<s> B', None), (-0.5, 'G H', -0.15)]}
    for n in range(3, 8):
        grams[n] = [(-0.5, ' '.join(seq[7 - n:]), -0.15)]
    grams[8] = [(-1.0, ' '.join(seq + 'K'), None)]
    lm = NGramLM.from_arpa(_write_arpa(tmp_path / 'hand8.arpa', grams), LABELS, unit='char')
    assert lm.order == 8
    j, k = LABELS.index('J'), LABELS.index('K')
    hist = [lm.bos_id] + [LABELS.index(c) for c in seq]
    assert abs(lm.log_prob_ids(hist, k)[0] - (-1.0 * beam_ref.math.log(10))) < 1e-6
    assert abs(lm.log_prob_ids(hist, j)[0] - (-1.1 * beam_ref.math.log(10))) < 1e-5
    x = np.full((2, 40, 29), -3.0)
    for i, c in enumerate(seq + 'J'):
        x[:, 2 * i, LABELS.index(c)] = 3.0
        x[:, 2 * i + 1, 0] = 3.0
    x[:, 14, k] = x[:, 14, j]                       # frame 14: J and K tie acoustically
    x[:, 16:, 0] = 3.0
    probs = _softmax(x)
    sizes = [40, 17]
    out = _device(probs, sizes, 8, lm=lm, alpha=1.0, beta=0.5, space_id=1)
    _check(out, probs, sizes, 8, lm=lm, alpha=1.0, beta=0.5, space_id=1, ties=[])
    for b in range(2):
        got = out[0][b, :out[2][b]].tolist()
        assert got == [LABELS.index(c) for c in seq + 'K'], (b, got)
        assert lookup_orders(lm, got, 1)[7] == 8


@pytest.mark.parametrize('with_unk', [False, True])
def test_out_of_vocabulary_words(tmp_path, with_unk):
    from codes.lm import NGramLM
    words = ['CAT', 'DOG', 'THE']
    grams = {1: [(-99, '<s>', -0.3), (-0.8, '</s>', None)] + [(-0.9, w, -0.2) for w in words],
             2: [(-0.2, '<s> THE', -0.1), (-0.3, 'THE CAT', -0.1), (-0.4, 'CAT </s>', None), (-0.5, 'THE DOG', None)],
             3: [(-0.1, '<s> THE CAT', None)]}
    if with_unk:
        grams[1].append((-2.5, '<unk>', None))
    lm = NGramLM.from_arpa(_write_arpa(tmp_path / 'w.arpa', grams), LABELS, unit='word')
    assert (lm.unk_id >= 0) == with_unk
    rng = np.random.default_rng(5)
    texts = ['THE CAT', 'THE BAT SAW DOG', 'ZZ CAT THE', 'DOGS']
    probs = np.stack([_spell(rng, s, 50, 29, noise=1.0) for s in texts])
    sizes = [50, 50, 44, 50]
    out = _device(probs, sizes, 16, lm=lm, alpha=0.6, beta=0.8, space_id=1)
    _check(out, probs, sizes, 16, lm=lm, alpha=0.6, beta=0.8, space_id=1)
    assert any(0 in lookup_orders(lm, out[0][b, :out[2][b]].tolist(), 1) for b in range(4))


# ----------------------------------------------------------------------------------------------------------- 5. long T
def test_long_utterances_no_lm():
    rng = np.random.default_rng(746)
    t = 746
    probs = _softmax(rng.standard_normal((4, t, 29)) * 2.5)
    sizes = [746, 745, 400, 1]
    out = _device(probs, sizes, 128)
    labels, offsets, lens, score, ctc = out
    for b, n in enumerate(sizes):
        want, want_lp = _host(probs[b], n, 128)
        assert labels[b, :lens[b]].tolist() == want, b
        assert abs(float(ctc[b]) - want_lp) <= 1e-6 * max(1.0, abs(want_lp)) and score[b] == ctc[b]
        assert not labels[b, lens[b]:].any()
    _check([x[2:3] for x in out], probs[2:3], sizes[2:3], 128)


def test_long_utterance_char_lm(tmp_path):
    lm, sents, _ = _make_lm(tmp_path, 6, 'char')
    rng = np.random.default_rng(300)
    t = 300
    probs = _spell(rng, ' '.join(sents[:30]), t, 29)[None]
    out = _device(probs, [t], 16, lm=lm, alpha=0.8, beta=1.0, space_id=1)
    _check(out, probs, [t], 16, lm=lm, alpha=0.8, beta=1.0, space_id=1)
    assert out[2][0] > 60


# --------------------------------------------------------------------------------------------- 6. edges, invariance
def test_minus_infinity_log_input():
    rng = np.random.default_rng(8)
    lp = np.log(_softmax(rng.standard_normal((3, 30, 29)) * 2.0))
    lp[rng.random(lp.shape) < 0.4] = -np.inf
    lp[..., 0] = np.maximum(lp[..., 0], np.log(0.05))
    lp[1, 5, :] = -np.inf                         # no label at all is possible in frame 5
    sizes = [30, 30, 20]
    _check(_device(lp, sizes, 16, log_input=True), lp, sizes, 16, log_input=True, ties=[])
    assert np.isneginf(_device(lp, sizes, 16, log_input=True)[4][1])


@pytest.mark.parametrize('frame', [0, 11])
def test_all_zero_frame(corpus_lms, frame):
    rng = np.random.default_rng(frame)
    probs = _softmax(rng.standard_normal((2, 25, 29)) * 2.0)
    probs[:, frame] = 0.0
    sizes = [25, frame + 1]
    _check(_device(probs, sizes, 16), probs, sizes, 16, ties=[])
    lm = corpus_lms['char']
    _check(_device(probs, sizes, 16, lm=lm, alpha=0.5, beta=1.0, space_id=1), probs, sizes, 16, lm=lm, alpha=0.5,
           beta=1.0, space_id=1, ties=[])


def test_sizes_are_clamped():
    rng = np.random.default_rng(4)
    probs = _softmax(rng.standard_normal((4, 20, 29)) * 2.0)
    out = _device(probs, [25, -3, 20, 1 << 30], 16)
    want = _device(probs, [20, 0, 20, 20], 16)
    for x, y in zip(out, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    _check(want, probs, [20, 0, 20, 20], 16, host=True)
    assert out[2][1] == 0 and out[3][1] == 0.0


def _abi_call(probs, sizes, w, lm=None, alpha=0.0, beta=0.0, space_id=-1, pad=64):
    """ds2_ctc_beam_search_batch called directly, every output buffer ``pad`` elements longer than (B, T) / (B,) and
    pre-filled with a sentinel -> (labels, offsets, lens, score, ctc) of shape (B, T) / (B,), and the untouched tails."""
    from ds2hip import lib
    b, t, a = probs.shape
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    sent_i, sent_f = -12345, float('nan')
    labels = torch.full((b * t + pad,), sent_i, dtype=torch.int32, device='cuda')
    offsets = torch.full((b * t + pad,), sent_i, dtype=torch.int32, device='cuda')
    lens = torch.full((b + pad,), sent_i, dtype=torch.int32, device='cuda')
    score = torch.full((b + pad,), sent_f, dtype=torch.float32, device='cuda')
    ctc = torch.full((b + pad,), sent_f, dtype=torch.float32, device='cuda')
    ws_bytes = lib.query('ds2_ctc_beam_ws_bytes', b, t, w)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device='cuda')
    if lm is None:
        lm_args = (None, 0, None, 0, 1, 0, -1, -1, -1, -1, 0.0, 0.0, 0.0)
    else:
        tabs = lm.to(p.device)
        word = tabs.get('word')
        lm_args = (tabs['ngram'], tabs['ngram'].shape[0], word, 0 if word is None else word.shape[0], lm.order,
                   1 if lm.unit == 'char' else 2, lm.bos_id, lm.eos_id, lm.hist_unk_id, space_id, float(alpha),
                   float(beta), float(lm.oov_logp))
    lib.call('ds2_ctc_beam_search_batch', p, s, b, t, a, 0, w, 0, *lm_args, ws, ws_bytes, labels, offsets, lens, score,
             ctc)
    torch.cuda.synchronize()
    labels, offsets, lens, score, ctc = [x.cpu().numpy() for x in (labels, offsets, lens, score, ctc)]
    tails = [labels[b * t:], offsets[b * t:], lens[b:]]
    assert all((x == sent_i).all() for x in tails), 'written past (B, T)'
    assert np.isnan(score[b:]).all() and np.isnan(ctc[b:]).all(), 'written past (B,)'
    return labels[:b * t].reshape(b, t), offsets[:b * t].reshape(b, t), lens[:b], score[:b], ctc[:b]


@pytest.mark.parametrize('unit', [None, 'word'])
def test_batch_and_padding_invariance(corpus_lms, unit):
    lm = corpus_lms[unit] if unit else None
    kw = dict(lm=lm, alpha=0.7, beta=1.1, space_id=1)
    rng = np.random.default_rng(21)
    sizes = [37, 1, 0, 50, 23]
    t = 64
    probs = np.full((len(sizes), t, 29), np.nan, np.float32)      # NaN past sizes[b]: never read
    for b, n in enumerate(sizes):
        probs[b, :n] = _softmax(rng.standard_normal((n, 29)) * 2.0)
    batch = _abi_call(probs, sizes, 32, **kw)
    for b, n in enumerate(sizes):
        assert not batch[0][b, batch[2][b]:].any() and not batch[1][b, batch[2][b]:].any()
        alone = _abi_call(probs[b:b + 1, :max(n, 1)] if n else np.zeros((1, 0, 29), np.float32), [n], 32, **kw)
        m = alone[2][0]
        assert m == batch[2][b]
        assert np.array_equal(alone[0][0, :m], batch[0][b, :m]) and np.array_equal(alone[1][0, :m], batch[1][b, :m])
        for k in (3, 4):
            assert alone[k][0].view(np.uint32) == batch[k][b].view(np.uint32)
    clean = np.nan_to_num(probs, nan=0.0)
    _check(batch, clean, sizes, 32, **kw)
