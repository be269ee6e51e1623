"""tests/conf_ref.py, the float64 statement of ds2_ctc_unit_posterior, held against brute force, against torch's CTC loss and
against its own exact variant; the header and the binding table; ``codes.metrics.word_matches``.  No GPU."""
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import conf_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dyadic(rng, n, a):
    """(n, a) probabilities from {1/2, 1/4, 0}"""
    return rng.choice([0.5, 0.25, 0.0], size=(n, a), p=[0.5, 0.3, 0.2]).astype(np.float32)


def test_reference_equals_enumeration_of_every_alignment():
    rng = np.random.RandomState(0)
    units = [u for ln in (1, 2, 3) for u in itertools.product((1, 2), repeat=ln)]      # A = 3, blank 0; repeats included
    seen_zero = seen_pos = 0
    for n in range(1, 7):
        span = _dyadic(rng, n, 3)
        for unit in units:
            want = cr.brute_force(span, unit, 0)
            assert cr.forward(span, unit, 0, exact=True) == want, (n, unit)
            got = cr.forward(span, unit, 0)
            if want == 0:
                seen_zero += 1
                assert got == -math.inf
            else:
                seen_pos += 1
                assert got == math.log(float(want)), (n, unit)                         # dyadic inputs: every step is exact
    assert seen_zero and seen_pos
    assert cr.forward(_dyadic(rng, 2, 3) + 0.25, (1, 1), 0) == -math.inf               # LL on two frames needs a blank between


def test_reference_equals_torch_ctc_loss_in_double():
    rng = np.random.RandomState(1)
    for n, unit, a in ((1, (3,), 5), (7, (1, 1), 3), (12, (2, 3, 3, 1), 5), (40, (4, 2, 4, 4, 1, 3), 6), (300, (1, 2, 2), 4)):
        p = rng.rand(n, a).astype(np.float32) ** 3 + np.float32(1e-3)
        p /= p.sum(1, keepdims=True)
        logp = torch.log(torch.from_numpy(p).double())[:, None, :]
        loss = torch.nn.functional.ctc_loss(logp, torch.tensor([unit]), torch.tensor([n]), torch.tensor([len(unit)]),
                                            blank=0, reduction='sum')
        got = cr.forward(p, unit, 0)
        assert abs(math.exp(got) - math.exp(-float(loss))) <= 1e-12, (n, unit)
        assert abs(got + float(loss)) <= 1e-12 * max(1.0, abs(got)) * n, (n, unit)


def test_rescaling_keeps_a_long_span_finite_and_nan_counts_as_zero():
    span = np.full((2000, 2), 0.5, np.float32)
    got = cr.forward(span, (1,), 0)
    # alignments of 2000 frames that read as one label: a run of i >= 1 label frames anywhere = 2000 * 2001 / 2
    assert math.isfinite(got) and abs(got - (math.log(2000 * 2001 / 2) - 2000 * math.log(2.0))) <= 1e-9
    span = np.array([[0.5, 0.5, np.nan], [np.nan, 0.25, -1.0], [0.5, 0.0, 0.5]], np.float32)
    clean = np.nan_to_num(span, nan=0.0).clip(min=0.0)
    for unit in ((1,), (1, 2), (2,)):
        assert cr.forward(span, unit, 0) == cr.forward(clean, unit, 0)


def test_exact_variant_equals_float64_on_powers_of_two():
    rng = np.random.RandomState(2)
    for n, unit in ((5, (1, 2)), (26, (1, 1, 2, 3)), (20, (3,)), (9, (2, 2, 2, 2))):
        span = _dyadic(rng, n, 4)
        p = cr.forward(span, unit, 0, exact=True)
        assert isinstance(p, Fraction) and Fraction(float(p)) == p
        got = cr.forward(span, unit, 0)
        assert got == (math.log(float(p)) if p else -math.inf)


def test_unit_finding_equals_group_words():
    from codes.align import group_words
    alphabet = '_ abc'                       # blank 0, space 1
    for text in ('ab c', ' ab  c ', '  ', '', 'a', ' a', 'a ', 'abc  ab   c', ' ' * 3 + 'b'):
        labels = [alphabet.index(c) for c in text]
        units = cr.find_units(labels, 1)
        words = group_words([(c, i, i) for i, c in enumerate(text)])
        assert [(''.join(alphabet[c] for c in labels[i:i + n]), i, i + n - 1) for i, n in units] == words, text
        assert cr.find_units(labels, -1) == [(i, 1) for i in range(len(text))]


def test_every_invalid_row_rule():
    probs = np.full((2, 10, 4), 0.25, np.float32)
    sizes = [10, 6]
    good = dict(labels=[1, 2, 3, 1], offsets=[0, 2, 3, 5], length=4, stride=4, utt=1)

    def valid(**kw):
        a = dict(good, **kw)
        return cr.row_valid(a['labels'], a['offsets'], a['length'], a['stride'], a['utt'], 2, sizes, 10, 4, 0)

    assert valid() and valid(length=0) and valid(utt=0, offsets=[0, 2, 3, 9])
    assert not valid(length=-1) and not valid(length=5)
    assert not valid(utt=-1) and not valid(utt=2)
    assert not valid(labels=[1, 4, 3, 1]) and not valid(labels=[1, -1, 3, 1]) and not valid(labels=[1, 0, 3, 1])
    assert not valid(offsets=[0, 2, 2, 5]) and not valid(offsets=[0, 3, 2, 5]) and not valid(offsets=[-1, 2, 3, 5])
    assert not valid(offsets=[0, 2, 3, 6])                                       # sizes[1] = 6
    assert not valid(utt=0, offsets=[0, 2, 3, 10])                               # T = 10
    assert valid(labels=[1, 2, 9, 9], offsets=[0, 2, 0, 0], length=2)            # nothing past lens counts
    out = cr.unit_posterior(probs, sizes, [[1, 2, 3, 1], [1, 2, 3, 1]], [[0, 2, 3, 5], [0, 2, 3, 6]], [4, 4], [1, 1], 3)
    assert out[3].tolist() == [2, -1] and (out[0][1] == -1).all() and np.isnan(out[2][1]).all()


def test_header_declares_both_symbols_as_the_binding_table_has_them():
    from ds2hip import lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ds2hip.h')).read(), flags=re.S)
    for name in ('ds2_ctc_unit_posterior_ws_bytes', 'ds2_ctc_unit_posterior'):
        m = re.search(r'\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, text)
        assert m, name
        assert len(m.group(1).split(',')) == len(lib.SIGNATURES[name][1]), name
    assert int(re.search(r'#define\s+DS2_UNIT_MAX_LABELS\s+(\d+)', text).group(1)) == lib.UNIT_MAX_LABELS == cr.MAX_LABELS
    assert lib.UNIT_MAX_LABELS == lib.KWS_MAX_LEN


def test_unit_confidence_refuses_words_without_a_space():
    from codes.confidence import UnitConfidence
    with pytest.raises(ValueError, match="unit='word' needs a space"):
        UnitConfidence(list('_abc'))
    assert UnitConfidence(list('_abc'), unit='char').space_id == -1
    assert UnitConfidence(list('_ abc')).space_id == 1


def test_word_matches_hand_cases():
    from codes.metrics import word_matches
    w = str.split
    assert word_matches(w('a b c'), w('a b c')) == [True, True, True]
    assert word_matches(w('a x c'), w('a b c')) == [True, False, True]            # substitution
    assert word_matches(w('a b x c'), w('a b c')) == [True, True, False, True]    # insertion (a hypothesis word dropped)
    assert word_matches(w('a c'), w('a b c')) == [True, True]                      # deletion (a reference word dropped)
    assert word_matches([], w('a b')) == [] and word_matches(w('a b'), []) == [False, False]
    assert word_matches([], []) == []
    assert word_matches(w('b a'), w('a b')) == [False, False]                      # two substitutions: the diagonal keeps 2
    assert word_matches(w('a a'), w('a')) == [False, True]                         # the back-trace takes the diagonal first


def test_word_matches_against_the_word_distance():
    from codes.decoder import _levenshtein
    from codes.metrics import word_matches
    rng = np.random.RandomState(3)
    for _ in range(200):
        hyp = [str(x) for x in rng.randint(0, 4, rng.randint(0, 8))]
        ref = [str(x) for x in rng.randint(0, 4, rng.randint(0, 8))]
        ok = word_matches(hyp, ref)
        assert len(ok) == len(hyp)
        dist = _levenshtein(hyp, ref)
        assert len(hyp) - sum(ok) <= dist                       # every wrong hypothesis word is a substitution or an insertion
        if dist == len(hyp) - len(ref):                         # the reference is a subsequence: insertions only
            assert len(hyp) - sum(ok) == dist
    # a reference of distinct words, some replaced by and some joined by words it does not have: no optimal alignment
    # drops a reference word (dropping one cannot bring two equal words together), so wrong words = distance
    for _ in range(100):
        ref = ['r%d' % i for i in range(rng.randint(0, 7))]
        hyp, edits = [], 0
        for word in ref:
            while rng.rand() < 0.3:
                hyp.append('new%d' % len(hyp))
                edits += 1
            if rng.rand() < 0.3:
                hyp.append('new%d' % len(hyp))
                edits += 1
            else:
                hyp.append(word)
        ok = word_matches(hyp, ref)
        assert _levenshtein(hyp, ref) == edits == len(hyp) - sum(ok)
        assert [h for h, c in zip(hyp, ok) if c] == [h for h in hyp if h.startswith('r')]
