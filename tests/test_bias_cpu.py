"""Phrase boosting without a GPU: codes.bias.ContextGraph against the brute-force definition of V and F (tests/bias_ref.py),
the BFS numbering, the NEW / NEW YORK example, the limits and refusals of ContextGraph and PhraseBooster, the reference
search with a root-only graph against beam_ref, and the argument refusals of ds2_ctc_beam_search_bias."""
import ctypes
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import beam_ref, bias_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_sets(n_labels, count, seed):
    """``count`` random phrase sets over the labels 1..n_labels (blank 0): 1..5 phrases of 1..4 labels, no duplicates."""
    rng = np.random.RandomState(seed)
    for _ in range(count):
        want = set()
        for _ in range(rng.randint(1, 6)):
            want.add(tuple(int(c) for c in rng.randint(1, n_labels + 1, size=rng.randint(1, 5))))
        yield sorted(want, key=lambda p: rng.rand())


@pytest.mark.parametrize('n_labels', [2, 3])
def test_tables_reproduce_v_and_f_for_every_string_up_to_length_7(n_labels):
    from codes.bias import ContextGraph
    strings = [y for n in range(8) for y in itertools.product(range(1, n_labels + 1), repeat=n)]
    for case, phrases in enumerate(_random_sets(n_labels, 100, 11 * n_labels)):
        g = ContextGraph(phrases, n_labels + 1, 0)
        paths, nxt, gain, final = bias_ref.tables(phrases, n_labels + 1, 0)
        assert g.paths == paths, (case, phrases)                                   # the BFS numbering is exact
        assert np.array_equal(g.next, nxt) and np.array_equal(g.gain, gain), (case, phrases)
        assert np.array_equal(g.final, final), (case, phrases)
        assert np.array_equal(g.trans, bias_ref.pack(nxt, gain)) and g.trans.dtype == np.int32
        assert g.gain.min() >= -63 and g.gain.max() <= 1 and g.final.max() <= 0
        assert not g.trans[:, 0].any()
        for y in strings[::3] if case % 4 else strings:
            assert g.walk(y) == (bias_ref.V(y, phrases), bias_ref.F(y, phrases)), (case, phrases, y)


def test_bfs_numbering_children_in_ascending_label_order():
    from codes.bias import ContextGraph
    g = ContextGraph([[3, 1], [1, 2, 2], [1, 1], [3], [1, 2, 1]], 4, 0)
    assert g.paths == [(), (1,), (3,), (1, 1), (1, 2), (3, 1), (1, 2, 1), (1, 2, 2)]
    assert g.depth.tolist() == [0, 1, 1, 2, 2, 2, 3, 3] and g.n_states == 8
    assert g.next[0].tolist() == [0, 1, 0, 2] and g.gain[0].tolist() == [0, 1, 0, 1]
    # a blank that is not label 0: its column is the one left empty
    h = ContextGraph([[0, 1]], 3, 2)
    assert h.paths == [(), (0,), (0, 1)] and not h.trans[:, 2].any() and h.next[0, 0] == 1


def test_new_york_example():
    from codes.bias import ContextGraph
    labels = [' '] + sorted(set('NEWYORKL'))
    ids = lambda s: [labels.index(c) + 1 for c in s]                                # noqa: E731
    phrases = [ids('NEW'), ids('NEW YORK')]
    g = ContextGraph(phrases, len(labels) + 1, 0)
    assert g.n_states == 9
    assert g.walk(ids('NEW YO')) == (6, 3)                    # pending credit is revocable: F keeps the complete NEW
    assert g.walk(ids('NEW YOLK')) == (3, 3)                  # keeps 3, not 7
    assert g.walk(ids('NEW YORK')) == (8, 8)
    assert g.walk(ids('NEW YORKNEW')) == (11, 11)
    assert g.walk(ids('NNEW YOLNEW')) == (6, 6)
    yol = g.paths.index(tuple(ids('NEW YO')))
    assert g.gain[yol, ids('L')[0]] == -3 and g.next[yol, ids('L')[0]] == 0 and g.final[yol] == -3
    for y in ('NEW YO', 'NEW YOLK', 'NEW YORK', 'NNEW YOLNEW', 'NENEW', 'YORK NEW Y'):
        assert g.walk(ids(y)) == (bias_ref.V(ids(y), phrases), bias_ref.F(ids(y), phrases)), y
    # overlap: AB and BC on ABC -- the leftmost occurrence wins and BC does not count
    h = ContextGraph([[1, 2], [2, 3]], 4, 0)
    assert h.walk([1, 2, 3]) == (2, 2) and h.walk([2, 3]) == (2, 2) and h.walk([1, 2, 2, 3]) == (4, 4)


def test_limits_of_the_graph():
    from codes.bias import ContextGraph
    from ds2hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    for name, have in (('LEN', lib.BIAS_MAX_LEN), ('PHRASES', lib.BIAS_MAX_PHRASES), ('STATES', lib.BIAS_MAX_STATES)):
        assert int(re.search(r'#define\s+DS2_BIAS_MAX_%s\s+(\d+)' % name, hdr).group(1)) == have
    assert (lib.BIAS_MAX_LEN, lib.BIAS_MAX_PHRASES, lib.BIAS_MAX_STATES) == (64, 1024, 32768)
    g = ContextGraph([[1] * 64], 3, 0)
    assert g.n_states == 65 and g.gain.min() == g.gain[63, 2] == -63 and g.next[63, 2] == 0
    assert g.walk([1] * 63) == (63, 0) and g.walk([1] * 130) == (130, 128) and g.walk([1] * 63 + [2, 1]) == (1, 0)
    with pytest.raises(ValueError, match='65 labels'):
        ContextGraph([[1] * 65], 2, 0)
    with pytest.raises(ValueError, match='0 labels'):
        ContextGraph([[]], 2, 0)
    for bad in ([0], [1, 5], [-1]):
        with pytest.raises(ValueError, match='phrase 1 holds'):
            ContextGraph([[1], bad], 5, 0)
    with pytest.raises(ValueError, match='duplicate'):
        ContextGraph([[1, 2], [2], [1, 2]], 3, 0)
    # 1024 phrases of two labels; one more is refused
    two = [[a, b] for a in range(1, 34) for b in range(1, 34)]
    assert ContextGraph(two[:1024], 34, 0).n_states == 1 + 32 + 1024
    with pytest.raises(ValueError, match='1025 phrases'):
        ContextGraph(two[:1025], 34, 0)
    # 32768 states exactly: the root, 32 first labels, and 1024 phrases with distinct first two labels, 991 of 33 labels and
    # 33 of 32 (1 + 32 + 991 * 32 + 33 * 31); one label more is refused
    body = [[1 + k // 32, 1 + k % 32] + [1 + (k + j) % 32 for j in range(31 if k < 991 else 30)] for k in range(1024)]
    g = ContextGraph(body, 33, 0)
    assert g.n_states == 32768 and g.trans.shape == (32768, 33) and int((g.trans & 0xFFFF).max()) == 32767
    assert g.gain.min() >= -63 and g.gain.max() == 1 and g.final.max() <= 0
    rng = np.random.RandomState(3)
    for k in rng.randint(0, 1024, size=6):
        y = body[k][:-1] + body[(k + 7) % 1024] + [5]
        assert g.walk(y) == (bias_ref.V(y, body), bias_ref.F(y, body))
    body[-1] = body[-1] + [1]
    with pytest.raises(ValueError, match='32769 states'):
        ContextGraph(body, 33, 0)


def test_phrase_booster_normalises_and_refuses_by_name():
    from codes.bias import PhraseBooster
    from codes.search import KeywordSearcher
    alphabet = json.load(open(os.path.join(ROOT, 'data', 'labels.en.json')))
    phrases = ['new york', "Don't", ' a ']
    b = PhraseBooster(alphabet, phrases, weight=1.5)
    s = KeywordSearcher(alphabet, phrases)
    assert b.keywords == s.keywords == ['NEW YORK', "DON'T", ' A '] and b.labels == s.labels
    assert b.weight == 1.5 and b.graph.n_states == 1 + 8 + 5 + 3 and b.graph.n_labels == len(alphabet)
    assert PhraseBooster(alphabet, ['cat']).weight == 2.0
    for bad, word in ((['cat', '123!?'], "'123!?'"), (['x' * 65], '65 labels'), (['cat', 'dog', 'CAT!'], "'CAT!'"),
                      (['under_score'], "'under_score'"), (['cat', ''], "''")):
        with pytest.raises(ValueError) as err:
            PhraseBooster(alphabet, bad)
        assert word in str(err.value) and 'PhraseBooster' in str(err.value), str(err.value)
    with pytest.raises(ValueError, match='no phrases'):
        PhraseBooster(alphabet, [])
    with pytest.raises(ValueError, match='not a finite'):
        PhraseBooster(alphabet, ['cat'], weight=float('inf'))
    letters = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ'
    many = [a + b2 for a in letters for b2 in letters] + ['A' + a + b2 for a in letters[:14] for b2 in letters]
    assert len(PhraseBooster(alphabet, many[:1024]).labels) == 1024
    with pytest.raises(ValueError, match='1025 phrases'):
        PhraseBooster(alphabet, many[:1025])
    long = [letters[k // 26] + letters[k % 26] + ''.join(letters[(k + j) % 26] for j in range(62)) for k in range(600)]
    with pytest.raises(ValueError, match='states; the most is 32768'):
        PhraseBooster(alphabet, long)
    assert len(PhraseBooster(alphabet, ['x' * 64]).labels[0]) == 64


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize('w', [1, 3, 16])
def test_reference_with_a_root_only_graph_is_beam_ref(w):
    rng = np.random.RandomState(w)
    lp = beam_ref.frame_log_probs(_softmax(rng.standard_normal((12, 6)) * 2.0), False)
    root = np.zeros((1, 6), np.int32), np.zeros(1, np.int32)
    s0, s1 = {}, {}
    want = beam_ref.beam_search(lp, 0, w, stats=s0)
    got = bias_ref.beam_search_bias(lp, 0, w, root[0], root[1], 3.0, stats=s1)
    assert got[:4] == want and got[4] == 0 and s0 == s1
    # and a real graph at weight 0: the same labelling and scores, with its count
    paths, nxt, gain, final = bias_ref.tables([[1, 2], [3]], 6, 0)
    got = bias_ref.beam_search_bias(lp, 0, w, bias_ref.pack(nxt, gain), final, 0.0)
    assert got[:4] == want and got[4] == bias_ref.F(want[0], [[1, 2], [3]])


def test_reference_boost_changes_the_labelling_and_counts_f():
    # frames: C, A, then B (0.4) or T (0.6): CAT without a boost, CAB with CAB boosted, CAT again with only CABS
    blank, C, A, B, T, S = 0, 1, 2, 3, 4, 5
    rows = np.full((6, 6), 1e-4, np.float32)
    for t, c in enumerate((C, blank, A, blank)):
        rows[t, c] = 1.0
    rows[4, T], rows[4, B] = 0.6, 0.4
    rows[5, blank] = 1.0
    lp = beam_ref.frame_log_probs(rows, False)

    def run(phrases, w):
        _, nxt, gain, final = bias_ref.tables(phrases, 6, blank)
        return bias_ref.beam_search_bias(lp, blank, 8, bias_ref.pack(nxt, gain), final, w)
    assert run([[C, A, B]], 0.0)[0] == [C, A, T]
    got = run([[C, A, B]], 1.0)
    assert got[0] == [C, A, B] and got[4] == 3 and got[2] == got[3] + 3.0
    got = run([[C, A, B, S]], 1.0)
    assert got[0] == [C, A, T] and got[4] == 0 and got[2] == got[3]
    bad = bias_ref.pack(*bias_ref.tables([[C, A, B]], 6, blank)[1:3]) | 0x7000
    _, nxt, gain, final = bias_ref.tables([[C, A, B]], 6, blank)
    assert np.array_equal(bias_ref.sanitised(bad, 4) & 0xFFFF, np.zeros_like(bad))
    assert np.array_equal(bias_ref.sanitised(bad, 4) >> 16, gain)
    assert np.array_equal(bias_ref.sanitised(bias_ref.pack(nxt, gain), 4), bias_ref.pack(nxt, gain))


def test_bias_entry_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    fn = lib.load().ds2_ctc_beam_search_bias
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    # probs sizes B T A blank W log | ngram cap word cap order unit bos eos unk space alpha beta oov | trans final S w |
    # ws ws_bytes labels offsets len score ctc bias stream
    ok = [one, one, 1, 4, 5, 0, 4, 0, None, 0, None, 0, 1, 0, -1, -1, -1, -1, 0.0, 0.0, 0.0, one, one, 3, 2.0,
          one, 1 << 20, one, one, one, one, one, one, None]

    def refused(changes):
        args = list(ok)
        for pos, val in changes:
            args[pos] = val
        rc = fn(*args)
        return rc, lib.load().ds2_last_error().decode()
    for pos, bad in ((23, 0), (23, -1), (23, 32769), (21, None), (22, None), (32, None), (24, float('inf')),
                     (24, float('-inf')), (24, float('nan'))):
        rc, msg = refused([(pos, bad)])
        assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_bias' in msg, (pos, bad, msg)
    assert 'states' in refused([(23, 32769)])[1] and 'finite' in refused([(24, float('nan'))])[1]
    assert 'NULL' in refused([(21, None)])[1]
    # and the refusals it shares with the batch entry, under its own name
    for pos, bad in ((6, 0), (6, 129), (4, 129), (5, 5), (1, None), (27, None), (26, 8), (13, 3)):
        rc, msg = refused([(pos, bad)])
        assert rc == lib.ERR_ARG and 'ds2_ctc_beam_search_bias' in msg, (pos, bad, msg)
    assert refused([(2, 0), (23, 32768)])[0] == 0                       # B = 0: nothing to do, and S at its limit is taken
