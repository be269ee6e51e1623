"""tests/edit_ref.py, the Python statement of ds2_edit_stats, held to what already exists (oracle/host.py's distances), to
its own invariants and to a back-trace; and tune_lm.py's grid parser and ``best`` ordering.  No GPU."""
import numpy as np
import pytest

from oracle import host
from tests import edit_ref

SPACE = 0
CHARS = ' abc'          # label 0 is the space: an alphabet of 4, so that ties abound


def _text(labels):
    return ''.join(CHARS[c] for c in labels)


def _pairs(count=300, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        hyp = rng.integers(0, 4, size=rng.integers(0, 13)).tolist()
        ref = rng.integers(0, 4, size=rng.integers(0, 13)).tolist()
        out.append((hyp, ref))
    return out


PAIRS = _pairs()


def test_distances_equal_the_oracle_on_strings():
    for hyp, ref in PAIRS:
        row = edit_ref.edit_stats_row(hyp, ref, SPACE)
        assert row[0] == host.cer_distance(_text(hyp), _text(ref)), (hyp, ref)
        assert row[5] == host.wer_distance(_text(hyp), _text(ref)), (hyp, ref)
        assert row[4] == len(_text(ref).replace(' ', '')) and row[9] == len(_text(ref).split())


def test_count_invariants_and_backtrace():
    for hyp, ref in PAIRS:
        for items in (edit_ref.char_items, edit_ref.word_items):
            h, r = items(hyp, SPACE), items(ref, SPACE)
            dist, s, d, i, match = edit_ref.align_counts(h, r)
            assert s + d + i == dist
            assert len(r) == match + s + d and len(h) == match + s + i
            assert (dist, s, d, i, match) == edit_ref.backtrace_counts(h, r)
            assert edit_ref.align_counts_diag(h, r) == (dist, s, d, i)


def test_diagonal_sweep_equals_the_table_on_longer_sequences():
    rng = np.random.default_rng(11)
    for m, n in ((70, 41), (1, 90), (64, 64), (0, 5), (5, 0), (0, 0)):
        h, r = rng.integers(0, 3, size=m).tolist(), rng.integers(0, 3, size=n).tolist()
        assert edit_ref.align_counts_diag(h, r) == edit_ref.align_counts(h, r)[:4]


def _labels(text):
    return [CHARS.index(c) for c in text]


@pytest.mark.parametrize('hyp,ref,want', [
    # AB vs BA: distance 2; the tie rule substitutes twice (substitution first), not delete + insert
    ('ab', 'ba', [2, 2, 0, 0, 2, 1, 1, 0, 0, 1]),
    # only spaces: no items on either level
    ('   ', ' ', [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
    ('  ', 'ab', [2, 0, 2, 0, 2, 1, 0, 1, 0, 1]),
    # double, leading and trailing spaces make no word and no character
    (' ab  c ', 'ab c', [0, 0, 0, 0, 3, 0, 0, 0, 0, 2]),
    ('ab  c', ' ab c  ', [0, 0, 0, 0, 3, 0, 0, 0, 0, 2]),
    # a missing space: characters agree, two reference words against one
    ('abc', 'ab c', [0, 0, 0, 0, 3, 2, 1, 1, 0, 2]),
    ('', 'a b', [2, 0, 2, 0, 2, 2, 0, 2, 0, 2]),
    ('a b', '', [2, 0, 0, 2, 0, 2, 0, 0, 2, 0]),
])
def test_hand_cases(hyp, ref, want):
    assert edit_ref.edit_stats_row(_labels(hyp), _labels(ref), SPACE) == want


def test_space_id_minus_one_makes_one_word():
    row = edit_ref.edit_stats_row([1, 0, 2], [1, 0, 3], -1)
    assert row == [1, 1, 0, 0, 3, 1, 1, 0, 0, 1]


def test_batch_form_invalid_rows_and_totals():
    hyp = np.array([[1, 2, 0, 3], [1, 1, 1, 1], [2, 0, 2, 9], [3, 3, 3, 3]], dtype=np.int32)
    hyp_len = [4, 5, 3, 2]                       # row 1: a length past the stride
    ref, offs, lens = [1, 2, 0, 3, 2, 2], [0, 4], [4, 2]
    stats, totals = edit_ref.edit_stats(hyp, hyp_len, ref, offs, lens, 4, SPACE, ref_index=[0, 0, 1, 2], group=[1, 1, 0, 0],
                                        n_groups=2)
    assert stats[0] == [0, 0, 0, 0, 3, 0, 0, 0, 0, 2]
    assert stats[1] == [-1] * 10 and stats[3] == [-1] * 10          # bad hyp_len; ref_index 2 of 2 references
    assert stats[2] == edit_ref.edit_stats_row([2, 0, 2], [2, 2], SPACE)
    assert totals == [stats[2], stats[0]]


def test_grid_parser():
    import tune_lm
    assert tune_lm.parse_grid('0,0.5,1,2', '--betas') == [0.0, 0.5, 1.0, 2.0]
    assert tune_lm.parse_grid('0:2:0.25', '--alphas') == [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
    assert tune_lm.parse_grid('0.1:0.3:0.1', '--alphas') == [0.1, 0.2, 0.3]          # inclusive despite rounding
    assert tune_lm.parse_grid('0:1:0.4', '--alphas') == [0.0, 0.4, 0.8]
    assert tune_lm.parse_grid(' 1.5 ', '--alphas') == [1.5]
    assert tune_lm.parse_grid('-1:1:1', '--betas') == [-1.0, 0.0, 1.0]
    for bad in ('', ' ', 'a,b', '0:1', '0:1:0', '0:1:-1', '1:0:0.5', '0:1:0.1:2', '1,,2', 'nan', '0:inf:1'):
        with pytest.raises(ValueError, match='--alphas'):
            tune_lm.parse_grid(bad, '--alphas')
    with pytest.raises(ValueError, match='more than 4096'):
        tune_lm.parse_grid('0:5000:1', '--alphas')


def test_best_ordering():
    import tune_lm
    e = lambda a, b, w, c: {'alpha': a, 'beta': b, 'word_dist': w, 'char_dist': c}      # noqa: E731
    grid = [e(2.0, 0.0, 5, 9), e(1.0, 1.0, 4, 9), e(0.5, 2.0, 4, 7), e(0.5, 1.0, 4, 7), e(0.25, 3.0, 4, 8), e(0.75, 0.0, 4, 7)]
    assert tune_lm.best_point(grid) == e(0.5, 1.0, 4, 7)          # words, then chars, then alpha, then beta
    assert tune_lm.best_point(grid[:2]) == e(1.0, 1.0, 4, 9)
