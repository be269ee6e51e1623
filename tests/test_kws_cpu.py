"""Keyword search without a GPU: tests/kws_ref.py against brute force on tiny cases and against hand-worked cases, the
refusals of codes.search.KeywordSearcher, and search.py's record assembly from given hits."""
import itertools
import json
import os

import numpy as np
import pytest

from tests import kws_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -np.inf


def _brute(e, labels, blank, t0, t):
    """The best score over every CTC alignment of the labels to frames t0..t that starts in l1's state, ends in lL's and
    never skips between equal neighbours; -inf if there is none."""
    n_states = 2 * len(labels) - 1
    ext = [labels[s // 2] if s % 2 == 0 else blank for s in range(n_states)]
    best = NEG
    for steps in itertools.product((0, 1, 2), repeat=t - t0):
        s, total, ok = 0, float(e[t0][ext[0]]), True
        for i, d in enumerate(steps):
            s2 = s + d
            if s2 >= n_states or (d == 2 and (s2 % 2 == 1 or ext[s2] == ext[s])):
                ok = False
                break
            s = s2
            total += float(e[t0 + 1 + i][ext[s]])
        if ok and s == n_states - 1:
            best = max(best, total)
    return best


@pytest.mark.parametrize('labels', [[1], [2], [1, 2], [1, 1], [2, 1]])
def test_reference_equals_brute_force_on_tiny_dyadic_cases(labels):
    rng = np.random.RandomState(7 + 10 * labels[0] + len(labels))
    for case in range(12):
        t_n = int(rng.randint(1, 7))
        logp = (-0.25 * rng.randint(0, 12, size=(t_n, 3))).astype(np.float32)       # dyadic: every sum is exact
        if case % 3 == 0:
            logp[rng.randint(t_n), rng.randint(3)] = NEG
        e = ref.emissions(logp, t_n)
        assert e.max() <= 0 and (e.max(axis=1) == 0).all()
        d, st = ref.ends(e, labels, 0)
        for t in range(t_n):
            want = max(_brute(e, labels, 0, t0, t) for t0 in range(t + 1))
            assert d[t] == want, (case, t)
            if want > NEG:
                assert 0 <= st[t] <= t and _brute(e, labels, 0, int(st[t]), t) == want, (case, t)


def _frames(rows):
    return np.asarray(rows, np.float32)


BLANK_TOP, L1_TOP, L1_COSTLY = [0, -4, -4], [-4, 0, -4], [0, -1, -4]


def test_tie_at_state_zero_zero_cost_run_starts_at_its_first_frame():
    logp = _frames([BLANK_TOP, BLANK_TOP, L1_TOP, L1_TOP, L1_TOP, BLANK_TOP])
    d, st = ref.ends(ref.emissions(logp, 6), [1], 0)
    assert d.tolist() == [-4, -4, 0, 0, 0, -4]
    assert st.tolist() == [0, 1, 2, 2, 2, 2]                # stay wins the tie with a fresh start
    # the plateau: three candidates of one score and one start become one hit whose end is the last of them
    assert ref.search_pair(logp, 6, [1], -0.5) == [(2, 4, 0.0)]


def test_costly_run_starts_at_its_last_frame_threshold_is_inclusive_and_count_exceeds_max_hits():
    logp = _frames([BLANK_TOP, BLANK_TOP, L1_COSTLY, L1_COSTLY, L1_COSTLY, BLANK_TOP])
    d, st = ref.ends(ref.emissions(logp, 6), [1], 0)
    assert d.tolist() == [-4, -4, -1, -1, -1, -4]
    assert st.tolist() == [0, 1, 2, 3, 4, 5]                # a fresh start (0) beats carrying -1 on
    found = ref.search_pair(logp, 6, [1], -1.0)             # D == min_score counts
    assert found == [(2, 2, -1.0), (3, 3, -1.0), (4, 4, -1.0)]
    assert ref.search_pair(logp, 6, [1], np.nextafter(-1.0, 0.0)) == []
    hits, score, count = ref.pack(found, 2)
    assert count == 3 and hits.tolist() == [[2, 2], [3, 3]] and score.tolist() == [-1.0, -1.0]
    hits, score, count = ref.pack(found, 4)
    assert count == 3 and hits[3].tolist() == [-1, -1] and score[3] == NEG


def test_two_labels_with_and_without_a_skip():
    # "12": l1 at frame 1, l2 at frame 2 directly (the skip over the blank); "11" needs the blank between
    logp = _frames([BLANK_TOP, L1_TOP, [-4, -4, 0], [-4, 0, -4], BLANK_TOP])
    assert ref.search_pair(logp, 5, [1, 2], -0.5) == [(1, 2, 0.0)]
    d, st = ref.ends(ref.emissions(logp, 5), [1, 1], 0)
    # l1 (t=1), blank (t=2, cost 4), l1 (t=3) is the only way through by t=3
    assert d[3] == -4.0 and st[3] == 1
    assert ref.search_pair(logp, 5, [1, 1], -0.5) == []
    assert ref.search_pair(logp, 3, [1, 2], -0.5) == [(1, 2, 0.0)] and ref.search_pair(logp, 2, [1, 2], -0.5) == []


def test_the_cluster_rule_branch_by_branch():
    # replace by a greater score; drop a lower one; extend across a dip at the same score and start; drop below threshold
    d = np.asarray([-9, -2, -1, -3, -1, -5, -2], np.float64)
    st = np.asarray([0, 0, 1, 1, 1, 5, 2])
    assert ref.cluster(d, st, -4.0) == [(1, 4, -1.0)]
    # a start after the current end emits; the same score with the same start extends
    assert ref.cluster(np.asarray([-1., -1., -1.]), np.asarray([0, 0, 2]), -4.0) == [(0, 1, -1.0), (2, 2, -1.0)]
    # the same score with another start that is not after the end is dropped
    assert ref.cluster(np.asarray([-1., -1., -1.]), np.asarray([0, 0, 1]), -4.0) == [(0, 1, -1.0)]
    # a hit may begin before the previous one ends: only a cluster's first candidate is held against that end
    assert ref.cluster(np.asarray([-2., -3., -1.]), np.asarray([0, 1, 0]), -4.0) == [(0, 0, -2.0), (0, 2, -1.0)]
    assert ref.cluster(d, st, np.nan) == [] and ref.cluster(d[:0], st[:0], -4.0) == []


def test_bad_keywords_nan_and_padding_in_the_reference():
    logp = _frames([L1_TOP, L1_TOP, [np.nan, np.nan, np.nan]])
    for bad in ([], [0], [3], [-1], [1] * 65):
        assert ref.search_pair(logp, 2, bad, -100.0) == []
    assert ref.search_pair(logp, 2, [1] * 64, -100.0) == []            # 127 states never fit two frames
    assert ref.search_pair(logp, 2, [1], -0.5) == [(0, 1, 0.0)]         # the NaN frame is padding
    e = ref.emissions(_frames([[np.nan, -1, -2], [NEG, NEG, NEG]]), 2)
    assert e.tolist() == [[NEG, 0, -1], [NEG, NEG, NEG]]
    hits, score, count = ref.search_batch(logp[None], [9], [[1], [2, 2]], [-0.5, -0.5], max_hits=2)
    assert count.tolist() == [[1, 0]]                                    # sizes is clamped to T; the NaN frame costs -inf
    assert hits[0, 0].tolist() == [[0, 1], [-1, -1]] and score[0, 0].tolist() == [0.0, NEG]
    assert (hits[0, 1] == -1).all() and (score[0, 1] == NEG).all()


def test_keyword_searcher_refuses_by_name_and_scales_the_threshold():
    from codes.search import KeywordSearcher
    alphabet = json.load(open(os.path.join(ROOT, 'data', 'labels.en.json')))
    s = KeywordSearcher(alphabet, ['chapter one', "Don't", ' a '], min_score_per_char=-0.75, max_hits=3)
    assert s.keywords == ['CHAPTER ONE', "DON'T", ' A ']
    assert s.labels[2] == [1, 3, 1] and s.max_hits == 3
    assert s.min_score.dtype == np.float64 and s.min_score.tolist() == [-0.75 * 11, -0.75 * 5, -0.75 * 3]
    for phrases, word in ((['cat', '123!?'], "'123!?'"), (['x' * 65], '65 labels'), (['cat', 'dog', 'CAT!'], "'CAT!'"),
                          (['under_score'], "'under_score'"), (['cat', ''], "''")):
        with pytest.raises(ValueError) as err:
            KeywordSearcher(alphabet, phrases)
        assert word in str(err.value), str(err.value)
    with pytest.raises(ValueError):
        KeywordSearcher(alphabet, [])
    with pytest.raises(ValueError):
        KeywordSearcher(alphabet, ['cat'], max_hits=65)
    assert len(KeywordSearcher(alphabet, ['x' * 64]).labels[0]) == 64
    # records(): only the counted rows, by keyword and then by row
    hits = np.full((1, 3, 3, 2), -1, np.int32)
    score = np.full((1, 3, 3), NEG)
    hits[0, 1, :2] = [[4, 6], [9, 12]]
    score[0, 1, :2] = [-2.5, 0.0]
    hits[0, 2, :] = [[0, 0], [1, 1], [2, 2]]
    score[0, 2, :] = -3.0
    found = s.records(hits, score, np.asarray([[0, 2, 7]], np.int32))
    assert found == [[
        {'keyword': "DON'T", 'utterance': 0, 'start_frame': 4, 'end_frame': 6, 'score': -2.5, 'score_per_char': -0.5},
        {'keyword': "DON'T", 'utterance': 0, 'start_frame': 9, 'end_frame': 12, 'score': 0.0, 'score_per_char': 0.0},
        {'keyword': ' A ', 'utterance': 0, 'start_frame': 0, 'end_frame': 0, 'score': -3.0, 'score_per_char': -1.0},
        {'keyword': ' A ', 'utterance': 0, 'start_frame': 1, 'end_frame': 1, 'score': -3.0, 'score_per_char': -1.0},
        {'keyword': ' A ', 'utterance': 0, 'start_frame': 2, 'end_frame': 2, 'score': -3.0, 'score_per_char': -1.0}]]


def test_search_cli_assembles_records_from_given_hits(tmp_path):
    import search
    hit = lambda kw, a, b, sc: {'keyword': kw, 'utterance': 0, 'start_frame': a, 'end_frame': b, 'score': sc,  # noqa: E731
                                'score_per_char': sc / len(kw)}
    # segment 1 starts at block 250 = 2.5 s; output step t is centred (2 t + 5) * 0.01 s into it
    later = search.hit_entries(1, 250, [hit('ON', 10, 12, -1.0), hit('CAT', 10, 14, -3.0)])
    assert later == [
        {'keyword': 'ON', 'start': 2.75, 'end': 2.79, 'score': -1.0, 'score_per_char': -0.5, 'segment': 1},
        {'keyword': 'CAT', 'start': 2.75, 'end': 2.83, 'score': -3.0, 'score_per_char': -1.0, 'segment': 1}]
    first = search.hit_entries(0, 20, [hit('ON', 40, 41, 0.0)])
    stats = {'noise_floor_db': -60.456, 'threshold_db': -48.449, 'speech_seconds': 3.21}
    rec = search.file_record('a.wav', 80000, stats, ['CAT', 'ON'], later + first, 2)
    assert list(rec) == ['path', 'duration', 'noise_floor_db', 'threshold_db', 'speech_seconds', 'keywords', 'truncated',
                         'hits']
    assert rec['path'] == 'a.wav' and rec['duration'] == 5.0 and rec['noise_floor_db'] == -60.46
    assert rec['threshold_db'] == -48.45 and rec['speech_seconds'] == 3.21
    assert rec['keywords'] == ['CAT', 'ON'] and rec['truncated'] == 2
    # by start, then by keyword ORDER (CAT before ON), not by the order given
    assert [(h['keyword'], h['start'], h['segment']) for h in rec['hits']] == [
        ('ON', 1.05, 0), ('CAT', 2.75, 1), ('ON', 2.75, 1)]
    json.dumps(rec)
    silent = search.file_record('s.wav', 32000, {'noise_floor_db': None, 'threshold_db': -60.51, 'speech_seconds': 0.0},
                                ['CAT'], [], 0)
    assert silent == {'path': 's.wav', 'duration': 2.0, 'noise_floor_db': None, 'threshold_db': -60.51,
                      'speech_seconds': 0.0, 'keywords': ['CAT'], 'truncated': 0, 'hits': []}
    kw_file = tmp_path / 'kw.txt'
    kw_file.write_text('chapter one\n\n  \nmister smith\r\n')
    assert search.read_phrases(['a b'], str(kw_file)) == ['a b', 'chapter one', 'mister smith']
    assert search.read_phrases(None, None) == []
