"""The pure-Python statement of the device search's contract (tests/beam_ref.py) against the host search
ds2_ctc_beam_search on the CPU: with no LM both must find the same labelling and log-probability."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from tests import beam_ref


def _softmax(rng, t, a):
    x = rng.standard_normal((t, a)) * 2.0
    e = np.exp(x - x.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize('a, w', [(5, 1), (5, 4), (8, 16), (29, 8)])
def test_reference_search_matches_the_host_search(a, w):
    from ds2hip import lib
    rng = np.random.default_rng(a * 100 + w)
    for t in (0, 1, 7, 25):
        probs = _softmax(rng, t, a) if t else np.zeros((0, a), np.float32)
        lab, off, score, ctc = beam_ref.beam_search(beam_ref.frame_log_probs(probs, False), 0, w)
        ids, offs = np.zeros(max(t, 1), np.int32), np.zeros(max(t, 1), np.int32)
        n, lp = ctypes.c_int(0), ctypes.c_float(0)
        lib.host_call('ds2_ctc_beam_search', np.ascontiguousarray(probs), t, a, 0, w, 0, ids, offs, len(ids), n, lp)
        assert lab == ids[:n.value].tolist()
        assert abs(ctc - lp.value) <= 1e-5 * max(1.0, abs(ctc)) and score == ctc


def test_exact_zero_probabilities():
    from ds2hip import lib
    rng = np.random.default_rng(3)
    probs = _softmax(rng, 20, 6)
    probs[rng.random(probs.shape) < 0.3] = 0.0
    probs[:, 0] = np.maximum(probs[:, 0], 0.05)
    lab, _, _, ctc = beam_ref.beam_search(beam_ref.frame_log_probs(probs, False), 0, 8)
    ids, offs = np.zeros(20, np.int32), np.zeros(20, np.int32)
    n, lp = ctypes.c_int(0), ctypes.c_float(0)
    lib.host_call('ds2_ctc_beam_search', probs, 20, 6, 0, 8, 0, ids, offs, 20, n, lp)
    assert lab == ids[:n.value].tolist() and abs(ctc - lp.value) < 1e-5


def _host_search(probs, blank, w):
    from ds2hip import lib
    t, a = probs.shape
    ids, offs = np.zeros(max(t, 1), np.int32), np.zeros(max(t, 1), np.int32)
    n, lp = ctypes.c_int(0), ctypes.c_float(0)
    lib.host_call('ds2_ctc_beam_search', np.ascontiguousarray(probs), t, a, blank, w, 0, ids, offs, len(ids), n, lp)
    return ids[:n.value].tolist(), lp.value


@pytest.mark.parametrize('a', [1, 2, 5, 29])
def test_nonzero_blank_matches_the_host_search(a):
    rng = np.random.default_rng(a)
    for blank in sorted({a - 1, a // 2}):
        for w in (1, 3, 16):
            for t in (1, 9, 30):
                probs = _softmax(rng, t, a)
                lp = beam_ref.frame_log_probs(probs, False)
                stats = {}
                lab, _, score, ctc = beam_ref.beam_search(lp, blank, w, stats=stats)
                assert not any(tie for tie, _ in stats['cut']) and not stats['pick'][0]
                want, want_lp = _host_search(probs, blank, w)
                assert lab == want, (a, blank, w, t)
                assert blank not in lab
                assert abs(ctc - want_lp) <= 1e-5 * max(1.0, abs(ctc)) and score == ctc


# Ties settled by hand (DESIGN.md "Device CTC beam search"): at the W-th key the lower candidate index i*A + c wins, the
# stay of slot i being i*A + blank; at the final pick the lower slot wins.  (name, probs (T, A), blank, W, labels, offsets)
HAND_TIES = [
    ('cut_between_extensions', [[0.2, 0.35, 0.35, 0.1]], 0, 1, [1], [0]),
    ('cut_stay_before_extension', [[0.1, 0.2, 0.35, 0.35]], 2, 1, [], []),
    ('cut_extension_before_stay', [[0.1, 0.35, 0.2, 0.35]], 3, 1, [1], [0]),
    ('final_pick_lower_slot', [[0.1, 0.4, 0.4, 0.1]], 0, 2, [1], [0]),
    ('cut_then_pick', [[0.1, 0.3, 0.3, 0.3], [0.6, 0.2, 0.1, 0.1]], 0, 2, [1], [0]),
]


@pytest.mark.parametrize('case', HAND_TIES, ids=[c[0] for c in HAND_TIES])
def test_hand_derived_ties(case):
    _, probs, blank, w, labels, offsets = case
    stats = {}
    lab, off, _, _ = beam_ref.beam_search(beam_ref.frame_log_probs(np.float32(probs), False), blank, w, stats=stats)
    assert (lab, off) == (labels, offsets)
    assert any(tie for tie, _ in stats['cut']) or stats['pick'][0]


def test_tie_statistics():
    lp = beam_ref.frame_log_probs(np.float32([[0.2, 0.35, 0.35, 0.1], [0.5, 0.3, 0.1, 0.1]]), False)
    stats = {}
    beam_ref.beam_search(lp, 0, 1, stats=stats)
    (tie0, gap0), (tie1, gap1) = stats['cut']
    tau = math.log(np.float32(0.35))
    assert tie0 and abs(gap0 - (tau - math.log(np.float32(0.2))) / abs(tau)) < 1e-12
    assert not tie1 and gap1 > 0.1
    assert stats['pick'] == (False, math.inf)
    stats = {}
    beam_ref.beam_search(lp, 0, 16, stats=stats)               # never more candidates than W: no cut
    assert stats['cut'] == [] and stats['pick'][0] is False


def _tiny_lm(tmp_path, labels, unit, blank):
    from codes.lm import NGramLM
    if unit == 'char':
        text = ('\\data\\\nngram 1=5\nngram 2=4\n\n\\1-grams:\n-99\t<s>\t-0.3\n-0.6\t</s>\n-0.5\tA\t-0.2\n'
                '-0.9\tB\t-0.1\n-0.7\t<space>\n\n\\2-grams:\n-0.1\t<s> B\n-0.2\tA A\n-0.4\tB </s>\n-0.3\t<space> A\n'
                '\n\\end\\\n')
    else:
        text = ('\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-99\t<s>\t-0.2\n-0.5\t</s>\n-0.8\tab\t-0.3\n'
                '-0.6\ta\n-1.2\t<unk>\n\n\\2-grams:\n-0.2\t<s> ab\n-0.1\tab a\n-0.3\ta </s>\n\n\\end\\\n')
    p = tmp_path / ('tiny_%s.arpa' % unit)
    p.write_text(text)
    return NGramLM.from_arpa(str(p), labels, unit=unit, blank_index=blank)


def exhaustive_best(lp, blank, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    """argmax over labellings of log p(l) + alpha LM + beta N by enumerating every alignment -> (labels, fused, ctc,
    margin to the runner-up)."""
    t, a = lp.shape
    total = {}
    for al in itertools.product(range(a), repeat=t):
        seq, prev = [], -1
        for c in al:
            if c != blank and c != prev:
                seq.append(c)
            prev = c
        v = sum(lp[i, c] for i, c in enumerate(al))
        k = tuple(seq)
        total[k] = np.logaddexp(total[k], v) if k in total else v
    fused = {k: v + (beam_ref.lm_score(lm, list(k), alpha, beta, space_id) if lm else 0.0) for k, v in total.items()}
    best = max(fused, key=fused.get)
    second = max((v for k, v in fused.items() if k != best), default=-math.inf)
    return list(best), fused[best], total[best], fused[best] - second


@pytest.mark.parametrize('unit', [None, 'char', 'word'])
@pytest.mark.parametrize('order', [('A', ' ', 'B', '_'), ('A', '_', ' ', 'B')])
def test_nonzero_blank_matches_exhaustive_enumeration(tmp_path, unit, order):
    labels = list(order)
    blank, space = labels.index('_'), labels.index(' ')
    lm = _tiny_lm(tmp_path, labels, unit, blank) if unit else None
    alpha, beta = (0.9, 0.4) if unit else (0.0, 0.0)
    rng = np.random.default_rng(len(unit or '') + blank)
    for _ in range(4):
        probs = _softmax(rng, 4, 4)
        lp = beam_ref.frame_log_probs(probs, False)
        lab, _, score, ctc = beam_ref.beam_search(lp, blank, 128, lm, alpha, beta, space)
        best, fused, total, margin = exhaustive_best(np.log(probs.astype(np.float64)), blank, lm, alpha, beta, space)
        assert margin > 1e-6
        assert lab == best
        assert abs(score - fused) <= 1e-9 and abs(ctc - total) <= 1e-9
