"""The pure-Python statement of the device search's contract (tests/beam_ref.py) against the host search
ds2_ctc_beam_search on the CPU: with no LM both must find the same labelling and log-probability."""
import ctypes

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
