"""CTC forced alignment without a GPU: the host reference (tests/align_ref.py) against brute force, the time of an output
step, the word grouping of ``codes.align``, and the C ABI's new entry points."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import align_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(t_n, a_n):
    """Dyadic log-inputs (every sum exact): random eighths, random with -inf entries, a few levels (many exact ties), and
    all equal (everything ties)."""
    rng = np.random.default_rng(100 * t_n + a_n)
    x = rng.integers(-40, 1, size=(t_n, a_n)) / 8.0
    holes = x.copy()
    holes[rng.random((t_n, a_n)) < 0.25] = -np.inf
    levels = rng.integers(-2, 1, size=(t_n, a_n)).astype(np.float64)
    return [x, holes, levels, np.full((t_n, a_n), -1.0)]


TRANSCRIPTS = [list(p) for n in range(4) for p in itertools.product((1, 2), repeat=n)]


@pytest.mark.parametrize('t_n', range(0, 7))
def test_reference_equals_brute_force(t_n):
    """Every transcript of length 0-3 over A = 3 (repeats included), T <= 6: the same score and, through the tie rule, the
    same path; infeasible cases (more labels plus repeats than frames, -inf everywhere) are -inf in both."""
    seen_inf = seen_tie = 0
    for x in _inputs(t_n, 3):
        for labels in TRANSCRIPTS:
            want, want_states = align_ref.brute_force(x, labels)
            got, got_states = align_ref.viterbi(x, labels)
            assert got == want, (t_n, labels)
            if want_states is None:
                assert got_states is None
                seen_inf += 1
                continue
            assert got_states.tolist() == want_states.tolist(), (t_n, labels, x)
            assert align_ref.is_valid_path(got_states, len(labels), labels)
            assert align_ref.collapse(got_states, labels) == labels
            assert align_ref.path_score(x, got_states, labels)[0] == want
            seen_tie += 1
    assert seen_inf > 0 and (t_n == 0 or seen_tie > 0)


def test_reference_counts_repeats_and_bad_labels_as_infeasible():
    x = np.zeros((3, 3))
    assert align_ref.viterbi(x, [1, 1])[0] == 0.0                       # 1, blank, 1: exactly fits
    assert align_ref.viterbi(x[:2], [1, 1]) == (-np.inf, None)
    assert align_ref.viterbi(x, [1, 3]) == (-np.inf, None)              # outside the alphabet
    assert align_ref.viterbi(x, [0]) == (-np.inf, None)                 # the blank is no label
    nan = np.full((2, 3), np.nan)
    assert align_ref.viterbi(align_ref.frame_terms(nan, True), []) == (-np.inf, None)
    st, sa, en, sc = align_ref.align_batch(np.zeros((2, 4, 3)), [4, 0], [[1, 2], []], log_input=True)
    # all equal: the path that is highest from the last frame backwards -- final blank, stay, then down one state a frame
    assert st.tolist() == [[1, 3, 4, 4], [-1] * 4] and sa.tolist() == [[0, 1], [-1, -1]] and en.tolist() == sa.tolist()
    assert sc.tolist() == [0.0, 0.0]


def test_frame_to_seconds_matches_the_convolutions():
    from codes.align import ForcedAligner
    from ds2hip import ops
    assert ForcedAligner.frame_to_seconds(0) == pytest.approx(0.05)
    assert ForcedAligner.frame_to_seconds(100) == pytest.approx(2.05)
    assert ForcedAligner.frame_to_seconds(8) - ForcedAligner.frame_to_seconds(7) == pytest.approx(0.02)
    for t_in in (21, 22, 101, 1000, 1501):
        # centre of the taps each layer reads: conv1 step u reads frames 2u-10 .. 2u, conv2 step t reads conv1 steps t .. t+10
        t1, t_out = ops.conv_out_frames(t_in)
        # (conv1's last step ends inside the input padded by 10 frames, and one more step would not)
        assert 2 * (t1 - 1) <= t_in - 1 + 10 < 2 * t1 and t_out == t1 - 10
        for t in (0, t_out - 1):
            lo, hi = 2 * t - 10, 2 * (t + 10)
            assert ForcedAligner.frame_to_seconds(t) == pytest.approx(0.01 * (lo + hi) / 2)
            assert 0 <= (lo + hi) // 2 <= t_in - 1


def test_word_grouping():
    from codes.align import group_words
    mk = lambda s: [(c, 2 * i, 2 * i + 1) for i, c in enumerate(s)]     # noqa: E731
    assert group_words([]) == []
    assert group_words(mk('AB C')) == [('AB', 0, 3), ('C', 6, 7)]
    assert group_words(mk(' AB')) == [('AB', 2, 5)]
    assert group_words(mk('AB ')) == [('AB', 0, 3)]
    assert group_words(mk('A  B')) == [('A', 0, 1), ('B', 6, 7)]
    assert group_words(mk('  ')) == []


def test_align_entry_points_are_declared_bound_and_exported():
    from ds2hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, res, nargs in (('ds2_ctc_align_ws_bytes', 'size_t', 3), ('ds2_ctc_align', 'int', 18)):
        m = re.search(r'\n\s*%s\s+%s\s*\(([^;]*?)\)\s*;' % (res, name), code)
        assert m, name + ' is not declared in include/ds2hip.h'
        assert len(m.group(1).split(',')) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(handle, name), name + ' is not exported'
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404
    # host-side argument checks need no device
    assert lib.query('ds2_ctc_align_ws_bytes', 2, 10, 3) >= 2 * 10 * 7
    assert lib.query('ds2_ctc_align_ws_bytes', 2, 10, 30) >= 2 * 10 * 61
    one = ctypes.c_void_p(16)                                           # never dereferenced: the call is refused first
    rc = lib.load().ds2_ctc_align(one, one, one, one, one, 1, 4, 3, 512, 0, 1, one, 1 << 30, one, one, one, one, None)
    assert rc == lib.ERR_ARG and b'511' in lib.load().ds2_last_error()
    rc = lib.load().ds2_ctc_align(one, one, one, one, one, 1, 4, 3, 5, 0, 1, one, 8, one, one, one, one, None)
    assert rc == lib.ERR_ARG and b'workspace' in lib.load().ds2_last_error()


def test_ctc_align_refuses_cpu_tensors():
    from codes.align import ForcedAligner
    from ds2hip import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)                 # noqa: E731
    with pytest.raises(RuntimeError):
        ops.ctc_align(torch.full((1, 4, 3), 1 / 3.), i32(4), i32(1, 2), i32(0), i32(2), 2)
    with pytest.raises(RuntimeError):
        ForcedAligner(['_', 'A', 'B']).align(torch.full((1, 4, 3), 1 / 3.), i32(4), i32(1, 2), i32(2))
