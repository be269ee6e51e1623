"""ds2_ctc_beam_search_rows against ds2_ctc_beam_search_batch: row r of a rows launch is, bit for bit, what the batch entry
gives for utterance utt[r] with (alpha[r], beta[r]) -- whatever else shares the launch."""
import numpy as np
import pytest
import torch

from tests.test_beam_edges_gpu import LABELS, _make_lm

pytestmark = pytest.mark.gpu
B, T, A = 3, 40, len(LABELS)
SIZES = [40, 0, 27]
SPACE = LABELS.index(' ')
PAIRS = [(0.0, 0.0), (0.8, 1.0), (2.0, 0.0), (0.3, -0.5)]


@pytest.fixture(scope='module')
def lms(tmp_path_factory):
    d = tmp_path_factory.mktemp('rows_lm')
    return {'none': None, 'char': _make_lm(d, 6, 'char')[0], 'word': _make_lm(d, 3, 'word')[0]}


@pytest.fixture(scope='module')
def inputs():
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((B, T, A))
    e = np.exp(x - x.max(-1, keepdims=True))
    probs = torch.from_numpy((e / e.sum(-1, keepdims=True)).astype(np.float32)).cuda()
    return probs, torch.tensor(SIZES, dtype=torch.int32, device='cuda')


_REF = {}


def _ref(inputs, lms, kind, w, pair):
    """ops.ctc_beam_search of the whole batch, once per distinct (LM, width, alpha, beta)."""
    from ds2hip import ops
    key = (kind, w, pair)
    if key not in _REF:
        _REF[key] = ops.ctc_beam_search(inputs[0], inputs[1], w, 0, False, lms[kind], pair[0], pair[1], SPACE)
    return _REF[key]


def _run(inputs, lms, kind, w, rows):
    from ds2hip import ops
    utt = torch.tensor([r[0] for r in rows], dtype=torch.int32, device='cuda')
    alpha = torch.tensor([r[1][0] for r in rows], dtype=torch.float32, device='cuda')
    beta = torch.tensor([r[1][1] for r in rows], dtype=torch.float32, device='cuda')
    return ops.ctc_beam_search_rows(inputs[0], inputs[1], utt, alpha, beta, w, 0, False, lms[kind], SPACE)


def _check(inputs, lms, kind, w, rows):
    out = _run(inputs, lms, kind, w, rows)
    assert [tuple(o.shape) for o in out] == [(len(rows), T), (len(rows), T), (len(rows),), (len(rows),), (len(rows),)]
    for r, (u, pair) in enumerate(rows):
        if 0 <= u < B:
            want = [o[u] for o in _ref(inputs, lms, kind, w, pair)]
        else:
            ninf = torch.tensor(float('-inf'), device='cuda')
            want = [torch.zeros(T, dtype=torch.int32, device='cuda'), torch.zeros(T, dtype=torch.int32, device='cuda'),
                    torch.tensor(0, dtype=torch.int32, device='cuda'), ninf, ninf]
        for name, got, exp in zip(('labels', 'offsets', 'len', 'score', 'ctc_logp'), out, want):
            assert torch.equal(got[r], exp), (kind, w, r, u, pair, name)
    return out


@pytest.mark.parametrize('w', [1, 16, 128])
@pytest.mark.parametrize('kind', ['none', 'char', 'word'])
def test_rows_equal_the_batch_entry(inputs, lms, kind, w):
    every = [(u, p) for p in PAIRS for u in range(B)]
    rng = np.random.default_rng(w)
    _check(inputs, lms, kind, w, [every[i] for i in rng.permutation(len(every))])      # rows permuted
    _check(inputs, lms, kind, w, [(2, p) for p in PAIRS])                               # one utterance, four weight pairs
    _check(inputs, lms, kind, w, [(u, PAIRS[1]) for u in range(B)])                     # one pair on all utterances
    for row in ((0, PAIRS[3]), (1, PAIRS[1])):                                          # R = 1 (utterance 1 has no frames)
        _check(inputs, lms, kind, w, [row])
    # a utt of -1 and of B: the empty result, the neighbours unchanged
    _check(inputs, lms, kind, w, [(0, PAIRS[1]), (-1, PAIRS[1]), (2, PAIRS[2]), (B, PAIRS[0]), (0, PAIRS[3])])


@pytest.mark.parametrize('kind', ['none', 'char'])
def test_more_rows_than_compute_units(inputs, lms, kind):
    rng = np.random.default_rng(7)
    rows = [(int(rng.integers(0, B)), PAIRS[int(rng.integers(0, len(PAIRS)))]) for _ in range(300)]
    out = _check(inputs, lms, kind, 16, rows)
    if kind == 'char':      # a bonus per character changes the labelling: the sweep is not comparing a constant with itself
        full = [torch.cat([o[0].reshape(-1), o[2]]) for o in (_ref(inputs, lms, kind, 16, p) for p in PAIRS)]
        assert any(not torch.equal(full[0], f) for f in full[1:])
    assert out[0].shape == (300, T)


def test_no_lm_ignores_the_weights(inputs, lms):
    out = _run(inputs, lms, 'none', 16, [(0, (5.0, -3.0)), (0, (0.0, 0.0))])
    for o in out:
        assert torch.equal(o[0], o[1])


def test_rows_arguments(inputs):
    from ds2hip import lib, ops
    probs, sizes = inputs
    empty_i = torch.zeros((0,), dtype=torch.int32, device='cuda')
    empty_f = torch.zeros((0,), dtype=torch.float32, device='cuda')
    out = ops.ctc_beam_search_rows(probs, sizes, empty_i, empty_f, empty_f, 16)          # R = 0 is fine
    assert out[0].shape == (0, T) and out[2].shape == (0,)
    utt = torch.zeros((2,), dtype=torch.int32, device='cuda')
    w2 = torch.zeros((2,), dtype=torch.float32, device='cuda')
    with pytest.raises(lib.Ds2Error, match='beam_width 129'):
        ops.ctc_beam_search_rows(probs, sizes, utt, w2, w2, 129)
    with pytest.raises(RuntimeError, match='one per entry of utt'):
        ops.ctc_beam_search_rows(probs, sizes, utt, w2[:1], w2, 16)
    with pytest.raises(RuntimeError, match='utt must be torch.int32'):
        ops.ctc_beam_search_rows(probs, sizes, utt.long(), w2, w2, 16)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.ctc_beam_search_rows(probs, sizes, utt.cpu(), w2, w2, 16)
    # a workspace sized for fewer rows is refused with the needed size
    labels = torch.empty((2, T), dtype=torch.int32, device='cuda')
    lens = torch.empty((2,), dtype=torch.int32, device='cuda')
    score = torch.empty((2,), dtype=torch.float32, device='cuda')
    need = lib.query('ds2_ctc_beam_ws_bytes', 2, T, 16)
    ws = torch.empty((need - 1,), dtype=torch.uint8, device='cuda')
    with pytest.raises(lib.Ds2Error, match='ds2_ctc_beam_ws_bytes = %d' % need):
        lib.call('ds2_ctc_beam_search_rows', probs, sizes, utt, w2, w2, B, 2, T, A, 0, 16, 0, None, 0, None, 0, 1, 0, -1, -1,
                 -1, -1, 0.0, ws, need - 1, labels, labels.clone(), lens, score, score.clone())
