"""ds2_ctc_keyword_search against tests/kws_ref.py with ==: the chain is one fp32 subtraction and fp64 additions in a fixed
order, so there is nothing to tolerate.  Every output sits between sentinels, and so does the workspace's end."""
import numpy as np
import pytest
import torch

from tests import kws_ref as ref

pytestmark = pytest.mark.gpu
NEG = -np.inf
PAD = 64
I_SENT, F_SENT, W_SENT = 0x5A5A5A5A, 12345.678, 0xA5


def _keyword_tensors(keywords, dev):
    lens = np.asarray([len(k) for k in keywords], np.int32)
    offs = (np.cumsum(lens) - lens).astype(np.int32)
    flat = np.asarray([v for k in keywords for v in k] or [0], np.int32)
    return [torch.from_numpy(x).to(dev) for x in (flat, offs, lens)]


def _guarded(shape, dtype, fill, dev):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n].view(shape)


def _untouched(whole, fill):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def _launch(logp, sizes, keywords, min_score, max_hits, blank=0, ws_fill=None):
    """One call with guarded outputs -> (hits, hit_score, n_hits) as numpy arrays."""
    from ds2hip import lib
    dev = 'cuda'
    logp_d = torch.from_numpy(np.ascontiguousarray(logp, np.float32)).to(dev)
    n_b, n_t, n_a = logp_d.shape
    n_k = len(keywords)
    flat, offs, lens = _keyword_tensors(keywords, dev)
    sizes_d = torch.from_numpy(np.asarray(sizes, np.int32)).to(dev)
    thr = torch.from_numpy(np.asarray(min_score, np.float64)).to(dev)
    ws_bytes = lib.query('ds2_ctc_keyword_search_ws_bytes', n_b, n_t)
    assert ws_bytes >= 4 * n_b * n_t
    ws = torch.full((ws_bytes + PAD,), W_SENT, dtype=torch.uint8, device=dev)
    if ws_fill is not None:
        ws[:ws_bytes] = ws_fill
    hits_w, hits = _guarded((n_b, n_k, max_hits, 2), torch.int32, I_SENT, dev)
    score_w, score = _guarded((n_b, n_k, max_hits), torch.float64, F_SENT, dev)
    count_w, count = _guarded((n_b, n_k), torch.int32, I_SENT, dev)
    lib.call('ds2_ctc_keyword_search', logp_d, sizes_d, flat, offs, lens, thr, n_b, n_t, n_a, n_k, blank, max_hits,
             ws, ws_bytes, hits, score, count)
    torch.cuda.synchronize()
    assert _untouched(hits_w, I_SENT) and _untouched(score_w, F_SENT) and _untouched(count_w, I_SENT)
    assert bool((ws[ws_bytes:] == W_SENT).all())
    return hits.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()


def _assert_equal(got, want, pairs=None):
    (hits, score, count), (w_hits, w_score, w_count) = got, want
    if pairs is not None:
        sel = tuple(np.asarray(pairs).T)
        hits, score, count, w_hits, w_score, w_count = (x[sel] for x in (hits, score, count, w_hits, w_score, w_count))
    assert (count == w_count).all(), (count, w_count)
    assert (hits == w_hits).all()
    assert (score == w_score).all()                          # (-inf == -inf; no NaN on either side)


def _log_softmax(rng, shape, scale=3.0):
    x = torch.from_numpy((rng.randn(*shape) * scale).astype(np.float32))
    return torch.log_softmax(x, dim=-1).numpy()


def _main_case():
    rng = np.random.RandomState(5)
    n_t, n_a = 70, 29                                        # the staging chunk is min(32, 1024 // 29) = 32 frames
    sizes = [0, 1, 31, 32, 33, 70, 64, 99]                   # (99 is clamped to T)
    logp = _log_softmax(rng, (len(sizes), n_t, n_a))
    for b, n in enumerate(sizes):
        logp[b, n:] = np.nan                                 # padding is never read
    logp[5, 10, :] = NEG                                     # a frame with no value at all
    logp[5, 20, 7] = np.nan                                  # a NaN inside a valid frame
    logp[6, 3, 4] = NEG
    word = lambda n: [int(v) for v in rng.randint(1, n_a, size=n)]    # noqa: E731
    keywords = [[7], [4, 9], word(32), word(33), word(64), word(65), [], [5, 5], [5, 5, 6], [7, 8, 8, 7], [3, 29], [3, -1],
                [4, 0], [12, 7, 12], [9]]
    assert len(keywords) % 4 != 0
    min_score = [-3.0, -9.0, -8.0 * 32, -8.0 * 33, -8.0 * 64, -1e9, -1e9, -14.0, -21.0, -30.0, -1e9, -1e9, -1e9, np.nan,
                 NEG]
    return logp, sizes, keywords, min_score


def test_equals_the_reference_on_log_softmax_data_with_every_kind_of_keyword():
    logp, sizes, keywords, min_score = _main_case()
    want = ref.search_batch(logp, sizes, keywords, min_score, max_hits=3)
    got = _launch(logp, sizes, keywords, min_score, 3)
    _assert_equal(got, want)
    count = want[2]
    assert (count[:, [5, 6, 10, 11, 12, 13]] == 0).all()     # too long, empty, bad ids, blank, NaN threshold
    assert count.max() > 3 and (count[0] == 0).all()         # max_hits is exceeded somewhere; sizes = 0 finds nothing
    assert all(count[5:7, k].sum() > 0 for k in (0, 1, 2, 3, 7, 8, 9, 14))
    # the public wrapper makes the same call
    from ds2hip import ops
    dev = 'cuda'
    flat, offs, lens = _keyword_tensors(keywords, dev)
    out = ops.keyword_search(torch.from_numpy(logp).to(dev), torch.tensor(sizes, dtype=torch.int32, device=dev), flat, offs,
                             lens, torch.tensor(min_score, dtype=torch.float64, device=dev), max_hits=3)
    _assert_equal([x.cpu().numpy() for x in out], want)


@pytest.mark.parametrize('n_a,n_t,sizes', [(2, 40, [40, 33, 32, 31, 1]), (29, 37, [37, 36, 0]), (256, 11, [3, 4, 5, 11, 9])])
def test_equals_the_reference_on_dyadic_data_where_ties_abound(n_a, n_t, sizes):
    logp, keywords, min_score = _dyadic_case(n_a, n_t, sizes)
    want = ref.search_batch(logp, sizes, keywords, min_score, max_hits=4)
    _assert_equal(_launch(logp, sizes, keywords, min_score, 4), want)
    assert want[2].max() > 4 and (want[2].sum(axis=0) > 0).sum() >= len(keywords) - 2


def _dyadic_case(n_a, n_t, sizes):
    rng = np.random.RandomState(n_a)
    logp = (-0.25 * rng.randint(0, 6, size=(len(sizes), n_t, n_a))).astype(np.float32)
    hi = n_a - 1
    keywords = [[hi], [hi, hi], [hi] * 3, [1] * 5]
    if n_a > 2:
        keywords += [[1, 2], [2, 1, 2, 3], [hi, 1, 1, hi - 1], [1, hi, 1]]
    return logp, keywords, [-0.5 * len(k) for k in keywords]


def test_all_equal_emissions_bind_every_tie_rule():
    logp = np.full((2, 35, 5), -1.0, np.float32)
    keywords = [[1], [1, 2], [1, 1], [2, 1, 2], [3, 3, 4, 4]]
    want = ref.search_batch(logp, [35, 6], keywords, [0.0] * 5, max_hits=2)
    _assert_equal(_launch(logp, [35, 6], keywords, [0.0] * 5, 2), want)
    # every frame costs 0: one hit per keyword, from frame 0 (stay beats a fresh start) to the last frame (the plateau)
    assert want[2].tolist() == [[1] * 5] * 2
    assert want[0][0, :, 0].tolist() == [[0, 34]] * 5 and want[0][1, :, 0].tolist() == [[0, 5]] * 5


def test_a_pair_does_not_depend_on_the_batch_the_other_keywords_or_the_workspace():
    rng = np.random.RandomState(11)
    n_b, n_k, n_t, n_a = 40, 70, 40, 29
    logp = _log_softmax(rng, (n_b, n_t, n_a), 2.0)
    logp[n_b - 1] = logp[0]
    sizes = rng.randint(0, n_t + 1, size=n_b)
    sizes[0] = sizes[n_b - 1] = 37
    keywords = [[int(v) for v in rng.randint(1, n_a, size=rng.randint(1, 21))] for _ in range(n_k)]
    keywords[0] = keywords[n_k - 1] = [6, 6, 11]
    min_score = [-7.0 * len(k) for k in keywords]
    alone = _launch(logp[:1], sizes[:1], keywords[:1], min_score[:1], 4)
    assert alone[2][0, 0] > 0
    corners = [(0, 0), (0, n_k - 1), (n_b - 1, 0), (n_b - 1, n_k - 1)]
    runs = [_launch(logp, sizes, keywords, min_score, 4, ws_fill=fill) for fill in (None, 0xFF, 0)]
    for got in runs:
        for b, k in corners:
            for x, y in zip(got, alone):
                assert x[b, k].tobytes() == y[0, 0].tobytes()
        for x, y in zip(got, runs[0]):
            assert x.tobytes() == y.tobytes()                # bit-identical from run to run, whatever the workspace held
    spot = corners + [(3, 5), (17, 33), (25, 68), (39, 1), (8, 42)]
    _assert_equal(runs[0], ref.search_batch(logp, sizes, keywords, min_score, max_hits=4, pairs=spot), pairs=spot)


def test_workspace_full_of_nan_changes_nothing():
    from ds2hip import lib, ops
    rng = np.random.RandomState(2)
    dev = 'cuda'
    logp = torch.from_numpy(_log_softmax(rng, (3, 50, 29))).to(dev)
    sizes = torch.tensor([50, 17, 33], dtype=torch.int32, device=dev)
    keywords = [[3], [4, 4], [1, 2, 3]]
    flat, offs, lens = _keyword_tensors(keywords, dev)
    thr = torch.tensor([-2.0, -8.0, -12.0], dtype=torch.float64, device=dev)
    ws = torch.full((lib.query('ds2_ctc_keyword_search_ws_bytes', 3, 50) // 4,), float('nan'), device=dev)
    a = ops.keyword_search(logp, sizes, flat, offs, lens, thr, ws=ws.view(torch.uint8))
    b = ops.keyword_search(logp, sizes, flat, offs, lens, thr)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    want = ref.search_batch(logp.cpu().numpy(), [50, 17, 33], keywords, [-2.0, -8.0, -12.0], max_hits=4)
    _assert_equal([x.cpu().numpy() for x in a], want)


def test_every_argument_error_is_refused_before_any_launch():
    from ds2hip import lib
    dev = 'cuda'
    n_b, n_t, n_a, n_k, max_hits = 2, 5, 29, 3, 4
    logp = torch.zeros((n_b, n_t, 257), device=dev)
    sizes = torch.full((n_b,), n_t, dtype=torch.int32, device=dev)
    flat = torch.ones((8,), dtype=torch.int32, device=dev)
    offs = torch.zeros((n_k,), dtype=torch.int32, device=dev)
    lens = torch.ones((n_k,), dtype=torch.int32, device=dev)
    thr = torch.zeros((n_k,), dtype=torch.float64, device=dev)
    need = lib.query('ds2_ctc_keyword_search_ws_bytes', n_b, n_t)
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev)
    hits = torch.full((n_b, n_k, max_hits, 2), I_SENT, dtype=torch.int32, device=dev)
    score = torch.full((n_b, n_k, max_hits), F_SENT, dtype=torch.float64, device=dev)
    count = torch.full((n_b, n_k), I_SENT, dtype=torch.int32, device=dev)
    good = dict(logp=logp, sizes=sizes, labels=flat, offs=offs, lens=lens, thr=thr, B=n_b, T=n_t, A=n_a, K=n_k, blank=0,
                max_hits=max_hits, ws=ws, ws_bytes=need, hits=hits, score=score, count=count)

    def call(**change):
        a = dict(good, **change)
        lib.call('ds2_ctc_keyword_search', a['logp'], a['sizes'], a['labels'], a['offs'], a['lens'], a['thr'], a['B'],
                 a['T'], a['A'], a['K'], a['blank'], a['max_hits'], a['ws'], a['ws_bytes'], a['hits'], a['score'],
                 a['count'])

    bad = [dict(A=257), dict(A=0), dict(K=0), dict(K=65536), dict(max_hits=0), dict(max_hits=65), dict(blank=n_a),
           dict(blank=-1), dict(B=-1), dict(T=-1), dict(ws_bytes=need - 1), dict(ws=None)]
    bad += [{name: None} for name in ('logp', 'sizes', 'labels', 'offs', 'lens', 'thr', 'hits', 'score', 'count')]
    for change in bad:
        with pytest.raises(lib.Ds2Error) as err:
            call(**change)
        assert err.value.code == lib.ERR_ARG, change
        if 'ws' in change or 'ws_bytes' in change:
            assert str(need) in str(err.value), str(err.value)
    torch.cuda.synchronize()
    assert bool((hits == I_SENT).all()) and bool((score == F_SENT).all()) and bool((count == I_SENT).all())
    assert lib.query('ds2_ctc_keyword_search_ws_bytes', -1, 5) == 0
    call()                                                   # and the arguments they were derived from are fine
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [[1] * n_k] * n_b         # logp = 0 everywhere: every frame is free, one hit 0..T-1
    assert hits[:, :, 0].cpu().tolist() == [[[0, n_t - 1]] * n_k] * n_b
