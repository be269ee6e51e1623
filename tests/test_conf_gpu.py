"""ds2_ctc_unit_posterior (csrc/ctc_unit.hip) against its float64 statement tests/conf_ref.py.

Bounds, kernel - reference:
  * exact cases (probabilities from {1/2, 1/4, 0} and spans of at most 26 frames -- or, for the units of 31 .. 64 labels,
    which need longer spans, 1/4 at no more than 10 places so that P is a small integer times 2^-(n + 10); conf_ref asserts
    that P is a double): |logp - ln P| <= 4 * 2^-52 * max(1, |ln P|), the two logarithms' and the exponent sum's roundings;
  * everything else: |dlogp| <= 2 * (3 n + 4) * 2^-53 + 4 * 2^-52 * max(1, |logp|) for a span of n frames (conf_ref.bound:
    three roundings per frame on non-negative terms, once for the kernel and once for the reference).
Measured on an MI355X: profiles/conf_errors.md."""
import math

import numpy as np
import pytest
import torch

from tests import conf_ref as cr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
WORST = {}                                   # case name -> the worst |dlogp| / bound seen (printed; profiles/conf_errors.md)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def make_case(probs, sizes, rows, space_id, blank=0, utt=None, stride=None):
    """rows: [(labels, offsets)].  Everything as numpy, labels / offsets padded to ``stride`` with garbage."""
    stride = stride or max([len(r[0]) for r in rows] + [1]) + 2
    labels = np.full((len(rows), stride), 10 ** 6, np.int32)
    offsets = np.full((len(rows), stride), -7, np.int32)
    lens = np.zeros(len(rows), np.int32)
    for r, (lab, off) in enumerate(rows):
        labels[r, :len(lab)], offsets[r, :len(lab)], lens[r] = lab, off, len(lab)
    return dict(probs=np.asarray(probs, np.float32), sizes=np.asarray(sizes, np.int32), labels=labels, offsets=offsets,
                lens=lens, utt=None if utt is None else np.asarray(utt, np.int32), space_id=space_id, blank=blank)


def run(case, max_units=None, ws=None):
    from ds2hip import ops
    out = ops.ctc_unit_posterior(dev(case['probs']), dev(case['sizes']), dev(case['labels']), dev(case['offsets']),
                                 dev(case['lens']), None if case['utt'] is None else dev(case['utt']), case['space_id'],
                                 case['blank'], max_units, ws)
    return [x.cpu().numpy() for x in out]


def reference(case, max_units=None, exact=False):
    return cr.unit_posterior(case['probs'], case['sizes'], case['labels'], case['offsets'], case['lens'], case['utt'],
                             case['space_id'], case['blank'], max_units, exact)


def check(name, case, got, want, exact=False):
    """structure equal; values within the bound of the module's docstring.  Returns the number of finite values."""
    for g, w, what in zip(got[:2] + got[3:], want[:2] + want[3:], ('first', 'len', 'n_units', 'dropped')):
        assert np.array_equal(g, w), (name, what, g, w)
    glp, wlp = got[2], want[2]
    assert np.array_equal(np.isnan(glp), np.isnan(wlp)), name
    finite = 0
    for r, k in zip(*np.nonzero(~np.isnan(wlp))):
        g, w = float(glp[r, k]), float(wlp[r, k])
        if not math.isfinite(w):
            assert g == w, (name, r, k, g, w)
            continue
        finite += 1
        i, ln = int(want[0][r, k]), int(want[1][r, k])
        n = int(case['offsets'][r, i + ln - 1]) - int(case['offsets'][r, i]) + 1
        lim = 4.0 * 2.0 ** -52 * max(1.0, abs(w)) if exact else cr.bound(n, w)
        WORST[name] = max(WORST.get(name, 0.0), abs(g - w) / lim)
        assert abs(g - w) <= lim, (name, r, k, g, w, n)
    return finite


def dyadic(rng, shape, quarter=0.3, zero=0.15):
    return rng.choice([0.5, 0.25, 0.0], size=shape, p=[1.0 - quarter - zero, quarter, zero]).astype(np.float32)


def random_rows(rng, n_rows, n_alpha, sizes, utt, space_id, max_len, blank=0):
    """label rows with repeats, leading / trailing / double spaces, and offsets strictly increasing below the size"""
    pool = [c for c in range(n_alpha) if c != blank]
    rows = []
    for r in range(n_rows):
        lim = int(sizes[utt[r]])
        n = int(rng.randint(1, min(max_len, lim) + 1))
        lab = rng.choice(pool, n)
        if n > 2 and rng.rand() < 0.7:
            lab[rng.randint(0, n - 1)] = lab[rng.randint(0, n - 1)]
            j = rng.randint(0, n - 1)
            lab[j + 1] = lab[j]                                             # an adjacent repeat
        if space_id >= 0:
            lab[rng.rand(n) < 0.25] = space_id
        rows.append((lab.tolist(), np.sort(rng.choice(lim, n, replace=False)).tolist()))
    return rows


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('n_alpha', [2, 29, 256])
def test_exact_small_spans(n_alpha):
    rng = np.random.RandomState(n_alpha)
    probs = dyadic(rng, (3, 26, n_alpha))
    sizes = [26, 19, 7]
    utt = [0, 1, 2, 0, 1, 2, 0]
    modes = (-1,) if n_alpha == 2 else (1, -1)
    for space_id in modes:
        rows = random_rows(rng, 7, n_alpha, sizes, utt, space_id, 14)
        if space_id >= 0:
            rows[0] = ([5, 5, 1, 7, 1, 1, 9, 9, 8], [3, 4, 6, 9, 10, 11, 12, 14, 20])   # LL on two frames: impossible
            probs[0, 3:5] = 0.25
        case = make_case(probs, sizes, rows, space_id, utt=utt)
        want = reference(case, exact=True)
        got = run(case)
        assert check('exact A=%d %s' % (n_alpha, 'words' if space_id >= 0 else 'chars'), case, got, want, exact=True) >= 4
        if space_id >= 0:
            assert got[2][0, 0] == -math.inf and want[2][0, 0] == -math.inf
    print('worst |dlogp| / bound:', {k: v for k, v in WORST.items() if k.startswith('exact A=%d' % n_alpha)})


def long_unit_case(lengths, n_alpha=29, t_max=80):
    """one row per unit length L: a word of L labels without adjacent repeats (plus one row WITH repeats, which needs its
    blanks) on a span of L + 2 (+ repeats) frames; probabilities from {1/2, 0}, the unit's own diagonal and the blank at 1/2,
    and 1/4 at up to 10 places of the diagonal band: P stays an integer of a few bits times 2^-(n + 10)"""
    rng = np.random.RandomState(7)
    probs = rng.choice([0.5, 0.0], size=(len(lengths) + 1, t_max, n_alpha), p=[0.6, 0.4]).astype(np.float32)
    rows = []
    for b, ln in enumerate(list(lengths) + [33]):
        lab = [2 + (k % 5) + 5 * int(rng.randint(0, 5)) for k in range(ln)]          # neighbours differ (k % 5 does)
        repeats = 0
        if b == len(lengths):
            lab[10], lab[20] = lab[9], lab[19]
            repeats = 2
        first, n = 1, ln + 2 + repeats
        probs[b, :, 0] = 0.5
        for k, c in enumerate(lab):
            probs[b, first + k:first + k + 3 + repeats, c] = 0.5
        for k in rng.choice(ln, min(ln, 10), replace=False):
            probs[b, first + k + int(rng.randint(0, 3 + repeats)), lab[k]] = 0.25
        off = [first + k for k in range(ln - 1)] + [first + n - 1]
        rows.append((lab, off))
    return make_case(probs, [t_max] * len(rows), rows, 1)


def test_exact_long_units_and_the_label_limit():
    lengths = (1, 2, 31, 32, 33, 63, 64, 65)
    case = long_unit_case(lengths)
    want = reference(case, exact=True)
    got = run(case)
    assert check('exact long units', case, got, want, exact=True) == len(lengths)          # 65 has no value, the repeats row has
    assert want[1][:, 0].tolist() == list(lengths) + [33] and np.isfinite(want[2][:7, 0]).all()
    assert np.isnan(got[2][7, 0]) and got[0][7, 0] == 0 and got[1][7, 0] == 65              # listed, with logp = NaN
    assert got[4].tolist() == [0] * 7 + [1, 0] and got[3].tolist() == [1] * 9               # and counted
    print('worst |dlogp| / bound:', WORST['exact long units'])


# ------------------------------------------------------------------ random and peaked cases
def float_probs(rng, shape, sharp):
    logits = (rng.randn(*shape) * sharp).astype(np.float32)
    p = np.exp(logits - logits.max(-1, keepdims=True)).astype(np.float32)
    return (p / p.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize('sharp', [1.0, 6.0], ids=['random', 'peaked'])
def test_random_and_peaked_against_float64(sharp):
    rng = np.random.RandomState(int(sharp))
    probs = float_probs(rng, (2, 320, 29), sharp)
    sizes, utt = [320, 301], [0, 1, 0, 1, 0]
    rows = random_rows(rng, 5, 29, sizes, utt, 1, 60)
    rows[0] = ([3, 4, 4, 9, 2], [5, 60, 130, 200, 304])                     # one word over 300 frames
    rows[1] = ([1, 7, 8, 1, 1, 8, 8, 6, 1], [0, 2, 40, 41, 50, 100, 250, 300, 301 - 1])
    name = 'random' if sharp == 1.0 else 'peaked'
    for space_id in (1, -1):
        case = make_case(probs, sizes, rows, space_id, utt=utt)
        assert check(name, case, run(case), reference(case)) >= 5
    print('worst |dlogp| / bound:', name, WORST[name])


def test_a_span_of_2000_frames_stays_finite():
    probs = np.zeros((1, 2048, 3), np.float32)
    probs[:, :, 0] = probs[:, :, 2] = 0.5
    case = make_case(probs, [2048], [([2, 2], [10, 2009])], 1)
    got, want = run(case), reference(case)
    assert check('2000 frames', case, got, want) == 1
    assert math.isfinite(got[2][0, 0]) and -1400.0 < got[2][0, 0] < -1350.0        # about ln(2000^3 / 6) - 2000 ln 2
    print('worst |dlogp| / bound:', '2000 frames', WORST['2000 frames'], got[2][0, 0])


# ------------------------------------------------------------------ isolation
def _raw_call(case, max_units, pad=64, fill_ws=True):
    """the entry itself, with sentinels around all five outputs and a workspace of 0xFF bytes (NaN as doubles)"""
    from ds2hip import lib
    rows, stride = case['labels'].shape
    bsz, t, a = case['probs'].shape
    n = rows * max_units
    bufs = [torch.full((n + 2 * pad,), -12345, dtype=torch.int32, device=DEV) for _ in range(2)]
    bufs.append(torch.full((n + 2 * pad,), -12345.0, dtype=torch.float64, device=DEV))
    bufs += [torch.full((rows + 2 * pad,), -12345, dtype=torch.int32, device=DEV) for _ in range(2)]
    views = [b[pad:b.numel() - pad] for b in bufs]
    nbytes = lib.query('ds2_ctc_unit_posterior_ws_bytes', rows, stride, max_units)
    ws = torch.full((nbytes,), 0xFF if fill_ws else 0, dtype=torch.uint8, device=DEV)
    lib.call('ds2_ctc_unit_posterior', dev(case['probs']), dev(case['sizes']), bsz, t, a, dev(case['labels']),
             dev(case['offsets']), dev(case['lens']), None if case['utt'] is None else dev(case['utt']), rows, stride,
             case['space_id'], case['blank'], max_units, ws, nbytes, *views)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:pad] == -12345).all()) and bool((b[-pad:] == -12345).all())
    return [v.clone() for v in views]


def isolation_case(poison):
    rng = np.random.RandomState(11)
    probs = float_probs(rng, (3, 48, 29), 2.0)
    sizes, utt = [48, 30, 17], [0, 1, 2, 1]
    rows = random_rows(rng, 4, 29, sizes, utt, 1, 20)
    rows[3] = ([1, 1], [3, 4])                                              # spaces only
    case = make_case(probs, sizes, rows, 1, utt=utt, stride=24)
    first, length, _, n_units, _ = reference(case)
    used = np.zeros(probs.shape[:2], bool)
    for r in range(len(rows)):
        for k in range(int(n_units[r])):
            i, ln = int(first[r, k]), int(length[r, k])
            used[utt[r], case['offsets'][r, i]:case['offsets'][r, i + ln - 1] + 1] = True
    for b, s in enumerate(sizes):
        assert not used[b, s:].any()
    pad_labels = np.arange(24)[None, :] >= case['lens'][:, None]
    if poison:
        case['probs'][~used] = np.nan                                       # outside every span, past sizes included
        case['labels'][pad_labels], case['offsets'][pad_labels] = -(10 ** 9), 10 ** 9
    else:
        case['probs'][~used] = 0.0
        case['labels'][pad_labels] = case['offsets'][pad_labels] = 0
    return case


def test_nothing_outside_the_spans_is_read_and_nothing_outside_the_outputs_written():
    clean_case, dirty_case = isolation_case(False), isolation_case(True)
    clean = _raw_call(clean_case, 12, fill_ws=False)
    dirty = _raw_call(dirty_case, 12)
    for a, b in zip(clean, dirty):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = [x.cpu().numpy().reshape(4, -1) if x.numel() > 4 else x.cpu().numpy() for x in clean]
    assert check('isolation', clean_case, got, reference(clean_case, 12)) >= 3


# ------------------------------------------------------------------ layout
def layout_case():
    rng = np.random.RandomState(5)
    probs = float_probs(rng, (3, 40, 29), 2.0)
    sizes, utt = [40, 33, 21], [2, 0, 0, 1, 2, 1, 0]
    rows = random_rows(rng, 7, 29, sizes, utt, 1, 18)
    rows[2] = ([], [])                                                      # no labels
    rows[4] = ([1, 1, 1], [0, 5, 20])                                       # spaces only
    rows[5] = ([2, 1, 3, 1, 4, 1, 5, 1, 6], [1, 2, 3, 4, 5, 6, 7, 8, 30])  # five words
    return make_case(probs, sizes, rows, 1, utt=utt), rows, utt


def test_rows_sharing_utterances_equal_the_rows_one_per_call():
    case, rows, utt = layout_case()
    got, want = run(case), reference(case)
    assert check('layout', case, got, want) >= 5
    assert got[3][2] == 0 and got[3][4] == 0 and got[3][5] == 5
    stride = case['labels'].shape[1]
    for r in range(len(rows)):
        one = make_case(case['probs'][utt[r]:utt[r] + 1], case['sizes'][utt[r]:utt[r] + 1], [rows[r]], 1, stride=stride)
        alone = run(one)                                                    # utt = NULL: the row is utterance 0
        for a, b in zip(alone, got):
            assert np.array_equal(a[0].view(np.int32) if a.ndim > 1 else a[0:1], b[r].view(np.int32) if b.ndim > 1 else b[r:r + 1])
    chars = dict(case, space_id=-1)
    assert check('layout chars', chars, run(chars), reference(chars)) >= 10


def test_max_units_below_the_count():
    case, _, _ = layout_case()
    full = run(case)
    capped = [x.cpu().numpy() for x in _raw_call(case, 2)]                  # (the sentinels: nothing past the cap is touched)
    want = reference(case, 2)
    assert capped[3].tolist() == full[3].tolist() and capped[3][5] == 5     # the TRUE count
    for k in range(3):
        assert np.array_equal(capped[k].reshape(7, 2).view(np.int32), full[k][:, :2].copy().view(np.int32))
    assert check('capped', case, [capped[0].reshape(7, 2), capped[1].reshape(7, 2), capped[2].reshape(7, 2), capped[3],
                                  capped[4]], want) >= 4


def test_every_invalid_row_rule():
    rng = np.random.RandomState(9)
    probs = float_probs(rng, (2, 12, 5), 1.0)
    sizes = [12, 6]
    good = ([2, 3, 1, 4], [0, 2, 3, 5])
    rows = [good, good, good, ([2, 5, 1, 4], good[1]), ([2, -1, 1, 4], good[1]), ([2, 0, 1, 4], good[1]),
            (good[0], [0, 2, 2, 5]), (good[0], [0, 3, 2, 5]), (good[0], [-1, 2, 3, 5]), (good[0], [0, 2, 3, 6]),
            (good[0], [0, 2, 3, 12]), good, good, good]
    utt = [1, -1, 2, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1]
    case = make_case(probs, sizes, rows, 1, utt=utt, stride=6)
    case['lens'][12], case['lens'][13] = -1, 7
    got, want = run(case), reference(case)
    assert want[3].tolist() == [2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 2, -1, -1]
    check('invalid rows', case, got, want)
    assert (got[0][want[3] < 0] == -1).all() and np.isnan(got[2][want[3] < 0]).all() and not got[4].any()


def test_argument_refusals():
    from ds2hip import lib
    case, _, _ = layout_case()
    rows, stride = case['labels'].shape
    bsz, t, a = case['probs'].shape
    mu = 8
    outs = [torch.empty(rows * mu, dtype=d, device=DEV) for d in (torch.int32, torch.int32, torch.float64)]
    outs += [torch.empty(rows, dtype=torch.int32, device=DEV) for _ in range(2)]
    nbytes = lib.query('ds2_ctc_unit_posterior_ws_bytes', rows, stride, mu)
    assert nbytes > 0 and lib.query('ds2_ctc_unit_posterior_ws_bytes', 0, stride, mu) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = [dev(case['probs']), dev(case['sizes']), bsz, t, a, dev(case['labels']), dev(case['offsets']), dev(case['lens']),
            dev(case['utt']), rows, stride, 1, 0, mu, ws, nbytes] + outs
    lib.call('ds2_ctc_unit_posterior', *good)
    for pos, bad in ((4, 0), (4, 257), (12, -1), (12, a), (11, -2), (11, a), (11, 0), (9, 0), (10, 0), (13, 0), (2, 0),
                     (3, 0), (2, (1 << 25) // t + 1), (9, (1 << 27) // stride + 1), (13, (1 << 27) // rows + 1), (0, None),
                     (1, None), (5, None), (6, None), (7, None), (14, None), (16, None), (17, None), (18, None), (19, None),
                     (20, None), (15, nbytes - 1)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(lib.Ds2Error) as err:
            lib.call('ds2_ctc_unit_posterior', *args)
        assert err.value.code == lib.ERR_ARG and 'ds2_ctc_unit_posterior' in str(err.value), (pos, bad)
        if pos == 15:
            assert str(nbytes) in str(err.value)                            # the message names the needed size
    args = list(good)
    args[8] = None                                                          # utt may be NULL (rows > B: rows 3.. are invalid)
    lib.call('ds2_ctc_unit_posterior', *args)
    torch.cuda.synchronize()
    assert outs[3].tolist()[3:] == [-1] * (rows - 3)


def test_twenty_launches_give_equal_bits():
    case, _, _ = layout_case()
    first = _raw_call(case, 9)
    for _ in range(19):
        again = _raw_call(case, 9)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))


# ------------------------------------------------------------------ end to end
def test_on_the_searches_own_output():
    from ds2hip import ops
    rng = np.random.RandomState(21)
    probs = float_probs(rng, (3, 40, 29), 3.0)
    sizes = np.array([40, 31, 18], np.int32)
    p_d, s_d = dev(probs), dev(sizes)
    labels, offs, lens = ops.ctc_beam_search_nbest(p_d, s_d, 8, 4, space_id=1)[:3]
    utt = torch.arange(12, dtype=torch.int32, device=DEV) // 4
    got = ops.ctc_unit_posterior(p_d, s_d, labels.view(12, 40), offs.view(12, 40), lens.view(12), utt.int(), space_id=1)
    case = dict(probs=probs, sizes=sizes, labels=labels.view(12, 40).cpu().numpy(), offsets=offs.view(12, 40).cpu().numpy(),
                lens=lens.view(12).cpu().numpy(), utt=utt.cpu().numpy(), space_id=1, blank=0)
    assert check('n-best rows', case, [x.cpu().numpy() for x in got], reference(case)) >= 12
    best = ops.argmax_rows(p_d.view(120, 29), 120, 29).view(3, 40)
    ids, goffs, glens = ops.greedy_collapse(best, s_d, 0)
    for space_id in (1, -1):
        got = ops.ctc_unit_posterior(p_d, s_d, ids, goffs, glens, space_id=space_id)
        case = dict(probs=probs, sizes=sizes, labels=ids.cpu().numpy(), offsets=goffs.cpu().numpy(), lens=glens.cpu().numpy(),
                    utt=None, space_id=space_id, blank=0)
        assert check('greedy rows', case, [x.cpu().numpy() for x in got], reference(case)) >= 3
    print('worst |dlogp| / bound:', {k: WORST[k] for k in ('n-best rows', 'greedy rows')})


# ------------------------------------------------------------------ decoders
ALPHABET = ['_', ' '] + list('abcdefghijklmnopqrstuvwxyz') + ["'"]


def _decoders(kind, **kw):
    from codes.decoder import DeviceBeamCTCDecoder, GreedyDecoder
    if kind == 'greedy':
        return GreedyDecoder(ALPHABET, **kw)
    return DeviceBeamCTCDecoder(ALPHABET, beam_width=8, nbest=3 if kind == 'nbest' else 1, **kw)


@pytest.mark.parametrize('kind', ['greedy', 'beam', 'nbest'])
def test_decoders_with_and_without_confidence(kind, monkeypatch):
    from codes.confidence import UnitConfidence
    from ds2hip import lib
    rng = np.random.RandomState(31)
    probs = dev(float_probs(rng, (3, 40, 29), 3.0))
    sizes = torch.tensor([40, 31, 18], dtype=torch.int32)
    real, names = lib.call, []

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', call)
    seqs, results = [], []
    for kw in ({}, {'confidence': None}, {'confidence': UnitConfidence(ALPHABET)}):
        del names[:]
        dec = _decoders(kind, **kw)
        strings, offsets = dec.decode(probs, sizes)
        seqs.append(list(names))
        results.append((strings, [[o.tolist() for o in row] for row in offsets], getattr(dec, 'last_scores', None),
                        getattr(dec, 'last_nbest_scores', None)))
        if kw.get('confidence') is None:
            assert dec.confidence is None and dec.last_confidences is None
    assert seqs[0] == seqs[1] and 'ds2_ctc_unit_posterior' not in seqs[0]
    assert seqs[2].count('ds2_ctc_unit_posterior') == 1
    assert [n for n in seqs[2] if n != 'ds2_ctc_unit_posterior'] == seqs[0]
    assert results[0] == results[1] == results[2]                           # strings, offsets and scores are unchanged
    conf = dec.last_confidences
    assert len(conf) == len(strings)
    seen = 0
    for b, row in enumerate(strings):
        assert len(conf[b]) == len(row)
        for n, text in enumerate(row):
            assert len(conf[b][n]) == len(text.split())
            assert all(c is not None and 0.0 <= c <= 1.0 + 1e-5 for c in conf[b][n])     # (fp32 rows sum to 1 +- 1e-7)
            seen += len(conf[b][n])
    assert seen >= 3
