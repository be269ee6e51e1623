"""Inputs, references and bounds shared by tests/test_ctc_fp64_gpu.py (the CTC kernels against float64) and
tests/test_ctc_ref_cpu.py (the float64 reference itself, and the proof that the bounds discriminate).  No GPU in here.

A case is a dict: acts (T,B,A) float32, labels (flat int32), label_lens, act_lens, plus name / regime.  Everything is
seeded; nothing depends on a kernel's output.
"""
import math
import zlib

import numpy as np

from oracle import ctc as octc

REGIMES = ('random', 'blank', 'peaked', 'flat', 'wide')
T_TRAIN = 746

# ------------------------------------------------------------------------------------------------ bounds
# Conditions, fixed by the project before anything was measured: the gradient tolerance of tests/test_kernels_gpu.py at
# T = 746 and the README's parity contract on the loss.  Every case has to meet them.
COND_GRAD_MAX = 5e-5            # max |grad - ref| / grad_scale
COND_COST_REL = 1e-4            # |cost - ref| <= COND_COST_REL * |ref| per utterance

# Measured bounds: twice the worst figure of the family over one run of the whole file on an MI355X, rounded up to a power
# of two (profiles/ctc_fp64_errors.md has every row and the derivation).  kernel - float64, never kernel - kernel.
#   cost_per_frame: max over utterances of |cost - ref| / tl        grad_max, grad_rms: of (grad - ref) / grad_scale
# `wide` (activations x 15, costs of 1e4 .. 1e5) is a family of its own: the kernel returns the cost as float32, whose
# spacing at 6e4 is 4e-3, and a - lse is formed in float32 at |a| ~ 100.
BOUNDS = {
    'main': {'cost_per_frame': 2.0 ** -20, 'grad_max': 2.0 ** -17, 'grad_rms': 2.0 ** -21},     # worst 4.3e-7, 2.1e-6, 1.3e-7
    'wide': {'cost_per_frame': 2.0 ** -17, 'grad_max': 2.0 ** -16, 'grad_rms': 2.0 ** -21},     # worst 3.1e-6, 6.7e-6, 2.1e-7
}


def family(regime):
    return 'wide' if regime == 'wide' else 'main'


# ------------------------------------------------------------------------------------------------ inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_labels(rng, nalpha, length, top=False):
    """``length`` labels in 1 .. A-1, each with probability ~0.15 a copy of its left neighbour, with one run of three
    where there is room; ``top`` puts symbol A - 1 in."""
    lab = rng.integers(1, nalpha, size=length).astype(np.int32)
    for i in range(1, length):
        if rng.random() < 0.15:
            lab[i] = lab[i - 1]
    if length >= 3:
        i = int(rng.integers(0, length - 2))
        lab[i + 1] = lab[i + 2] = lab[i]
    if top and length:
        lab[int(rng.integers(0, length))] = nalpha - 1
    return lab


def repeats(lab):
    return int(np.sum(np.asarray(lab[1:]) == np.asarray(lab[:-1]))) if len(lab) > 1 else 0


def random_alignment(rng, lab, tl):
    """One alignment (tl symbols, blank 0) that collapses to ``lab``, or None when there is none.  Every extended state
    gets its mandatory frame (labels, and the blank between equal neighbours); the rest are spread at random."""
    n = len(lab)
    ext = np.zeros(2 * n + 1, dtype=np.int64)
    ext[1::2] = lab
    need = np.zeros(2 * n + 1, dtype=np.int64)
    need[1::2] = 1
    for i in range(1, n):
        if lab[i] == lab[i - 1]:
            need[2 * i] = 1
    extra = tl - int(need.sum())
    if extra < 0:
        return None
    dur = need + rng.multinomial(extra, np.full(2 * n + 1, 1.0 / (2 * n + 1)))
    return np.repeat(ext, dur)


def make_acts(rng, regime, t_max, nalpha, labels_per_utt, act_lens):
    bsz = len(act_lens)
    if regime == 'flat':
        return np.zeros((t_max, bsz, nalpha), dtype=np.float32)
    a = rng.standard_normal((t_max, bsz, nalpha))
    if regime == 'random':
        a *= 2.0
    elif regime == 'wide':
        a *= 30.0
    elif regime == 'blank':
        a[:, :, 0] += 8.0
    elif regime == 'peaked':
        for b in range(bsz):
            tl = min(int(act_lens[b]), t_max)
            path = random_alignment(rng, labels_per_utt[b], tl)
            if path is None:
                continue
            a[np.arange(tl), b, path] += 18.0
            wrong_t = np.nonzero(rng.random(tl) < 0.03)[0]
            for t in wrong_t:
                k = int(rng.integers(0, nalpha - 1))
                k += k >= path[t]                       # any symbol but the alignment's
                a[t, b, k] += 25.0
    else:
        raise ValueError(regime)
    return a.astype(np.float32)


def make_case(name, regime, t_max, nalpha, label_lens, act_lens, top=False, labels=None):
    rng = _rng(name, regime, t_max, nalpha, tuple(label_lens), tuple(act_lens))
    if labels is None:
        labels = [make_labels(rng, nalpha, int(n), top=top) for n in label_lens]
    labels = [np.asarray(x, dtype=np.int32) for x in labels]
    assert all(len(x) == n for x, n in zip(labels, label_lens))
    assert all(0 < int(v) < nalpha for x in labels for v in x)
    acts = make_acts(rng, regime, t_max, nalpha, labels, act_lens)
    flat = np.concatenate(labels).astype(np.int32) if sum(label_lens) else np.zeros(0, np.int32)
    return {'name': name, 'regime': regime, 'acts': acts, 'labels': flat, 'labels_per_utt': labels,
            'label_lens': np.asarray(label_lens, np.int32), 'act_lens': np.asarray(act_lens, np.int32)}


def training_lengths(bsz, t_max=T_TRAIN):
    """Mixed lengths of one training batch: full-length and short clips, L from 0 to 300, always an utterance with L = 300
    at full length, one with L = 0 and one shorter than T / 4.  Every transcript is feasible (L <= tl / 2.4: ~15 % of the
    labels repeat their neighbour)."""
    rng = _rng('lengths', bsz, t_max)
    act = [t_max, t_max, 150]
    lab = [300, 0, 40]
    while len(act) < bsz:
        kind = len(act) % 3
        tl = t_max if kind == 0 else int(rng.integers(t_max // 2, t_max)) if kind == 1 else int(rng.integers(20, t_max // 4))
        act.append(tl)
        lab.append(int(rng.integers(0, min(300, int(tl / 2.4)) + 1)))
    return lab[:bsz], act[:bsz]


MATRIX = [(bsz, nalpha, regime) for bsz in (10, 32, 64) for nalpha in (29, 43) for regime in REGIMES]


def matrix_case(bsz, nalpha, regime):
    lab, act = training_lengths(bsz)
    return make_case('train B=%d A=%d' % (bsz, nalpha), regime, T_TRAIN, nalpha, lab, act)


# ------------------------------------------------------------------------------------------------ references
_refs = {}


def reference(case):
    """(costs (B,), grad (T,B,A)) in float64 by oracle.ctc.ctc_loss_and_grad_fast, once per case.  For regime `flat` the
    costs are the closed form (no floating-point recursion at all)."""
    key = (case['name'], case['regime'], case['acts'].shape, tuple(case['label_lens']), tuple(case['act_lens']))
    if key not in _refs:
        tl = np.minimum(case['act_lens'], case['acts'].shape[0])         # an act_len beyond T means T
        costs, grad = octc.ctc_loss_and_grad_fast(case['acts'], case['labels'], tl, case['label_lens'])
        if case['regime'] == 'flat':
            closed = flat_costs(case)
            assert np.allclose(costs, closed, rtol=1e-12, atol=1e-9), (costs, closed)
            costs = closed
        _refs[key] = (costs, grad)
    return _refs[key]


def count_alignments(lab, tl):
    """The number of length-``tl`` alignments of ``lab``, by the alpha recursion over Python integers."""
    n = len(lab)
    s_len = 2 * n + 1
    ext = np.zeros(s_len, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(s_len, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    if tl <= 0:
        return 1 if n == 0 else 0
    cnt = np.array([0] * s_len, dtype=object)
    cnt[:2] = 1
    for _ in range(1, tl):
        new = cnt.copy()
        new[1:] += cnt[:-1]
        new[2:] += np.where(skip[2:], cnt[:-2], 0)
        cnt = new
    return int(cnt[-2:].sum())


def flat_costs(case):
    """All activations equal: every log-probability is -ln A, so cost = tl ln A - ln N with N alignments."""
    t_max, _, nalpha = case['acts'].shape
    out = []
    for lab, tl in zip(case['labels_per_utt'], case['act_lens']):
        tl = min(int(tl), t_max)
        n = count_alignments(lab, tl)
        out.append(tl * math.log(nalpha) - math.log(n) if n else np.inf)
    return np.asarray(out, dtype=np.float64)


def single_path(case):
    """Closed form for utterances with exactly one alignment (tl = L + repeats, or L = 0): cost = -sum of log p along the
    path, gradient = softmax - one-hot(path).  Returns (costs, grad) in float64."""
    acts = case['acts'].astype(np.float64)
    m = acts.max(-1, keepdims=True)
    logp = acts - m - np.log(np.exp(acts - m).sum(-1, keepdims=True))
    grad = np.zeros_like(acts)
    costs = np.zeros(acts.shape[1])
    for b, (lab, tl) in enumerate(zip(case['labels_per_utt'], case['act_lens'])):
        tl = int(tl)
        assert len(lab) == 0 or tl == len(lab) + repeats(lab)
        path = random_alignment(np.random.default_rng(0), lab, tl)
        costs[b] = -logp[np.arange(tl), b, path].sum()
        grad[:tl, b] = np.exp(logp[:tl, b])
        grad[np.arange(tl), b, path] -= 1.0
    return costs, grad


# ------------------------------------------------------------------------------------------------ error figures
def errors(case, costs, grad, ref_costs, ref_grad, grad_scale=1.0):
    """kernel - float64: {'cost_abs', 'cost_rel', 'cost_per_frame'} as the worst utterance, {'grad_max', 'grad_rms'} over
    the valid frames, divided by grad_scale.  A cost that is infinite on both sides counts as exact; on one side only, or
    NaN, as infinitely wrong."""
    costs = np.asarray(costs, np.float64)
    t_max = case['acts'].shape[0]
    tl = np.minimum(case['act_lens'].astype(np.int64), t_max)
    same_inf = np.isinf(ref_costs) & (costs == ref_costs)
    with np.errstate(invalid='ignore'):
        e = np.where(same_inf, 0.0, np.abs(costs - ref_costs))
    e = np.where(np.isnan(e), np.inf, e)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(e == 0, 0.0, e / np.abs(ref_costs))
    valid = np.arange(t_max)[:, None] < tl[None, :]
    d = (np.asarray(grad, np.float64) - ref_grad * grad_scale) / grad_scale
    d = np.where(np.isnan(d), np.inf, d)
    dv = d[valid]
    return {'cost_abs': float(e.max()), 'cost_rel': float(rel.max()), 'cost_per_frame': float((e / np.maximum(tl, 1)).max()),
            'grad_max': float(np.abs(d).max()), 'grad_rms': float(np.sqrt(np.mean(dv * dv))) if dv.size else 0.0}


def violations(err, regime):
    """What a result misses: the conditions, and the measured bounds of its family."""
    bad = []
    if not err['grad_max'] <= COND_GRAD_MAX:
        bad.append('condition: grad max %.3e > %.1e' % (err['grad_max'], COND_GRAD_MAX))
    if not err['cost_rel'] <= COND_COST_REL:
        bad.append('condition: cost rel %.3e > %.1e' % (err['cost_rel'], COND_COST_REL))
    for name, bound in BOUNDS[family(regime)].items():
        if bound is not None and not err[name] <= bound:
            bad.append('%s %.3e > %.3e (%s family)' % (name, err[name], bound, family(regime)))
    return bad
