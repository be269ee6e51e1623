"""The float64 CTC reference that tests/test_ctc_fp64_gpu.py holds the kernels to, tied to everything else that states the
same loss (CPU only), and the proof that the bounds of tests/ctc_cases.py can tell a wrong kernel from a right one:
torch's ctc_loss in float32 -- log-space alpha / beta carried in fp32, what csrc/ctc.hip's header says it must not be --
and two wrong recursions must land outside them.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ctc as octc
from tests import ctc_cases as cc


def _torch_ctc(case, dtype):
    """(costs (B,), grad (T,B,A)) of F.ctc_loss on log_softmax(acts) in ``dtype`` on the CPU."""
    a = torch.as_tensor(case['acts']).to(dtype).requires_grad_(True)
    costs = F.ctc_loss(a.log_softmax(-1), torch.as_tensor(case['labels'], dtype=torch.long),
                       torch.as_tensor(case['act_lens'], dtype=torch.long), torch.as_tensor(case['label_lens'], dtype=torch.long),
                       blank=0, reduction='none', zero_infinity=False)
    costs.sum().backward()
    return costs.detach().double().numpy(), a.grad.double().numpy()


RAGGED = [
    # name, T, A, label_lens, act_lens, labels (None = seeded with repeats)
    ('ragged', 40, 7, [5, 0, 9, 1, 3], [40, 17, 33, 1, 9], None),
    ('empty, tl = 0, tl = 1', 12, 5, [0, 0, 1, 0, 2], [12, 0, 1, 1, 0], None),
    ('infeasible', 10, 5, [3, 4, 6, 2], [3, 7, 5, 2], [[1, 2, 2], [3, 3, 3, 3], [1, 2, 3, 4, 1, 2], [4, 4]]),
    ('runs', 30, 4, [8, 12, 3], [30, 29, 5], [[1] * 8, [2, 2, 2, 1, 1, 3, 3, 3, 3, 1, 2, 2], [3, 3, 3]]),
]


@pytest.mark.parametrize('name,t_max,nalpha,label_lens,act_lens,labels', RAGGED, ids=[r[0] for r in RAGGED])
@pytest.mark.parametrize('regime', ['random', 'peaked'])
def test_fast_reference_is_the_loop_oracle(name, t_max, nalpha, label_lens, act_lens, labels, regime):
    case = cc.make_case(name, regime, t_max, nalpha, label_lens, act_lens, labels=labels)
    c0, g0 = octc.ctc_loss_and_grad(case['acts'], case['labels'], case['act_lens'], case['label_lens'])
    c1, g1 = octc.ctc_loss_and_grad_fast(case['acts'], case['labels'], case['act_lens'], case['label_lens'])
    assert np.array_equal(np.isinf(c0), np.isinf(c1)) and not np.isnan(c1).any()
    if name == 'infeasible':
        assert list(np.isinf(c1)) == [True, False, True, True]
    fin = np.isfinite(c0)
    assert np.abs(c0[fin] - c1[fin]).max(initial=0.0) <= 1e-12
    assert np.abs(g0 - g1).max() <= 1e-12
    assert np.all(g1[:, ~fin] == 0)
    for b, tl in enumerate(act_lens):
        assert np.all(g1[tl:, b] == 0)


def test_fast_reference_is_brute_force_on_tiny_cases():
    rng = np.random.default_rng(21)
    for t_len, label in ((3, [1]), (4, [1, 2]), (4, [2, 2]), (4, [1, 1]), (3, [1, 1]), (2, []), (5, [3, 3]), (5, [1, 2, 1]), (1, [2])):
        acts = 2 * rng.standard_normal((t_len, 1, 4))
        costs, _ = octc.ctc_loss_and_grad_fast(acts, label, [t_len], [len(label)])
        bf = octc.ctc_brute_force(acts[:, 0], label)
        if np.isinf(bf):
            assert np.isinf(costs[0]) and costs[0] > 0
        else:
            assert abs(costs[0] - bf) < 1e-12, (t_len, label)


@pytest.mark.parametrize('regime', ['random', 'blank', 'peaked', 'wide'])
def test_fast_reference_is_torch_float64_at_training_length(regime):
    case = cc.make_case('torch64', regime, 746, 29, [300, 0, 40, 511, 1], [746, 700, 150, 746, 746])
    c, g = octc.ctc_loss_and_grad_fast(case['acts'], case['labels'], case['act_lens'], case['label_lens'])
    ct, gt = _torch_ctc(case, torch.float64)
    print('CTCREF|%s|cost %.3e|grad %.3e' % (regime, np.abs(c - ct).max(), np.abs(g - gt).max()))
    assert np.abs(c - ct).max() <= 1e-10 * max(1.0, np.abs(ct).max())           # 1e5 * eps per unit of cost
    assert np.abs(g - gt).max() <= 1e-10


@pytest.mark.parametrize('nalpha,label_lens,act_lens', [(29, [300, 0, 40, 7, 3], [746, 746, 150, 20, 3]), (2, [4, 1], [9, 30]),
                                                        (256, [20, 0], [60, 5])])
def test_flat_closed_form(nalpha, label_lens, act_lens):
    """All-equal activations: cost = tl ln A - ln N, N counted in integers; the gradient sums to zero over every frame."""
    case = cc.make_case('flat pin', 'flat', max(act_lens), nalpha, label_lens, act_lens)
    c, g = octc.ctc_loss_and_grad_fast(case['acts'], case['labels'], case['act_lens'], case['label_lens'])
    closed = cc.flat_costs(case)
    fin = np.isfinite(closed)                   # (the three-label utterance is a run of three in three frames: N = 0)
    assert np.array_equal(np.isposinf(c), ~fin) and fin.sum() >= len(fin) - 1
    assert np.abs(c[fin] - closed[fin]).max() <= 1e-12 * np.abs(closed[fin]).max() + 1e-12
    assert np.abs(g.sum(-1)).max() <= 1e-9          # the posteriors sum to one: up to 746 additions at |alpha| ~ 2500, 5.6e-13 each
    # the count itself, against enumeration
    assert cc.count_alignments([1, 1], 4) == 5 and cc.count_alignments([1, 2], 3) == 5 and cc.count_alignments([], 7) == 1
    assert cc.count_alignments([1, 1], 2) == 0 and cc.count_alignments([1], 0) == 0 and cc.count_alignments([], 0) == 1
    for lab, tl in (([1, 2], 4), ([2, 2], 5), ([1], 3)):
        bf = octc.ctc_brute_force(np.zeros((tl, 3)), lab)
        assert abs(bf - (tl * math.log(3) - math.log(cc.count_alignments(lab, tl)))) < 1e-12


def single_path_case(regime='random', nalpha=29):
    labels = [[3, 3, 3, 5, 5, 1], [], [7], [2, 4, 6, 8, 8]]
    return cc.make_case('single path', regime, 12, nalpha, [6, 0, 1, 5], [9, 12, 1, 6], labels=labels)


@pytest.mark.parametrize('regime', ['random', 'peaked', 'wide'])
def test_single_path_closed_form(regime):
    case = single_path_case(regime)
    c, g = octc.ctc_loss_and_grad_fast(case['acts'], case['labels'], case['act_lens'], case['label_lens'])
    cs, gs = cc.single_path(case)
    assert np.abs(c - cs).max() <= 1e-12 * max(1.0, np.abs(cs).max())
    assert np.abs(g - gs).max() <= 1e-12


# ------------------------------------------------------------------------------------- the bounds discriminate
def _bounds_fixed():
    return all(v is not None for fam in cc.BOUNDS.values() for v in fam.values())


@pytest.mark.parametrize('bsz,nalpha,regime', cc.MATRIX, ids=['B%d-A%d-%s' % m for m in cc.MATRIX])
def test_float32_log_space_ctc_misses_the_bounds(bsz, nalpha, regime):
    """F.ctc_loss in float32 on the CPU (alpha / beta in fp32 log space) against float64 on every case of the training-size
    matrix: it must land outside the fixed bounds of the case's family -- asserted on the gradient, whose fp32 error
    (2e-4 .. 6e-2) is 25 x .. 3800 x the bound in every one of the 30 cases, so a kernel that carried the recursion in fp32
    fails the GPU file on every matrix case.

    The COST bound separates it in the random (2.7e-6 .. 5.4e-6 per frame against 9.5e-7), flat (1.1e-5 .. 2.6e-5) and wide
    (1.9e-5 .. 4.2e-5 against 7.6e-6) regimes, which is asserted; not in blank (2.5e-7 .. 1.3e-6) and peaked
    (6.9e-7 .. 1.0e-6).  That is a finding about the kernel's interface, not a bound to be tightened: the cost is returned
    as float32, whose rounding alone is up to 3.3e-7 per frame (half a unit in the last place of a cost of 2500 is 1.2e-4),
    the size of the fp32 recursion's own cost error in those two regimes."""
    assert _bounds_fixed()
    case = cc.matrix_case(bsz, nalpha, regime)
    c64, g64 = _torch_ctc(case, torch.float64)
    c32, g32 = _torch_ctc(case, torch.float32)
    err = cc.errors(case, c32, g32, c64, g64)
    b = cc.BOUNDS[cc.family(regime)]
    print('CTCF32|B=%d A=%d|%s|%.3e|%.3e|%.3e|%.3e|%.3e' % (bsz, nalpha, regime, err['cost_abs'], err['cost_per_frame'],
                                                         b['cost_per_frame'], err['grad_max'], b['grad_max']))
    assert cc.violations(err, regime)
    assert err['grad_max'] > 10 * b['grad_max']
    if regime in ('random', 'flat', 'wide'):
        assert err['cost_per_frame'] > b['cost_per_frame']


def _forward_costs(case, skip_equal=False, last_only=False):
    """Costs by the float64 alpha recursion alone, with two switchable MISTAKES: ``skip_equal`` allows the s-2 -> s
    transition between equal labels, ``last_only`` takes the total from the last state alone.  With neither it is the loss."""
    acts = case['acts'].astype(np.float64)
    logp = octc._log_softmax(acts)
    out = []
    for b, (lab, tl) in enumerate(zip(case['labels_per_utt'], case['act_lens'])):
        tl = int(tl)
        s_len = 2 * len(lab) + 1
        ext = np.zeros(s_len, dtype=np.int64)
        ext[1::2] = lab
        skip = np.zeros(s_len, dtype=bool)
        skip[2:] = (ext[2:] != 0) & ((ext[2:] != ext[:-2]) | skip_equal)
        em = logp[:tl, b][:, ext]
        alpha = np.full(s_len, -np.inf)
        alpha[:2] = em[0, :2]
        stack = np.full((3, s_len), -np.inf)
        for t in range(1, tl):
            stack[0] = alpha
            stack[1, 1:] = alpha[:-1]
            stack[2, 2:] = np.where(skip[2:], alpha[:-2], -np.inf)
            alpha = octc._lse_rows(stack) + em[t]
        tail = alpha[-1:] if last_only else alpha[-2:]
        out.append(-float(octc._lse_rows(tail.reshape(-1, 1))[0]))
    return np.asarray(out)


@pytest.mark.parametrize('mutant', ['skip_equal', 'last_only'])
def test_wrong_recursions_miss_the_bounds_tenfold(mutant):
    """Two classic CTC mistakes, made in a copy of the reference: each must miss the cost bound by >= 10 x on at least one
    training-size matrix case (and the unmutated copy must be the reference)."""
    assert _bounds_fixed()
    worst = 0.0
    for nalpha in (29, 43):
        for regime in ('random', 'peaked', 'blank'):
            case = cc.matrix_case(10, nalpha, regime)
            ref, _ = cc.reference(case)
            assert np.abs(_forward_costs(case) - ref).max() <= 1e-9
            got = _forward_costs(case, **{mutant: True})
            tl = case['act_lens'].astype(np.float64)
            ratio = float((np.abs(got - ref) / tl).max() / cc.BOUNDS['main']['cost_per_frame'])
            print('CTCMUT|%s|A=%d|%s|%.3e' % (mutant, nalpha, regime, ratio))
            worst = max(worst, ratio)
    assert worst >= 10.0
