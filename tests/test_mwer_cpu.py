"""tests/mwer_ref.py, the float64 statement of ds2_ctc_mwer_grad, held to what already exists (torch autograd over
F.ctc_loss in double, oracle.ctc.ctc_brute_force) and to the rules of include/ds2hip.h "MWER"; the C surface of the two new
symbols; the ``training.mwer`` block's refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ctc as octc
from tests import mwer_cases as mc
from tests import mwer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_mwer(acts, act_lens, hyps, risks, refs, ctc_weight):
    """loss (B,) and d(sum loss)/d acts by autograd over F.ctc_loss in float64."""
    a = torch.tensor(np.asarray(acts, dtype=np.float64), requires_grad=True)
    losses = []
    for b in range(a.shape[1]):
        tl = int(act_lens[b])
        logp = a[:tl, b:b + 1].log_softmax(-1)

        def cost(lab):
            lab = torch.as_tensor(np.asarray(lab, dtype=np.int64)).reshape(1, -1)
            return F.ctc_loss(logp, lab, torch.tensor([tl]), torch.tensor([lab.shape[1]]), blank=0, reduction='sum',
                              zero_infinity=False)
        c = torch.stack([cost(h) for h in hyps[b]])
        post = torch.softmax(-c, 0)
        exp_risk = (post * torch.tensor(np.asarray(risks[b], dtype=np.float64))).sum()
        losses.append(exp_risk + ctc_weight * cost(refs[b]))
    total = torch.stack(losses)
    total.sum().backward()
    return total.detach().numpy(), a.grad.numpy()


def _small_case():
    rng = np.random.default_rng(5)
    acts = rng.standard_normal((12, 2, 5)) * 1.5
    refs = [np.array([1, 2, 2, 4]), np.array([3, 1])]
    hyps = [[np.array([1, 2, 2, 4]), np.array([1, 2, 4]), np.array([1, 3, 2, 4, 4]), np.array([2, 2])],
            [np.array([3, 1]), np.array([3]), np.zeros(0, np.int64)]]
    risks = [[0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0]]
    return acts, np.array([12, 9]), hyps, risks, refs


def test_reference_equals_torch_autograd_in_double():
    acts, act_lens, hyps, risks, refs = _small_case()
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3)
    loss, grad = _torch_mwer(acts, act_lens, hyps, risks, refs, 0.3)
    assert np.abs(res['loss'] - loss).max() <= 1e-12 * max(1.0, np.abs(loss).max())
    assert np.abs(res['grad'] - grad).max() <= 1e-12
    assert np.all(res['grad'][9:, 1] == 0.0)
    # grad_scale multiplies, nothing else
    res2 = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3, grad_scale=0.25)
    assert np.abs(res2['grad'] - 0.25 * grad).max() <= 1e-12


def test_reference_costs_equal_brute_force():
    rng = np.random.default_rng(11)
    acts = rng.standard_normal((4, 1, 3))
    hyps = [[np.array([1]), np.array([1, 2]), np.array([2, 2]), np.zeros(0, np.int64)]]
    risks = [[1.0, 0.0, 2.0, 2.0]]
    refs = [np.array([1, 2])]
    res = mwer_ref.mwer(acts, [4], hyps, risks, refs, ctc_weight=0.5)
    brute = np.array([octc.ctc_brute_force(acts[:, 0], list(h)) for h in hyps[0]])
    assert np.abs(res['hyp_costs'][0] - brute).max() <= 1e-12
    assert abs(res['ref_costs'][0] - brute[1]) <= 1e-12
    p = np.exp(-brute) / np.exp(-brute).sum()
    assert np.abs(res['posterior'][0] - p).max() <= 1e-12
    assert abs(res['exp_risk'][0] - float(p @ np.array(risks[0]))) <= 1e-12
    assert abs(res['loss'][0] - (float(p @ np.array(risks[0])) + 0.5 * brute[1])) <= 1e-12


def test_one_hypothesis_or_equal_risks_leave_only_the_ctc_term():
    acts, act_lens, hyps, risks, refs = _small_case()
    ctc_only = mwer_ref.mwer(acts, act_lens, [[], []], [[], []], refs, ctc_weight=0.3)
    one = mwer_ref.mwer(acts, act_lens, [h[:1] for h in hyps], [[7.0], [2.0]], refs, ctc_weight=0.3)
    assert np.abs(one['grad'] - ctc_only['grad']).max() <= 1e-15
    assert np.allclose(one['exp_risk'], [7.0, 2.0], rtol=0, atol=1e-15)
    same = mwer_ref.mwer(acts, act_lens, hyps, [[3.0] * 4, [5.0] * 3], refs, ctc_weight=0.3)
    assert np.abs(same['grad'] - ctc_only['grad']).max() <= 1e-14
    assert np.all(ctc_only['exp_risk'] == 0.0)                            # no finite row: E = 0


def test_a_constant_added_to_the_risks_changes_nothing():
    acts, act_lens, hyps, risks, refs = _small_case()
    base = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3)
    moved = mwer_ref.mwer(acts, act_lens, hyps, [[w + 17.0 for w in r] for r in risks], refs, ctc_weight=0.3)
    assert np.abs(base['grad'] - moved['grad']).max() <= 1e-12
    assert np.abs(moved['exp_risk'] - base['exp_risk'] - 17.0).max() <= 1e-12


def test_infeasible_rows_dropped_rows_and_infeasible_references():
    acts, act_lens, hyps, risks, refs = _small_case()
    long_row = np.array([1, 1, 1, 1, 1, 1])                               # needs 11 frames; utterance 1 has 9
    hyps = [hyps[0], hyps[1] + [long_row]]
    risks = [risks[0], risks[1] + [1e6]]
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3)
    assert np.isinf(res['hyp_costs'][1][3]) and res['posterior'][1][3] == 0.0 and res['weights'][1][3] == 0.0
    without = mwer_ref.mwer(acts, act_lens, [hyps[0], hyps[1][:3]], [risks[0], risks[1][:3]], refs, ctc_weight=0.3)
    assert np.array_equal(res['grad'], without['grad']) and np.array_equal(res['exp_risk'], without['exp_risk'])
    # dropped: longer than max_label_len -- the same as infeasible, and counted
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3, max_label_len=4)
    assert list(res['dropped']) == [1, 1] and res['posterior'][0][2] == 0.0
    # an infeasible reference: no gradient from that utterance, the other one untouched; zero_batch_if_inf: none at all
    bad_refs = [refs[0], long_row]
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, bad_refs, ctc_weight=0.3)
    assert np.isinf(res['ref_costs'][1]) and np.all(res['grad'][:, 1] == 0.0) and np.any(res['grad'][:, 0] != 0.0)
    assert np.isfinite(res['exp_risk'][1])
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, bad_refs, ctc_weight=0.3, zero_batch_if_inf=True)
    assert np.all(res['grad'] == 0.0)


def test_descent_case_has_distinct_risks_and_the_reference_gradient_descends():
    case = mc.descent_case()
    assert all(len(set(r)) >= 2 for r in case['risks'])
    res = mwer_ref.mwer(case['acts'], case['act_lens'], case['hyps'], case['risks'], case['refs'], ctc_weight=0.0)
    assert all(np.isfinite(c).sum() >= 2 for c in res['hyp_costs'])
    after = mwer_ref.expected_risk(case['acts'].astype(np.float64) - mc.DESCENT_LR * res['grad'], case['act_lens'],
                                   case['hyps'], case['risks'])
    assert np.all(after < res['exp_risk']), (after, res['exp_risk'])


def test_grad_condition_is_the_issues_formula():
    acts, act_lens, hyps, risks, refs = _small_case()
    res = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.3)
    from tests import ctc_cases as cc
    fam = cc.BOUNDS['main']
    p, e = res['posterior'][0], res['exp_risk'][0]
    s_w = 0.3 + float(np.sum(p * np.abs(np.array(risks[0]) - e)))
    want = s_w * 2.0 ** -17 + 2.0 * 3.0 * (2.0 * 2.0 ** -20 * 12)
    assert abs(mwer_ref.grad_condition(res, 0, risks[0], 0.3, 12, fam) - want) <= 1e-18


def test_the_symbols_are_declared_and_bound_and_the_revision_stays_404():
    from ds2hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404 == lib.ABI_VERSION
    assert re.search(r'size_t\s+ds2_ctc_mwer_ws_bytes\(', hdr) and re.search(r'int\s+ds2_ctc_mwer_grad\(', hdr)
    assert int(re.search(r'#define\s+DS2_MWER_MAX_NBEST\s+(\d+)', hdr).group(1)) == lib.MWER_MAX_NBEST == 128
    assert len(lib.SIGNATURES['ds2_ctc_mwer_ws_bytes'][1]) == 5 and len(lib.SIGNATURES['ds2_ctc_mwer_grad'][1]) == 26
    handle = lib.load()
    assert handle.ds2_version() == 404
    assert hasattr(handle, 'ds2_ctc_mwer_grad')
    # the size query: two fp64 planes of (B (N+1), T, 2 L + 1) and small change; 0 for what the entry refuses
    t, bsz, a, n, lmax = 746, 10, 29, 4, 100
    planes = 2 * 8 * bsz * (n + 1) * t * (2 * lmax + 1)
    got = lib.query('ds2_ctc_mwer_ws_bytes', t, bsz, a, n, lmax)
    assert planes <= got <= planes + 16 * bsz * (n + 1) + 8 * t * bsz + 64
    assert lib.query('ds2_ctc_mwer_ws_bytes', t, bsz, a, 0, lmax) == 0
    from ds2hip import ops
    with pytest.raises(RuntimeError, match='device tensors'):
        z = torch.zeros(1, dtype=torch.int32)
        ops.ctc_mwer_grad(torch.zeros(4, 1, 3), z, torch.zeros(1, 1, 4, dtype=torch.int32), z.view(1, 1), z,
                          torch.zeros(1, 1), z, z, z, 1)


def _cfg(block, langs=('en',)):
    return {'model': {'langs': list(langs)}, 'training': {'batch_size': 2, 'mwer': block}}


def test_config_block_defaults_and_refusals():
    from codes.utils import training_utils as tu
    assert tu.get_mwer({'training': {'batch_size': 2}}) is None
    assert tu.get_mwer(_cfg({})) == {'nbest': 4, 'beam_width': 8, 'ctc_weight': 0.01, 'risk': 'word'}
    assert tu.get_mwer(_cfg({'nbest': 2, 'risk': 'char'}), labels=['_', 'A', 'B'])['nbest'] == 2
    for block, word in (({'nbets': 4}, 'nbets'), ({'nbest': 0}, 'nbest'), ({'nbest': 9}, 'nbest'),
                        ({'nbest': 2.5}, 'nbest'), ({'beam_width': 0}, 'beam_width'), ({'beam_width': 129}, 'beam_width'),
                        ({'risk': 'phone'}, 'risk'), ({'ctc_weight': -1}, 'ctc_weight'),
                        ({'ctc_weight': float('nan')}, 'ctc_weight')):
        with pytest.raises(ValueError, match=word):
            tu.get_mwer(_cfg(block))
    with pytest.raises(ValueError, match='space'):
        tu.get_mwer(_cfg({}), labels=['_', 'A', 'B'])
    assert tu.get_mwer(_cfg({}), labels=['_', 'A', ' '])['risk'] == 'word'
    with pytest.raises(ValueError, match='multi-task'):
        tu.get_mwer(_cfg({}, langs=('en', 'pt_BR')))
    # the same refusals where the functions are called directly
    from codes.ctc import MWERLoss, mwer_costs_and_grad
    with pytest.raises(ValueError, match='unknown'):
        MWERLoss(1, nbets=3)
    acts = torch.zeros(4, 1, 3)
    with pytest.raises(ValueError, match='space'):
        mwer_costs_and_grad(acts, [1], [4], [1], -1)
    with pytest.raises(ValueError, match='nbest'):
        mwer_costs_and_grad(acts, [1], [4], [1], 2, nbest=9)
    with pytest.raises(ValueError, match='risk'):
        mwer_costs_and_grad(acts, [1], [4], [1], 2, risk='phone')
