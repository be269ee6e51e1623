"""ds2_ctc_mwer_grad (csrc/ctc_mwer.hip) against its float64 statement tests/mwer_ref.py, against the composition of existing
ops it replaces, and ``codes.ctc.mwer_costs_and_grad`` end to end.  kernel - float64 throughout; the bounds are

  * the project's CTC cost bound as it stands (tests/ctc_cases.py BOUNDS 'main': |cost - ref| <= 2^-20 * tl) for hyp_costs and
    ref_costs;
  * the derived condition |dgrad| / grad_scale <= S_w * G + 2 * dW * (2 * C) per utterance (mwer_ref.grad_condition);
  * MEASURED bounds for the posteriors, the expected risk (relative to max(1, the utterance's largest risk): it is returned
    as a float32 of that magnitude) and the gradient: twice the worst figure over ``CASES`` on an MI355X,
    rounded up to a power of two (profiles/mwer_errors.md has every row).

The `wide` regime of tests/ctc_cases.py is left out: its costs of 1e4 .. 1e5 make every posterior 0 or 1.
"""
import numpy as np
import pytest
import torch

from tests import ctc_cases as cc
from tests import edit_ref, mwer_cases as mc, mwer_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FAM = cc.BOUNDS['main']
# worst measured: posterior 3.43e-7 (A=256), exp_risk 9.03e-8 (count<N), grad_max 5.30e-7 (edge L=255): profiles/mwer_errors.md
MEASURED = {'posterior': 2.0 ** -20, 'exp_risk': 2.0 ** -22, 'grad_max': 2.0 ** -19}
CTC_WEIGHT = 0.3


def _lens(case):
    return [len(h) for rows in case['hyps'] for h in rows] + [len(r) for r in case['refs']]


def pack(case, nbest=None, stride=None):
    """The case as the device search would hand it over: hyp (B,N,stride), hyp_len (B,N), count (B), risk (B,N) -- with
    GARBAGE (labels of 10^6, lengths of -7 and 10^6, NaN risks) in every row at or past the count and behind every row's
    length -- and NaN in acts at and past act_lens."""
    bsz = len(case['refs'])
    n = nbest or case['nbest']
    stride = stride or max(_lens(case) + [1]) + 3
    hyp = np.full((bsz, n, stride), 10 ** 6, dtype=np.int32)
    hyp_len = np.full((bsz, n), -7, dtype=np.int32)
    hyp_len[:, 1::2] = 10 ** 6
    risk = np.full((bsz, n), np.nan, dtype=np.float32)
    count = np.zeros(bsz, dtype=np.int32)
    for b, rows in enumerate(case['hyps']):
        count[b] = len(rows)
        for i, h in enumerate(rows):
            hyp[b, i, :len(h)] = h
            hyp_len[b, i] = len(h)
            risk[b, i] = case['risks'][b][i]
    acts = np.array(case['acts'], dtype=np.float32)
    for b, tl in enumerate(case['act_lens']):
        acts[max(int(tl), 0):, b] = np.nan
    refs = case['refs']
    flat = np.concatenate([np.asarray(r, np.int32) for r in refs] + [np.zeros(1, np.int32)])
    ref_lens = np.array([len(r) for r in refs], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(ref_lens)[:-1]]).astype(np.int32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)     # noqa: E731
    return dict(acts=dev(acts), act_lens=dev(np.asarray(case['act_lens'], np.int32)), hyp=dev(hyp), hyp_len=dev(hyp_len),
                hyp_count=dev(count), risk=dev(risk), ref=dev(flat), ref_offsets=dev(offs), ref_lens=dev(ref_lens))


def run(case, ctc_weight=CTC_WEIGHT, grad_scale=1.0, zero=False, max_label_len=None, ws=None, packed=None):
    from ds2hip import ops
    p = packed or pack(case)
    lmax = max(_lens(case)) if max_label_len is None else max_label_len
    out = ops.ctc_mwer_grad(p['acts'], p['act_lens'], p['hyp'], p['hyp_len'], p['hyp_count'], p['risk'], p['ref'],
                            p['ref_offsets'], p['ref_lens'], lmax, ctc_weight, grad_scale, zero, ws=ws)
    return out


_refs = {}


def reference(case, ctc_weight=CTC_WEIGHT, grad_scale=1.0, zero=False, max_label_len=None):
    key = (case['name'], case['regime'], ctc_weight, grad_scale, zero, max_label_len)
    if key not in _refs:
        _refs[key] = mwer_ref.mwer(case['acts'], case['act_lens'], case['hyps'], case['risks'], case['refs'], ctc_weight,
                                   grad_scale, zero, max_label_len)
    return _refs[key]


def figures(case, got, ref, ctc_weight=CTC_WEIGHT, grad_scale=1.0):
    """Worst figures of one launch against the reference, and the exact checks (which rows are infinite, dropped, zero)."""
    ref_costs, hyp_costs, posterior, exp_risk, dropped, grad = [x.cpu().numpy().astype(np.float64) for x in got]
    bsz, n = posterior.shape
    t_max = case['acts'].shape[0]
    fig = {'cost_per_frame': 0.0, 'posterior': 0.0, 'exp_risk': 0.0, 'grad_max': 0.0, 'cond_ratio': 0.0}
    assert np.all(np.isfinite(grad)), case['name']
    for b in range(bsz):
        tl = max(min(int(case['act_lens'][b]), t_max), 1)
        k = len(case['hyps'][b])
        want = np.concatenate([ref['hyp_costs'][b], [ref['ref_costs'][b]]])
        have = np.concatenate([hyp_costs[b, :k], [ref_costs[b]]])
        assert np.array_equal(np.isinf(want), np.isinf(have)), (case['name'], b, want, have)
        fin = np.isfinite(want)
        if fin.any():
            fig['cost_per_frame'] = max(fig['cost_per_frame'], float(np.abs(want[fin] - have[fin]).max()) / tl)
        assert np.all(np.isinf(hyp_costs[b, k:])) and np.all(posterior[b, k:] == 0.0), (case['name'], b)
        if k:
            fig['posterior'] = max(fig['posterior'], float(np.abs(posterior[b, :k] - ref['posterior'][b]).max()))
            assert np.all(posterior[b, :k][np.isinf(ref['hyp_costs'][b])] == 0.0)
        top = max([1.0] + [abs(float(w)) for w in case['risks'][b]])     # exp_risk is a float32 of that magnitude
        fig['exp_risk'] = max(fig['exp_risk'], abs(exp_risk[b] - ref['exp_risk'][b]) / top)
        assert int(dropped[b]) == int(ref['dropped'][b]), (case['name'], b)
        assert np.all(grad[tl if case['act_lens'][b] > 0 else 0:, b] == 0.0), (case['name'], b)
        err = float(np.abs(grad[:, b] - ref['grad'][:, b]).max()) / abs(grad_scale)
        cond = mwer_ref.grad_condition(ref, b, case['risks'][b], ctc_weight if np.isfinite(ref['ref_costs'][b]) else 0.0,
                                       tl, FAM)
        if not np.any(ref['grad'][:, b] != 0.0):
            assert not np.any(grad[:, b] != 0.0), (case['name'], b)      # no gradient means exactly none
        else:
            fig['cond_ratio'] = max(fig['cond_ratio'], err / cond)
        fig['grad_max'] = max(fig['grad_max'], err)
    return fig


def check(case, fig):
    print('%-28s %-7s cost/frame %.2e  posterior %.2e  exp_risk %.2e  grad %.2e  grad/condition %.3f'
          % (case['name'], case['regime'], fig['cost_per_frame'], fig['posterior'], fig['exp_risk'], fig['grad_max'],
             fig['cond_ratio']))
    assert fig['cost_per_frame'] <= FAM['cost_per_frame'], fig
    assert fig['cond_ratio'] <= 1.0, fig
    for key, bound in MEASURED.items():
        assert fig[key] <= bound, (key, fig)


def _edge(lmax):
    """Row and reference lengths at lmax and one below, B = 2, N = 2, T just above 2 L."""
    return mc.make_case('edge L=%d' % lmax, 'random', 2 * lmax + 8, 29, [lmax, lmax - 1], [2 * lmax + 8, 2 * lmax + 5], 2,
                        hyp_lens=[[lmax - 1, lmax], [lmax, lmax - 7]])


CASES = {
    'random': lambda: mc.make_case('base', 'random', 40, 29, [6, 9, 4], [40, 33, 25], 4),
    'peaked': lambda: mc.make_case('base', 'peaked', 40, 29, [6, 9, 4], [40, 33, 25], 4),
    'count<N': lambda: mc.make_case('count<N', 'random', 40, 29, [6, 9, 4], [40, 33, 25], 4, counts=[4, 2, 1]),
    'N=1': lambda: mc.make_case('N=1', 'random', 40, 29, [6, 9, 4], [40, 33, 25], 1),
    'infeasible hyp': lambda: mc.make_case('infeasible hyp', 'random', 40, 29, [6, 5, 4], [40, 12, 25], 4,
                                           hyp_lens=[[5, 6, 7, 6], [5, 9, 4, 13], [4, 3, 5, 30]]),
    'empty hyp': lambda: mc.make_case('empty hyp', 'random', 40, 29, [6, 9, 4], [40, 33, 25], 4,
                                      hyp_lens=[[0, 6, 5, 7], [9, 0, 8, 10], [4, 5, 3, 0]]),
    'empty ref': lambda: mc.make_case('empty ref', 'random', 40, 29, [0, 9, 0], [40, 33, 25], 4,
                                      hyp_lens=[[0, 1, 2, 1], [9, 8, 8, 10], [1, 1, 2, 0]]),
    'A=2': lambda: mc.make_case('A=2', 'random', 40, 2, [6, 9, 4], [40, 33, 25], 4,
                                hyp_lens=[[5, 6, 7, 4], [9, 8, 10, 7], [4, 5, 3, 2]]),
    'A=256': lambda: mc.make_case('A=256', 'random', 40, 256, [6, 9, 4], [40, 33, 25], 4),
    'L=127': lambda: _edge(127), 'L=128': lambda: _edge(128), 'L=255': lambda: _edge(255), 'L=256': lambda: _edge(256),
    'L=511': lambda: mc.make_case('L=511', 'random', 1030, 29, [500], [1030], 1, hyp_lens=[[511]]),
}
_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_against_float64(name):
    case = get_case(name)
    ref = reference(case)
    if name == 'infeasible hyp':
        assert np.isinf(ref['hyp_costs'][1][3]) and np.isinf(ref['hyp_costs'][2][3])
    check(case, figures(case, run(case), ref))


def test_grad_scale_and_zero_ctc_weight():
    case = get_case('random')
    check(case, figures(case, run(case, 0.0, 0.125), reference(case, 0.0, 0.125), 0.0, 0.125))


def test_dropped_rows_longer_than_max_label_len():
    case = mc.make_case('dropped', 'random', 40, 29, [6, 7, 4], [40, 33, 25], 4, hyp_lens=[[5, 9, 7, 6], [8, 7, 6, 5], [4, 3, 12, 8]])
    ref = reference(case, max_label_len=8)
    assert list(ref['dropped']) == [1, 0, 1]
    check(case, figures(case, run(case, max_label_len=8), ref))


@pytest.mark.parametrize('zero', [False, True])
def test_infeasible_reference(zero):
    case = mc.make_case('infeasible ref', 'random', 40, 29, [6, 21, 4], [40, 22, 25], 4,
                        hyp_lens=[[5, 6, 7, 6], [5, 9, 4, 7], [4, 3, 5, 2]])
    ref = reference(case, zero=zero)
    assert np.isinf(ref['ref_costs'][1]) and np.isfinite(ref['exp_risk'][1])
    got = run(case, zero=zero)
    check(case, figures(case, got, ref))
    grad = got[5].cpu().numpy()
    assert not np.any(grad[:, 1] != 0.0)
    assert np.any(grad[:, 0] != 0.0) != zero and np.any(grad[:, 2] != 0.0) != zero


def test_twenty_launches_on_a_nan_workspace_are_bit_identical():
    from ds2hip import ops
    case = get_case('random')
    p = pack(case)
    nbytes = ops.ctc_mwer_ws_bytes(40, 3, 29, 4, max(_lens(case)))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    first = [x.clone() for x in run(case, ws=ws, packed=p)]
    check(case, figures(case, first, reference(case)))
    for _ in range(19):
        again = run(case, ws=ws, packed=p)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))


def test_argument_refusals():
    from ds2hip import lib, ops
    case = get_case('random')
    p = pack(case)
    t, bsz, a = p['acts'].shape
    n, stride = p['hyp'].shape[1:]
    outs = [torch.empty(s, dtype=d, device=DEV) for s, d in (((bsz,), torch.float32), ((bsz, n), torch.float32),
                                                             ((bsz, n), torch.float32), ((bsz,), torch.float32),
                                                             ((bsz,), torch.int32), ((t, bsz, a), torch.float32))]
    ws = torch.empty(ops.ctc_mwer_ws_bytes(t, bsz, a, n, 16), dtype=torch.uint8, device=DEV)
    good = [p['acts'], p['act_lens'], t, bsz, a, p['hyp'], p['hyp_len'], p['hyp_count'], n, stride, p['risk'], p['ref'],
            p['ref_offsets'], p['ref_lens'], 16, 0.3, 1.0, 0] + outs + [ws]
    lib.call('ds2_ctc_mwer_grad', *good)
    for pos, bad in ((2, 0), (3, 0), (3, 65536), (4, 1), (4, 257), (8, 0), (8, 129), (9, -1), (14, -1), (14, 512),
                     (15, -0.5), (15, float('inf')), (16, float('nan')), (0, None), (5, None), (10, None), (13, None),
                     (18, None), (22, None), (23, None), (24, None)):
        args = list(good)
        args[pos] = bad
        with pytest.raises(lib.Ds2Error) as err:
            lib.call('ds2_ctc_mwer_grad', *args)
        assert err.value.code == lib.ERR_ARG and 'ds2_ctc_mwer_grad' in str(err.value), (pos, bad)
    assert ops.ctc_mwer_ws_bytes(t, bsz, a, 0, 16) == 0
    with pytest.raises(RuntimeError, match='ws holds'):
        ops.ctc_mwer_grad(p['acts'], p['act_lens'], p['hyp'], p['hyp_len'], p['hyp_count'], p['risk'], p['ref'],
                          p['ref_offsets'], p['ref_lens'], 16, ws=ws[:64])
    with pytest.raises(RuntimeError, match='must be'):
        ops.ctc_mwer_grad(p['acts'], p['act_lens'], p['hyp'], p['hyp_len'], p['hyp_count'], p['risk'].double(), p['ref'],
                          p['ref_offsets'], p['ref_lens'], 16)


def composition(case, ctc_weight, grad_scale=1.0):
    """What the kernel replaces, from existing ops: acts replicated to (T, B (N+1), A), ONE ds2_ctc_loss_grad call over all
    rows, the posteriors and the weighted sum in torch (float64)."""
    from ds2hip import ops
    bsz, n = len(case['refs']), case['nbest']
    assert all(len(rows) == n for rows in case['hyps'])
    rows = [h for b in range(bsz) for h in list(case['hyps'][b]) + [case['refs'][b]]]
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    flat = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(1, np.int32)])
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    act_lens = np.repeat(np.asarray(case['act_lens'], np.int32), n + 1)
    acts = torch.from_numpy(case['acts']).to(DEV)
    rep = acts.repeat_interleave(n + 1, dim=1).contiguous()
    dev = lambda x: torch.from_numpy(x).to(DEV)                             # noqa: E731
    costs, grads = ops.ctc_loss_grad(rep, dev(flat), dev(offs), dev(lens), dev(act_lens), int(lens.max()))
    c = costs.double().view(bsz, n + 1)
    risk = torch.tensor(np.array(case['risks']), dtype=torch.float64, device=DEV)
    post = torch.softmax(-c[:, :n], 1)
    exp_risk = (post * risk).sum(1, keepdim=True)
    w = torch.cat([-post * (risk - exp_risk), torch.full((bsz, 1), ctc_weight, dtype=torch.float64, device=DEV)], 1)
    g = grads.double().view(acts.shape[0], bsz, n + 1, acts.shape[2])
    return (grad_scale * (g * w.view(1, bsz, n + 1, 1)).sum(2)).cpu().numpy(), exp_risk.view(-1).cpu().numpy()


@pytest.mark.parametrize('name', ['random', 'peaked'])
def test_kernel_against_the_composition_of_existing_ops(name):
    """A second reference that runs on the GPU and shares nothing with ctc_mwer.hip but the recursion's source.  Both sides
    meet the derived condition against float64 (the composition's rows through tests/test_ctc_fp64_gpu.py's bounds), so
    they differ by at most twice it."""
    case = get_case(name)
    assert all(np.all(np.isfinite(c)) for c in reference(case)['hyp_costs'])
    got = run(case)
    want, exp_risk = composition(case, CTC_WEIGHT)
    grad = got[5].cpu().numpy().astype(np.float64)
    ref = reference(case)
    for b in range(len(case['refs'])):
        tl = int(case['act_lens'][b])
        cond = mwer_ref.grad_condition(ref, b, case['risks'][b], CTC_WEIGHT, tl, FAM)
        err = float(np.abs(grad[:tl, b] - want[:tl, b]).max())
        print('%s utterance %d: kernel - composition %.2e, 2 x condition %.2e' % (name, b, err, 2 * cond))
        assert err <= 2.0 * cond
        # the expected risks: each side's costs are within C = cost_per_frame * tl of float64, which moves a posterior by
        # at most 2 C and the expected risk by at most 2 C times the spread of the risks (the condition's second term)
        spread = float(max(case['risks'][b]) - min(case['risks'][b]))
        assert abs(float(got[3][b]) - exp_risk[b]) <= 2.0 * (2.0 * spread * 2.0 * FAM['cost_per_frame'] * tl)


def test_a_step_along_the_gradient_lowers_the_expected_risk():
    """ctc_weight = 0: after acts -= lr * grad, the float64 expected risk over the SAME fixed hypothesis list is lower for
    every utterance (tests/test_mwer_cpu.py shows that the reference's own gradient gives descent at this lr)."""
    case = mc.descent_case()
    assert all(len(set(r)) >= 2 for r in case['risks'])
    before = reference(case, 0.0)['exp_risk']
    grad = run(case, 0.0)[5].cpu().numpy().astype(np.float64)
    acts = np.where(np.isfinite(grad), case['acts'].astype(np.float64) - mc.DESCENT_LR * grad, 0.0)
    after = mwer_ref.expected_risk(acts, case['act_lens'], case['hyps'], case['risks'])
    print('expected risk before', before, 'after', after)
    assert np.all(after < before)


def _e2e_inputs():
    rng = np.random.default_rng(2024)
    t, bsz, a, space = 60, 4, 29, 1
    refs = []
    for n in (12, 9, 15, 7):
        lab = rng.integers(2, a, size=n)
        lab[3::4] = space
        refs.append(lab.astype(np.int32))
    act_lens = np.array([60, 51, 60, 38], np.int32)
    acts = cc.make_acts(rng, 'peaked', t, a, refs, act_lens)
    acts = (0.25 * acts + 1.0 * rng.standard_normal(acts.shape)).astype(np.float32)     # an unsure model: alternatives differ
    return acts, act_lens, refs, space


def end_to_end(risk):
    """``mwer_costs_and_grad`` at T = 60, B = 4 against the reference pipeline fed with the hypotheses the device search
    returned, read back: tests/edit_ref.py for the distances (``==``), mwer_ref for the rest.  Returns (case, figures,
    loss error)."""
    from codes.ctc import mwer_costs_and_grad
    acts, act_lens, refs, space = _e2e_inputs()
    bsz, n = len(refs), 4
    targets = torch.from_numpy(np.concatenate(refs))
    sizes = torch.tensor([len(r) for r in refs], dtype=torch.int32)
    loss, grad, info = mwer_costs_and_grad(torch.from_numpy(acts).to(DEV), targets, torch.from_numpy(act_lens), sizes, space,
                                           nbest=n, beam_width=8, ctc_weight=0.05, risk=risk, grad_scale=0.25)
    hyp, hyp_len, count = info['hyp'].cpu().numpy(), info['hyp_len'].cpu().numpy(), info['count'].cpu().numpy()
    assert count.min() >= 2                                              # there are alternatives to weigh
    hyps = [[hyp[b, i, :hyp_len[b, i]] for i in range(count[b])] for b in range(bsz)]
    col = 5 if risk == 'word' else 0
    risks = [[float(edit_ref.edit_stats_row(list(h), list(refs[b]), space)[col]) for h in hyps[b]] for b in range(bsz)]
    got_risk = info['risk'].cpu().numpy()
    for b in range(bsz):
        assert list(got_risk[b, :count[b]]) == risks[b]
    case = {'name': 'e2e ' + risk, 'regime': 'e2e', 'acts': acts, 'act_lens': act_lens, 'hyps': hyps, 'risks': risks,
            'refs': refs, 'nbest': n}
    ref = mwer_ref.mwer(acts, act_lens, hyps, risks, refs, 0.05, 0.25)
    got = (info['ref_costs'], torch.full((bsz, n), float('inf')), info['posterior'], info['exp_risk'], info['dropped'], grad)
    hyp_costs = got[1].clone()
    for b in range(bsz):                         # (the function does not hand the rows' costs on: take the reference's pattern)
        hyp_costs[b, :count[b]] = torch.from_numpy(ref['hyp_costs'][b]).float()
    want_loss = ref['exp_risk'] + 0.05 * ref['ref_costs']
    top = np.array([max([1.0] + r) for r in risks])
    loss_err = np.abs(loss.cpu().numpy() - want_loss) - 0.05 * FAM['cost_per_frame'] * act_lens   # what the cost bound allows
    return case, figures(case, (got[0], hyp_costs) + got[2:], ref, 0.05, 0.25), float((loss_err / top).max())


@pytest.mark.parametrize('risk', ['word', 'char'])
def test_end_to_end_against_the_reference_pipeline(risk):
    case, fig, loss_err = end_to_end(risk)
    check(case, fig)
    assert loss_err <= MEASURED['exp_risk']            # (relative to the largest risk, beyond the CTC term's own cost bound)
