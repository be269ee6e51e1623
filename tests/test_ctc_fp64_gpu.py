"""The CTC loss and gradient kernels (csrc/ctc.hip) against float64 at the size we train, and at every boundary of the code.

Reference: oracle/ctc.py ``ctc_loss_and_grad_fast`` in float64 (tests/test_ctc_ref_cpu.py ties it to the loop oracle, to path
enumeration and to torch's ctc_loss in double), and two closed forms with no floating-point recursion in them (all-equal
activations; single-path utterances).  Every case prints one row

    CTCFP64|case|regime|B|A|cost abs|cost rel|cost / frame|grad max|grad rms        (gradient figures divided by grad_scale)

of kernel - float64 and asserts, at its end, the CONDITIONS the suite already made (gradient 5e-5, cost 1e-4 relative) and the
MEASURED BOUNDS of its family (tests/ctc_cases.py BOUNDS; profiles/ctc_fp64_errors.md has every row of the run they come from).
tests/test_ctc_ref_cpu.py proves that fp32 log-space CTC and two wrong recursions fall outside those bounds.

The cost of an utterance is sequential arithmetic of one workgroup and therefore deterministic: the invariants on costs are
asserted bit for bit.  The gradient sums label states with LDS float atomics; it is held to the bounds instead.

Near-zero costs.  The `peaked` cases hold utterances whose cost is 4e-7 .. 2e-4 (a short clip on which every frame is confidently
right), and the 1e-4 RELATIVE cost condition applies to them too.  The kernels first missed it there by 5e-2 .. 2.1 (a cost of
exactly 0 returned for a true 4e-7): the row log-sum-exp was kept as one float and a - lse was formed at |a| ~ 20, where the
spacing is 1.9e-6, and the recursion's log(1 + small) dropped every term below 6e-8.  csrc/ctc.hip now keeps the row maximum and
log1p(sum of the other terms) apart and forms the recursion's log term as log1p of the two smaller terms; the worst relative
cost error of the file is 6.9e-6 (profiles/ctc_fp64_errors.md has the rows before and after).
"""
import numpy as np
import pytest
import torch

from tests import ctc_cases as cc
from tests.test_ctc_ref_cpu import single_path_case

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _args(case, acts=None):
    """Device tensors (acts, labels, offsets, label_lens, act_lens) and max_label_len of a case."""
    lens = case['label_lens']
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    labels = case['labels'] if case['labels'].size else np.zeros(1, np.int32)
    return (_dev(case['acts'] if acts is None else acts), _dev(labels), _dev(offs), _dev(lens), _dev(case['act_lens'])), int(lens.max())


def launch(ops, case, grad_scale=1.0, zero_batch_if_inf=False, acts=None):
    args, max_len = _args(case, acts)
    costs, grad = ops.ctc_loss_grad(*args, max_len, grad_scale, zero_batch_if_inf)
    torch.cuda.synchronize()
    return costs.cpu().numpy(), grad.cpu().numpy()


def row(label, case, costs, grad, grad_scale=1.0, ref=None):
    """Print the case's row and return what it misses (a list of strings, empty when all is met)."""
    rc, rg = ref if ref is not None else cc.reference(case)
    err = cc.errors(case, costs, grad, rc, rg, grad_scale)
    t_max, bsz, nalpha = case['acts'].shape
    print('CTCFP64|%s|%s|%d|%d|%.3e|%.3e|%.3e|%.3e|%.3e' % (label, case['regime'], bsz, nalpha, err['cost_abs'], err['cost_rel'],
                                                          err['cost_per_frame'], err['grad_max'], err['grad_rms']))
    return ['%s %s: %s' % (label, case['regime'], v) for v in cc.violations(err, case['regime'])]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def nan_padded(case):
    acts = case['acts'].copy()
    for b, tl in enumerate(case['act_lens']):
        acts[int(tl):, b] = np.nan
    return acts


# --------------------------------------------------------------------------------------------- training size
@pytest.mark.parametrize('bsz,nalpha,regime', cc.MATRIX, ids=['B%d-A%d-%s' % m for m in cc.MATRIX])
def test_training_size(ops, bsz, nalpha, regime):
    """T = 746, mixed lengths in one batch (L = 0 .. 300, full-length and short clips), every regime; then the same case with
    NaN in every padded frame: costs unchanged bit for bit, gradient exactly 0 in the padding and still within the bounds."""
    case = cc.matrix_case(bsz, nalpha, regime)
    costs, grad = launch(ops, case)
    bad = row(case['name'], case, costs, grad)
    costs_n, grad_n = launch(ops, case, acts=nan_padded(case))
    bad += row(case['name'] + ', NaN padding', case, costs_n, grad_n)
    assert same_bits(costs, costs_n)
    for b, tl in enumerate(case['act_lens']):
        assert np.all(grad_n[int(tl):, b] == 0) and np.all(grad[int(tl):, b] == 0)
    assert not bad, '\n'.join(bad)


# --------------------------------------------------------------------------------------------- structural edges
EDGE_REGIMES = ('random', 'peaked')


@pytest.mark.parametrize('regime', EDGE_REGIMES)
@pytest.mark.parametrize('length', [127, 128, 255, 256, 511])
def test_state_count_at_each_template_switch(ops, length, regime):
    """S = 2 L + 1 = 255 | 257 (256- / 512-thread form), 511 | 513 (512 / 1024) and 1023 = MAX_S - 1, the longest transcript."""
    case = cc.make_case('L=%d' % length, regime, 746, 29, [length, 5], [746, 400])
    costs, grad = launch(ops, case)
    bad = row(case['name'], case, costs, grad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('regime', EDGE_REGIMES)
def test_short_utterance_in_the_1024_thread_form(ops, regime):
    case = cc.make_case('L=3 beside L=511', regime, 746, 29, [3, 511, 0], [40, 746, 746])
    costs, grad = launch(ops, case)
    bad = row(case['name'], case, costs, grad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('regime', EDGE_REGIMES)
@pytest.mark.parametrize('nalpha', [2, 32, 33, 64, 65, 128, 129, 256])
def test_alphabet_sizes(ops, nalpha, regime):
    """CH = min(32, 1024 / A) starts to shrink at A = 33 and is 4 at A = 256; the row log-sum-exp loops once A > 64, the
    gradient kernel once A > 128, and its occupancy row is exactly full at A = 256.  Every transcript uses symbol A - 1."""
    case = cc.make_case('A=%d' % nalpha, regime, 80, nalpha, [12, 0, 30], [80, 37, 71], top=True)
    assert all((lab == nalpha - 1).any() for lab in case['labels_per_utt'] if len(lab))
    costs, grad = launch(ops, case)
    bad = row(case['name'], case, costs, grad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('regime', EDGE_REGIMES)
@pytest.mark.parametrize('nalpha,ch', [(29, 32), (43, 23), (256, 4)])
def test_utterance_lengths_around_the_staging_chunks(ops, nalpha, ch, regime):
    """tl = 1 (no chunk at all), CH, CH + 1 (the steps an exact multiple of CH), 2 CH, 2 CH + 1, and act_lens = T + 5, which
    means T."""
    assert ch == min(32, 1024 // nalpha)
    t_max = 2 * ch + 1
    case = cc.make_case('A=%d tl around CH=%d' % (nalpha, ch), regime, t_max, nalpha, [1, 2, 0, 2, 2, 0, 2],
                        [1, ch, ch + 1, 2 * ch, 2 * ch + 1, 1, t_max + 5], top=True)
    costs, grad = launch(ops, case)
    bad = row(case['name'], case, costs, grad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('regime', EDGE_REGIMES)
@pytest.mark.parametrize('grad_scale', [1 / 10, 0.3 / 7], ids=['1/10', '0.3/7'])
def test_grad_scale(ops, grad_scale, regime):
    """What training passes: 1 / B, or w_i / n per task.  Costs are not scaled; the gradient is, all of it."""
    case = cc.make_case('grad_scale', regime, 120, 29, [20, 0, 45, 7], [120, 64, 111, 33])
    costs, grad = launch(ops, case, grad_scale=grad_scale)
    costs1, _ = launch(ops, case)
    bad = row('grad_scale=%.4f' % grad_scale, case, costs, grad, grad_scale=grad_scale)
    assert same_bits(costs, costs1)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('regime', ['random', 'peaked', 'wide'])
def test_single_path_closed_form(ops, regime):
    """tl = L + repeats (and L = 0): one alignment, cost = -sum log p along it, gradient = softmax - one-hot."""
    case = single_path_case(regime)
    costs, grad = launch(ops, case)
    bad = row('single path', case, costs, grad, ref=cc.single_path(case))
    assert not bad, '\n'.join(bad)


def test_argument_refusals(ops):
    """A = 257, A = 1 and max_label_len = 512 are refused with DS2_ERR_ARG before anything is launched."""
    from ds2hip import lib
    labels, offs, lens, act_lens = (_dev(np.asarray(x, np.int32)) for x in ([1, 1], [0, 1], [1, 1], [4, 4]))
    for nalpha, max_len in ((257, 1), (1, 1), (29, 512)):
        acts = torch.zeros(4, 2, nalpha, device=DEV)
        costs = torch.full((2,), 7.0, device=DEV)
        grad = torch.full((4, 2, nalpha), 7.0, device=DEV)
        ws = torch.empty(lib.query('ds2_ctc_ws_bytes', 4, 2, nalpha, 1), dtype=torch.uint8, device=DEV)
        with pytest.raises(lib.Ds2Error) as ei:
            lib.call('ds2_ctc_loss_grad', acts, labels, offs, lens, act_lens, 4, 2, nalpha, max_len, 1.0, 0, costs, grad, ws)
        assert ei.value.code == lib.ERR_ARG
        torch.cuda.synchronize()
        assert bool((costs == 7.0).all()) and bool((grad == 7.0).all())


# --------------------------------------------------------------------------------------------- invariants, bit for bit
def _placed(ops, u, others, pos):
    """Costs and gradient of utterance ``u`` (a B = 1 case) at position ``pos`` of a batch filled up with ``others``."""
    bsz = others['acts'].shape[1] + 1
    order = list(range(pos)) + [-1] + list(range(pos, bsz - 1))
    pick = lambda key: [u[key][0] if i < 0 else others[key][i] for i in order]            # noqa: E731
    acts = np.stack([u['acts'][:, 0] if i < 0 else others['acts'][:, i] for i in order], 1)
    labs = pick('labels_per_utt')
    case = {'name': 'placed', 'regime': u['regime'], 'acts': acts, 'labels_per_utt': labs,
            'labels': np.concatenate(labs).astype(np.int32), 'label_lens': np.asarray(pick('label_lens'), np.int32),
            'act_lens': np.asarray(pick('act_lens'), np.int32)}
    costs, grad = launch(ops, case)
    return costs[pos:pos + 1], grad[:, pos:pos + 1]


@pytest.mark.parametrize('regime', EDGE_REGIMES)
def test_cost_does_not_depend_on_position_or_company(ops, regime):
    """One utterance alone, first and last of a B = 64 batch, and beside an L = 511 transcript (1024-thread form, other smax):
    the same cost to the bit, the gradient within the bounds every time."""
    u = cc.make_case('the utterance', regime, 746, 29, [100], [700])
    rng = np.random.default_rng(5)
    others = cc.make_case('63 others', regime, 746, 29, list(rng.integers(0, 40, 63)), list(rng.integers(100, 747, 63)))
    longer = cc.make_case('one long other', regime, 746, 29, [511], [746])
    alone, grad = launch(ops, u)
    bad = row('alone', u, alone, grad)
    for label, (c, g) in (('position 0 of 64', _placed(ops, u, others, 0)), ('position 63 of 64', _placed(ops, u, others, 63)),
                          ('after L=511', _placed(ops, u, longer, 1)), ('before L=511', _placed(ops, u, longer, 0))):
        bad += row(label, u, c, g)
        assert same_bits(c, alone), label
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('fill', ['as left by the last launch', 'NaN bytes'])
def test_twenty_launches_on_one_workspace(ops, fill):
    """The entry point on a workspace of the test's own, 20 times: identical costs, also when every byte of the workspace is
    0xff (a NaN in every double and float) before each launch -- nothing is read from rows t >= tl or states s >= S."""
    from ds2hip import lib
    case = cc.make_case('one workspace', 'random', 746, 29, [200, 0, 30, 511, 1], [746, 300, 91, 746, 1])
    (acts, labels, offs, lens, act_lens), max_len = _args(case)
    t_max, bsz, nalpha = case['acts'].shape
    ws = torch.zeros(lib.query('ds2_ctc_ws_bytes', t_max, bsz, nalpha, max_len), dtype=torch.uint8, device=DEV)
    bad, first = [], None
    for i in range(20):
        if fill == 'NaN bytes':
            ws.fill_(255)
        costs, grad = torch.full((bsz,), 7.0, device=DEV), torch.full(case['acts'].shape, 7.0, device=DEV)
        lib.call('ds2_ctc_loss_grad', acts, labels, offs, lens, act_lens, t_max, bsz, nalpha, max_len, 1.0, 0, costs, grad, ws)
        torch.cuda.synchronize()
        costs, grad = costs.cpu().numpy(), grad.cpu().numpy()
        if i in (0, 19):
            bad += row('launch %d, workspace %s' % (i + 1, fill), case, costs, grad)
        else:
            bad += ['launch %d: %s' % (i + 1, v) for v in
                    cc.violations(cc.errors(case, costs, grad, *cc.reference(case)), case['regime'])]
        first = costs if first is None else first
        assert same_bits(costs, first), 'launch %d' % (i + 1)
    reused, _ = launch(ops, case)                        # and the cached workspace of ops gives the same costs
    assert same_bits(reused, first)
    assert not bad, '\n'.join(bad)


def test_zero_batch_if_inf_beyond_one_stride(ops):
    """B = 200 (the flag's scan of the costs walks in strides of 128 threads) with the one infeasible utterance last, then
    first: costs as without the flag, every gradient element exactly 0.  Without an infeasible utterance it changes nothing."""
    rng = np.random.default_rng(8)
    lens, acts_len = list(rng.integers(0, 9, 200)), list(rng.integers(24, 41, 200))
    feasible = cc.make_case('B=200', 'random', 40, 29, lens, acts_len)
    c0, g0 = launch(ops, feasible)
    c1, g1 = launch(ops, feasible, zero_batch_if_inf=True)
    bad = row('B=200 feasible', feasible, c0, g0) + row('B=200 feasible, flag', feasible, c1, g1)
    assert same_bits(c0, c1)
    for where in (199, 0):
        labels = [np.asarray(x) for x in feasible['labels_per_utt']]
        labels[where] = np.full(5, 3, np.int32)                     # five equal labels need nine frames
        lens2, acts_len2 = list(lens), list(acts_len)
        lens2[where], acts_len2[where] = 5, 6
        case = cc.make_case('B=200, infeasible at %d' % where, 'random', 40, 29, lens2, acts_len2, labels=labels)
        c0, g0 = launch(ops, case)
        c1, g1 = launch(ops, case, zero_batch_if_inf=True)
        bad += row(case['name'], case, c0, g0)
        assert np.isposinf(c0[where]) and np.isfinite(np.delete(c0, where)).all() and np.all(g0[:, where] == 0)
        assert same_bits(c0, c1)
        assert np.all(g1 == 0)
    assert not bad, '\n'.join(bad)


def test_nan_inside_a_valid_frame_stays_in_its_utterance(ops):
    """One NaN activation in a valid frame of utterance b.  Asserted: every other utterance's cost is bit identical to the clean
    run, b's cost is not finite, and without ``zero_batch_if_inf`` the others' gradient is within the bounds.

    Observed on an MI355X (the CTCNAN lines): the NaN frame makes every state of b NaN, and fmax, which ignores a NaN operand,
    turns the next frame's states into -inf: b ends as an INFEASIBLE utterance, cost +inf, its own gradient exactly 0, no NaN
    anywhere in the batch's gradient.  With ``zero_batch_if_inf`` the +inf cost then zeroes the whole batch's gradient, the
    flag's rule -- the same outcome the autograd path reaches through the trainer's +-inf rule (codes/engine.py:27-30)."""
    case = cc.make_case('NaN inside', 'random', 120, 29, [20, 0, 45, 7], [120, 64, 111, 33])
    b, t_nan = 2, 50
    clean, _ = launch(ops, case)
    acts = case['acts'].copy()
    acts[t_nan, b, 5] = np.nan
    rc, rg = cc.reference(case)
    keep = [i for i in range(4) if i != b]
    sub = dict(case, act_lens=case['act_lens'][keep], acts=case['acts'][:, keep])       # (for the error figures only)
    bad = []
    for flag in (False, True):
        costs, grad = launch(ops, case, zero_batch_if_inf=flag, acts=acts)
        gb = grad[:, b]
        print('CTCNAN|zero_batch_if_inf=%d|cost[b]=%r|grad[b]: %d NaN of %d in valid frames, %d non-zero in padding|others: %d NaN'
              % (flag, float(costs[b]), int(np.isnan(gb[:111]).sum()), gb[:111].size, int((gb[111:] != 0).sum()),
                 int(np.isnan(grad[:, keep]).sum())))
        assert not np.isfinite(costs[b])
        assert same_bits(costs[keep], clean[keep])
        if flag and np.isinf(costs[b]):
            assert np.all(grad == 0)                    # an infinite cost under the flag: the whole batch, exactly
        else:
            bad += row('NaN in utterance %d, flag %d: the others' % (b, flag), sub, costs[keep], grad[:, keep], ref=(rc[keep], rg[:, keep]))
    assert not bad, '\n'.join(bad)


# --------------------------------------------------------------------------------------------- the host wrapper
def test_host_wrapper(ops):
    from codes.ctc import CTCLoss, ctc_costs_and_grad
    bad = []
    # B = 1; labels / lengths as int64 CPU tensors and as device tensors
    one = cc.make_case('wrapper B=1', 'random', 50, 29, [9], [50])
    for where in ('cpu', DEV):
        to = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int64).to(where)      # noqa: E731
        c, g = ctc_costs_and_grad(_dev(one['acts']), to(one['labels']), to(one['act_lens']), to(one['label_lens']))
        bad += row('wrapper B=1, int64 on %s' % where, one, c.cpu().numpy(), g.cpu().numpy())
    # every transcript empty
    empty = cc.make_case('wrapper all empty', 'random', 30, 29, [0, 0, 0], [30, 1, 17])
    c, g = ctc_costs_and_grad(_dev(empty['acts']), torch.zeros(0, dtype=torch.int32), torch.as_tensor(empty['act_lens']),
                              torch.as_tensor(empty['label_lens']), grad_scale=1 / 3)
    bad += row('wrapper all empty', empty, c.cpu().numpy(), g.cpu().numpy(), grad_scale=1 / 3)
    # autograd with an upstream factor
    case = cc.make_case('wrapper autograd', 'peaked', 120, 29, [20, 0, 45, 7], [120, 64, 111, 33])
    a = _dev(case['acts']).requires_grad_(True)
    loss = CTCLoss()(a, torch.as_tensor(case['labels']), torch.as_tensor(case['act_lens']), torch.as_tensor(case['label_lens']))
    assert loss.shape == (1,)
    (loss * 0.37 / 4).sum().backward()
    rc, rg = cc.reference(case)
    assert abs(float(loss) - rc.sum()) <= cc.COND_COST_REL * rc.sum()
    costs, _ = launch(ops, case)
    bad += row('CTCLoss, upstream 0.37 / 4', case, costs, a.grad.cpu().numpy(), grad_scale=0.37 / 4)
    assert not bad, '\n'.join(bad)


def test_host_wrapper_refuses_what_the_kernel_cannot_check(ops):
    """A label >= A, a negative label, more labels promised than given, lengths that do not match B: the kernels would index
    out of bounds with them, so the wrapper raises before anything reaches the device."""
    from codes.ctc import ctc_costs_and_grad
    acts = torch.zeros(8, 2, 5, device=DEV)
    ok = ([1, 4, 2], [8, 8], [2, 1])
    ctc_costs_and_grad(acts, *[torch.tensor(x) for x in ok])
    for labels, act_lens, label_lens in (([1, 5, 2], [8, 8], [2, 1]), ([1, -1, 2], [8, 8], [2, 1]), ([1, 4, 2], [8, 8], [2, 2]),
                                         ([1, 4, 2], [8, 8], [4, -1]), ([1, 4, 2], [8], [2, 1]), ([1, 4, 2], [8, 8, 8], [2, 1, 0])):
        with pytest.raises(ValueError):
            ctc_costs_and_grad(acts, torch.tensor(labels), torch.tensor(act_lens), torch.tensor(label_lens))
