"""The whole training step -- ``DeepSpeech._forward_impl`` / ``_backward_impl`` and ``Trainer._forward_backward`` on top -- against
the float64 oracle on every backward route: one forward and one backward pass per (case, route) of tests/model_cases.py.

Method, reference, yardstick, regimes and conditioning are described in tests/model_cases.py (tests/test_model_cases_cpu.py
proves on the CPU that the cases are what they claim to be).  For every tensor the device produces -- the logits, every
BatchNorm running statistic after the pass, every parameter's gradient -- the test computes e64 (device against float64) and
asserts e64 <= K[family] * e32, as max-abs and as rms, where e32 is the float32 CPU oracle's own error on the same input.
K is one number per family, fixed from one measured run of all cases (profiles/model_fp64_errors.md has the table and the
derivation: twice the worst measured ratio of the family, rounded up to a power of two).

The weight gradients are split-K sums with float atomics, so nothing here is bit-for-bit, with one exception: a slice that
``grad_ready`` reports as final must not change afterwards, so the hook's clones are compared with ``torch.equal``.

What the routes add to the bound:
  fb_nan     NaN in every parameter's gradient view before the pass (the padding words between parameters left alone): the
             bound then also proves that every element was overwritten, not accumulated into.
  trainer    two passes on one trainer with two different inputs, the second one checked: stale sums must not survive.
  hook       reported spans are disjoint, cover the flat buffer, arrive head first, then the layers top-down, then the conv
             block; every clone equals the final buffer.  With the conv block frozen its span is exactly zero.
  raw_dw     ``codes.model._DW_HH_GROUP_MAX_K`` = 0: one gemm_raw per dW_hh problem, ``acc_beta`` 0 (fb_nan) and 1 (trainer).
  T = 1      both weight_hh gradients are exactly zero on both routes.
"""
import pytest
import torch

from tests import model_cases as mc

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# e64 <= K * e32, per tensor family: see profiles/model_fp64_errors.md
K = {'logits': 4.0, 'stats': 4.0, 'head': 4.0, 'rnn': 4.0, 'conv': 4.0}


@pytest.fixture(scope='module')
def ops():
    from ds2hip import ops as _ops
    return _ops


_state = {}


def _state_dict(case):
    if case.name not in _state:
        _state[case.name] = mc.state_dict_for(case)
    return _state[case.name]


class _Table:
    """One printed row per tensor; the bounds are asserted at the end of the case so that one run shows every figure."""

    def __init__(self, case, route, ref):
        self.case, self.route, self.ref, self.bad = case, route, ref, []

    def add(self, name, got):
        r64, (m32, s32) = self.ref['r64'][name], self.ref['e32'][name]
        assert tuple(got.shape) == tuple(r64.shape), (name, got.shape, r64.shape)
        m64, s64 = mc.errors(got, r64)
        rm, rs = m64 / max(m32, mc.TINY), s64 / max(s32, mc.TINY)
        tag = '%s|%s|%s' % (self.case.name, self.route.name, name)
        print('MODELFP64|%s|%.3e|%.3e|%.2f|%.3e|%.3e|%.2f|%.3e' % (tag, m64, m32, rm, s64, s32, rs, self.ref['amax'][name]))
        amax = self.ref['amax'][name]
        if amax >= mc.CONDITION_FLOOR and m32 > mc.CONDITION * amax:
            self.bad.append('BAD CASE %s: the float32 restatement itself is off by %.3e (max|ref| %.3e)' % (tag, m32, amax))
        bound = K[mc.family_of(name)]
        if not (rm <= bound and rs <= bound):
            self.bad.append('%s: e64 / e32 = %.2f (max: %.3e / %.3e), %.2f (rms: %.3e / %.3e) > K = %g'
                            % (tag, rm, m64, m32, rs, s64, s32, bound))

    def check(self, ok, message):
        if not ok:
            self.bad.append('%s|%s: %s' % (self.case.name, self.route.name, message))


def _build(case, route):
    from codes.model import DeepSpeech
    model = DeepSpeech(**case.kwargs)
    model.load_state_dict(_state_dict(case))
    model = model.to(DEV)
    model.train()
    model.overlap_wgrad, model.defer_wgrad = route.overlap, route.defer
    if route.frozen:
        model.conv.requires_grad_(False)
    return model


def _loss_fn(case, batch):
    from codes.ctc import ctc_costs_and_grad
    _, labels, pct, sizes = batch

    def loss_fn(acts):
        return ctc_costs_and_grad(acts, labels, mc.out_sizes_of(pct, acts.shape[0]), sizes, grad_scale=1.0 / case.bsz,
                                  zero_batch_if_inf=True)
    return loss_fn


def _expected_spans(model):
    head, c = model.fc[0].module, model.conv
    spans = [model._span(head[0].weight, head[1].weight)]
    for layer in reversed(list(model.rnns)):
        first = layer.batch_norm.module.weight if layer.batch_norm is not None else layer.rnn.weight_ih_l0
        spans.append(model._span(first, layer.rnn.weight_hh_l0_reverse))
    spans.append(model._span(c[0].weight, c[4].bias))
    return spans


def _make_hook(gflat, log):
    """What ``Trainer._bucket_hook``'s hook does, with a clone in place of the all-reduce."""
    comm = torch.cuda.Stream()

    def ready(lo, hi, also_wait=None, after=None):
        if after is not None:
            comm.wait_event(after)
        else:
            comm.wait_stream(torch.cuda.current_stream())
        if also_wait is not None:
            comm.wait_stream(also_wait)
        with torch.cuda.stream(comm):
            log.append((lo, hi, gflat[lo:hi].clone()))
    return ready


def run_route(ops, monkeypatch, case, route):
    from codes import model as model_mod
    from codes.ctc import CTCLoss
    from codes.engine import Trainer
    ref = mc.reference(case, DEV)
    table = _Table(case, route, ref)
    model = _build(case, route)
    hid, t_out = model._rnn_hidden_size, mc.conv_out_time(case.t_in)
    if hid == 800:
        assert ops.gru_bwd_dh_wanted(torch.device(DEV, torch.cuda.current_device()), case.bsz, hid) == (9 <= case.bsz <= 12)
    raw_calls = []
    if route.raw_dw:
        monkeypatch.setattr(model_mod, '_DW_HH_GROUP_MAX_K', 0)
        real = ops.gemm_raw
        monkeypatch.setattr(ops, 'gemm_raw', lambda *a, **kw: (raw_calls.append(kw.get('beta')), real(*a, **kw))[1])
    batch = mc.inputs_for(case)
    x, labels, pct, sizes = batch
    x = x.to(DEV)
    log = []
    if route.entry == 'autograd':
        logits = model(x)
        loss = CTCLoss()(logits.transpose(0, 1), labels, mc.out_sizes_of(pct, logits.shape[1]), sizes)
        (loss / case.bsz).sum().backward()
        loss_v = float(loss.item()) / case.bsz
    elif route.entry == 'fb':
        filled = model.flat_grad()
        with torch.no_grad():
            for p in model._plist:
                p.grad.fill_(float('nan'))
        costs, acts = model.forward_backward(x, _loss_fn(case, batch))
        assert model.flat_grad() is filled          # the pass wrote into the buffer that held the NaNs
        logits, loss_v = acts.transpose(0, 1), float(costs.sum().item()) / case.bsz
    else:
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, nesterov=True)
        trainer = Trainer(model, opt, device=DEV, max_norm=400)
        assert trainer._fused
        gflat = model.flat_grad()
        buffers = {k: b.clone() for k, b in model.named_buffers() if 'running' in k}
        # first another batch of the same shape, with no synchronisation behind it; the running statistics go back to
        # where they were so that the second pass is the reference's pass
        other = mc.inputs_for(case, other=True)
        trainer._forward_backward(other[0].to(DEV), _loss_fn(case, other), None)
        with torch.no_grad():
            for k, b in model.named_buffers():
                if 'running' in k:
                    b.copy_(buffers[k])
        hook = _make_hook(gflat, log) if route.entry == 'hook' else None
        del raw_calls[:]
        costs, acts = trainer._forward_backward(x, _loss_fn(case, batch), hook)
        logits, loss_v = acts.transpose(0, 1), float(costs.sum().item()) / case.bsz
    torch.cuda.synchronize()
    ops.check_async_errors()

    print('MODELFP64|%s|%s|loss|%.9g|%.9g' % (case.name, route.name, loss_v, ref['loss']))
    table.check(abs(loss_v - ref['loss']) <= mc.CONDITION * abs(ref['loss']), 'loss %r against %r' % (loss_v, ref['loss']))
    table.add('logits', logits)
    for k, v in model.state_dict().items():
        if 'running' in k:
            table.add('buf:' + k, v)
    for k, p in model.named_parameters():
        if route.frozen and k.startswith('conv.'):
            continue
        table.add('grad:' + k, p.grad)

    if t_out == 1:
        for k, p in model.named_parameters():
            if 'weight_hh' in k:
                table.check(bool((p.grad == 0).all()), '%s is not exactly zero at T = 1' % k)
    if route.raw_dw:
        table.check(len(raw_calls) == 4 * len(model.rnns), '%d gemm_raw launches' % len(raw_calls))
        table.check(set(raw_calls) == {1.0 if route.entry == 'trainer' else 0.0}, 'acc_beta %r' % (set(raw_calls),))
    if route.entry == 'hook':
        gflat = model.flat_grad()
        spans = [(lo, hi) for lo, hi, _ in log]
        table.check(spans == _expected_spans(model), 'spans reported as %r' % (spans,))
        edge = 0
        for lo, hi in sorted(spans):
            table.check(lo == edge and hi > lo, 'spans overlap or leave a gap at %d: %r' % (edge, sorted(spans)))
            edge = hi
        table.check(edge == gflat.numel(), 'spans end at %d of %d' % (edge, gflat.numel()))
        for p, o in zip(model._plist, model._offsets):
            table.check(any(lo <= o and o + p.numel() <= hi for lo, hi in spans), 'a parameter at %d is in no span' % o)
        for lo, hi, clone in log:
            table.check(torch.equal(clone, gflat[lo:hi]), 'the slice [%d, %d) changed after it was reported final (%d elements)'
                        % (lo, hi, int((clone != gflat[lo:hi]).sum())))
        if route.frozen:
            lo, hi = spans[-1]
            table.check(bool((gflat[lo:hi] == 0).all()), 'the frozen conv block\'s span is not exactly zero')
    assert not ops._persistent_off                  # no recurrence launch fell back to the launch-per-step kernels
    assert not table.bad, '\n'.join(table.bad)


def _params():
    return [pytest.param(c, r, id='%s-%s' % (c.name, r.name)) for c in mc.cases() for r in c.routes]


@pytest.mark.parametrize('case,route', _params())
def test_training_step_against_fp64(ops, monkeypatch, case, route):
    run_route(ops, monkeypatch, case, route)
