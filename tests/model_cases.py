"""Cases, float64 reference and yardstick of the whole-step suite (tests/test_model_fp64_gpu.py): one forward and one backward
pass of ``codes.model.DeepSpeech`` on every backward route, against ``oracle.model.OracleDeepSpeech`` in float64.  No GPU.

The method is that of tests/test_gru_fp64_gpu.py, unchanged.  The reference is the oracle model in float64 (the golden files
pin it to the reference project) with ``seeded_state_dict`` weights, the loss ``F.ctc_loss(log_softmax(logits), ...,
reduction='sum') / B``.  The yardstick is the SAME oracle in float32 on the CPU: its error against float64, e32, is what
correctly rounded float32 arithmetic in another summation order costs on exactly this input.  For every tensor the device
produces the GPU test computes e64 (device against float64) and asserts e64 <= K[family] * e32, as max-abs and as rms; e32
never comes from device code.  The rule is absolute, so it also holds the gradients that are exactly zero (a conv bias in
front of a BatchNorm; ``conv.1.bias`` where nothing is clipped); TINY keeps the ratio finite where both sides are exact.

Families (one K each, profiles/model_fp64_errors.md has the measured table and the derivation): 'logits'; 'stats' (every
BatchNorm running mean and variance after the pass); 'head' (gradients of ``fc.*``); 'rnn' (gradients of ``rnns.*``: per layer
BatchNorm, weight_ih*, weight_hh*, both directions); 'conv' (gradients of ``conv.*``).

Regimes of the conv block's hard clip: 'seeded' = the plain ``seeded_state_dict`` (about half of both conv outputs sit on the
lower clip), 'open' = the same with ``conv.1`` / ``conv.4`` weight = 2 and bias = 10 (nothing clipped at either end, so the
whole step is a smooth function of its inputs).  The clip mask reaches only the conv block's own gradients.

Conditioning: a case is usable only where the float32 restatement itself stays within CONDITION * max|ref| of float64 for
every held tensor with max|ref| >= 1e-6 (tests/test_model_cases_cpu.py asserts it for every case; a case that misses it is
replaced, never loosened).

References are computed once per case and shared by the routes (``reference``'s module-level cache).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle.model import OracleDeepSpeech, conv_out_time, seeded_state_dict
from tests.golden.make_golden import seeded_inputs, seeded_labels

TINY = 1e-12            # as tests/test_gru_fp64_gpu.py: only keeps the ratio finite where the float32 restatement is exact
CONDITION = 2e-4        # float32 restatement against float64, times max|ref|
CONDITION_FLOOR = 1e-6  # tensors smaller than this everywhere (the exactly-zero gradients) have no relative conditioning

FAMILIES = ('logits', 'stats', 'head', 'rnn', 'conv')
REGIMES = ('seeded', 'open')

PROD = dict()                                             # H = 800, five layers
WIDE2 = dict(rnn_hidden_size=800, num_rnn_layers=2)
TINY2 = dict(rnn_hidden_size=32, num_rnn_layers=2)

# ------------------------------------------------------------------------------------------------- routes
# entry:   'autograd' = model(x), CTCLoss, .backward() (prezeroed=False, no hook, a fresh gradient buffer)
#          'fb'       = DeepSpeech.forward_backward with NaN in every parameter's gradient view beforehand (prezeroed=False)
#          'trainer'  = Trainer._forward_backward(hook=None), run twice with two inputs, the second pass checked (prezeroed=True)
#          'hook'     = Trainer._forward_backward with a grad_ready hook that clones each reported slice on its own stream
# overlap / defer: DeepSpeech.overlap_wgrad / defer_wgrad;  frozen: requires_grad_(False) on model.conv
# raw_dw:  codes.model._DW_HH_GROUP_MAX_K set to 0, so that every dW_hh problem goes through gemm_raw
Route = namedtuple('Route', 'name entry overlap defer frozen raw_dw')


def _route(name, entry, overlap=True, defer=True, frozen=False, raw_dw=False):
    return Route(name, entry, overlap, defer, frozen, raw_dw)


AUTOGRAD = _route('autograd', 'autograd')
FB = _route('fb_nan', 'fb')
TRAINER = _route('trainer', 'trainer')
PROD_ROUTES = (AUTOGRAD, FB, TRAINER,
               _route('fb_nan-no_overlap', 'fb', overlap=False), _route('trainer-no_overlap', 'trainer', overlap=False),
               _route('fb_nan-no_defer', 'fb', defer=False), _route('trainer-no_defer', 'trainer', defer=False),
               _route('hook-defer', 'hook'), _route('hook-no_defer', 'hook', defer=False),
               _route('hook-frozen_conv', 'hook', frozen=True))
RAW_ROUTES = (_route('fb_nan-raw_dw', 'fb', raw_dw=True), _route('trainer-raw_dw', 'trainer', raw_dw=True))

Case = namedtuple('Case', 'name kwargs bsz t_in regime seed lengths label_lens routes')


def _label_lens(bsz, t_out):
    """3 .. 8 labels per utterance (at most t_out // 2, so that any transcript is feasible), 0 .. 1 at a single frame."""
    if t_out == 1:
        return [(i + 1) % 2 for i in range(bsz)]
    return [min(3 + (5 * i) % 6, t_out // 2) for i in range(bsz)]


def cases():
    out = []

    def add(name, kwargs, bsz, t_in, regime, routes, seed, lengths=None, label_lens=None):
        if label_lens is None:
            label_lens = _label_lens(bsz, conv_out_time(t_in))
        out.append(Case(name, kwargs, bsz, t_in, regime, seed, lengths, tuple(label_lens), tuple(routes)))

    # the production shape: the d(h)-hand-off recurrence, the coefficient planes, spare_cus = 82 under the top layer and the
    # deferred weight-gradient GEMMs all run together
    add('prod-seeded', PROD, 10, 61, 'seeded', PROD_ROUTES, 1234)
    # (seed: of the seeds 1234 .. 1329 two in three leave one to three of conv1's 0.7 M outputs beyond five deviations, i.e. on
    # a clip; this one keeps every activation of both convs 0.2 away from either end)
    add('prod-open', PROD, 10, 61, 'open', (AUTOGRAD,), 1293)
    # batch sizes where the chain changes form: one, two and three batch parts, the d(h)-hand-off boundary at 9, the 16x16
    # boundary at 13 / 17, the two-tile part at 33; odd row counts in every GEMM and BatchNorm of the chain
    # (B = 33's seed: with 333 and 334 the float32 restatement itself flips a clip mask of conv1 and misses the conditioning
    # limit on conv.0.weight / conv.1.bias by a factor of ten)
    for bsz in (1, 5, 9, 13, 17, 33):
        add('B%d' % bsz, WIDE2, bsz, 61, 'seeded', (TRAINER, AUTOGRAD), 335 if bsz == 33 else 300 + bsz)
    # sequence edges: T = 1 (no dW_hh product at all) and T = 2
    add('T1', TINY2, 3, 11, 'seeded', (FB, TRAINER), 21)
    add('T2', TINY2, 3, 13, 'seeded', (FB, TRAINER), 22, label_lens=[2, 1, 0])
    # the per-problem dW_hh route at a well-conditioned small shape, prezeroed both ways (acc_beta 0 and 1)
    add('raw_dw', WIDE2, 10, 61, 'seeded', RAW_ROUTES, 310)
    # one ragged batch, so that the CTC sizes are not all full
    add('ragged', WIDE2, 4, 61, 'seeded', (TRAINER, AUTOGRAD), 77, lengths=[61, 61 - 17, 61 - 40, 51],
        label_lens=[6, 4, 3, 2])
    return out


def case_by_name(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------- inputs
def state_dict_for(case):
    sd = seeded_state_dict(OracleDeepSpeech(**case.kwargs), case.seed)
    if case.regime == 'open':
        for k in ('conv.1', 'conv.4'):
            sd[k + '.weight'] = torch.full_like(sd[k + '.weight'], 2.0)
            sd[k + '.bias'] = torch.full_like(sd[k + '.bias'], 10.0)
    return sd


def inputs_for(case, other=False):
    """(x (B,T_in,161), labels, pct, label sizes) of the case; ``other``: a different batch of the same shape (what the
    trainer route runs first, so that stale sums would show in the second pass)."""
    seed = case.seed + (5000 if other else 0)
    x = torch.from_numpy(seeded_inputs(seed + 1, case.bsz, case.t_in, lengths=case.lengths))
    labels = seeded_labels(seed + 2, case.label_lens, 29)
    off = 0
    for n in case.label_lens:                      # no repeated neighbour: a transcript of n labels needs n frames only
        for i in range(off + 1, off + n):
            if labels[i] == labels[i - 1]:
                labels[i] = 1 + labels[i] % 28
        off += n
    lengths = case.lengths if case.lengths is not None else [case.t_in] * case.bsz
    pct = torch.tensor([n / float(case.t_in) for n in lengths], dtype=torch.float32)
    return x, torch.from_numpy(labels), pct, torch.tensor(case.label_lens, dtype=torch.int32)


def out_sizes_of(pct, t_out):
    return (pct * t_out).int()                     # codes.engine.sanitize_inputs


def family_of(name):
    if name == 'logits':
        return 'logits'
    if name.startswith('buf:'):
        return 'stats'
    top = name.split(':', 1)[1].split('.', 1)[0]
    return {'fc': 'head', 'rnns': 'rnn', 'conv': 'conv'}[top]


def errors(x, r64):
    """(max abs, rms) of x - r64, in float64 on r64's device."""
    e = x.detach().to(r64.device, torch.float64) - r64
    if e.numel() == 0:
        return 0.0, 0.0
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------- reference
def oracle_pass(case, dtype):
    """One training-mode forward and backward pass of the oracle in ``dtype``: {'logits', 'buf:<running stat>', 'grad:<param>'}
    and the clip census of the conv block {'conv1' / 'conv2': (outputs on the lower clip, on the upper, in all)}."""
    model = OracleDeepSpeech(**case.kwargs)
    model.load_state_dict(state_dict_for(case))
    model = model.to(dtype)
    model.train()
    x, labels, pct, sizes = inputs_for(case)
    logits, inter = model(x.to(dtype), return_intermediates=True)
    out_sizes = out_sizes_of(pct, logits.shape[1])
    loss = F.ctc_loss(logits.transpose(0, 1).log_softmax(-1), labels.long(), out_sizes.long(), sizes.long(), blank=0,
                      reduction='sum') / case.bsz
    loss.backward()
    out = {'logits': logits.detach()}
    for k, v in model.state_dict().items():
        if 'running' in k:
            out['buf:' + k] = v.detach().clone()
    for k, p in model.named_parameters():
        out['grad:' + k] = p.grad.detach().clone()
    clip = {k: (int((inter[k] <= 0).sum()), int((inter[k] >= 20).sum()), inter[k].numel()) for k in ('conv1', 'conv2')}
    return out, clip, float(loss.detach())


_refs = {}


def reference(case, dev='cpu'):
    """{'r64': float64 tensors on ``dev``, 'e32': {tensor: (max, rms)} of the float32 restatement, 'amax': {tensor: max|ref|},
    'clip': the float64 pass's clip census, 'loss'}.  Computed once per case and shared by the routes."""
    key = (case.name, str(dev))
    if key not in _refs:
        base = _refs.get((case.name, 'cpu'))
        if base is None:
            r64, clip, loss = oracle_pass(case, torch.float64)
            r32, _, _ = oracle_pass(case, torch.float32)
            base = {'r64': r64, 'e32': {k: errors(r32[k], r64[k]) for k in r64}, 'clip': clip, 'loss': loss,
                    'amax': {k: float(v.abs().max()) for k, v in r64.items()}}
            _refs[(case.name, 'cpu')] = base
        if str(dev) != 'cpu':
            moved = dict(base)
            moved['r64'] = {k: v.to(dev) for k, v in base['r64'].items()}
            _refs[key] = moved
    return _refs[key]


def conditioning(ref):
    """Worst e32 / max|ref| over the held tensors with max|ref| >= CONDITION_FLOOR, and the tensor it belongs to."""
    worst, where = 0.0, None
    for k, (m32, _) in ref['e32'].items():
        if ref['amax'][k] >= CONDITION_FLOOR and m32 / ref['amax'][k] > worst:
            worst, where = m32 / ref['amax'][k], k
    return worst, where


if __name__ == '__main__':                       # the conditioning and clip census of every case, for the profile document
    import time
    for c in cases():
        t0 = time.time()
        ref = reference(c)
        print('%-12s B=%-3d T=%-3d loss %.4f  worst e32 / max|ref| = %.2e (%s)  clip %s  %.1f s'
              % (c.name, c.bsz, conv_out_time(c.t_in), ref['loss'], *conditioning(ref),
                 {k: '%d/%d of %d' % v for k, v in ref['clip'].items()}, time.time() - t0))
