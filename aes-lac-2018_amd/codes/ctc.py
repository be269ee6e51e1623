"""CTC criterion with the warp-ctc call signature the reference uses.

Reference call sites: ``train.py:12,179`` (``from warpctc_pytorch import CTCLoss``), ``codes/engine.py:22``
``criterion(out, targets, out_sizes, target_sizes)`` and ``codes/metrics.py:43,51``.  Contract kept:
  acts (T,B,A) un-normalised device activations (softmax applied inside), labels 1-D int32 (CPU or device),
  act_lens / label_lens int32 (B) (CPU or device)  ->  1-element tensor = SUM over the batch of -log p,
  differentiable w.r.t. acts only, blank = 0.
The arithmetic is ``ds2_ctc_loss_grad`` (csrc/ctc.hip); the gradient is produced in the same pass and
handed to autograd in backward.  An infeasible utterance contributes +inf (and, like warp-ctc, no gradient of its
own); the trainer then applies ``codes/engine.py:24-30``: the batch loss becomes ``0 * loss``, i.e. the value is
reported as 0 and the WHOLE batch's gradient is zero (``zero_batch_if_inf`` does that inside the gradient kernel
for the fused step; the autograd path gets it from the 0 factor).

``mwer_costs_and_grad`` / ``MWERLoss`` (not in the reference): the minimum-word-error-rate loss over the device N-best list
with the same call shapes (``ds2_ctc_mwer_grad``, csrc/ctc_mwer.hip; README "MWER fine-tuning").
"""
import torch

from ds2hip import ops


def ctc_costs_and_grad(acts, labels, act_lens, label_lens, grad_scale=1.0, zero_batch_if_inf=False):
    """Raw kernel call: returns (costs (B,), grad (T,B,A)) on the device of ``acts``.

    The four small integer arrays the warp-ctc signature passes on the host (labels, lengths) travel to the
    device in ONE upload through a reusable pinned staging buffer."""
    dev = acts.device
    label_lens_c = torch.as_tensor(label_lens).to('cpu', torch.int32).reshape(-1)
    act_lens_c = torch.as_tensor(act_lens).to('cpu', torch.int32).reshape(-1)
    labels_c = torch.as_tensor(labels).to('cpu', torch.int32).reshape(-1)
    bsz = label_lens_c.numel()
    max_len = int(label_lens_c.max().item()) if bsz else 0
    # the kernels index acts and their LDS rows with these values and cannot check them on the device: refuse here
    if acts.dim() != 3 or bsz != acts.shape[1] or act_lens_c.numel() != bsz:
        raise ValueError('ctc: acts must be (T, B, A) with B = %d lengths; got acts %s, %d act_lens'
                         % (bsz, tuple(acts.shape), act_lens_c.numel()))
    if bsz and (int(label_lens_c.min()) < 0 or int(label_lens_c.sum()) > labels_c.numel()):
        raise ValueError('ctc: label_lens must be >= 0 and sum to no more than the %d labels given' % labels_c.numel())
    if labels_c.numel() and not (0 <= int(labels_c.min()) and int(labels_c.max()) < acts.shape[2]):
        raise ValueError('ctc: labels must lie in 0 .. %d (the alphabet of acts)' % (acts.shape[2] - 1))
    nlab = max(int(labels_c.numel()), 1)
    packed = torch.zeros(nlab + 3 * bsz, dtype=torch.int32)
    packed[:labels_c.numel()] = labels_c
    if bsz > 1:
        packed[nlab + 1:nlab + bsz] = torch.cumsum(label_lens_c, 0)[:-1]          # start of each utterance's labels
    packed[nlab + bsz:nlab + 2 * bsz] = label_lens_c
    packed[nlab + 2 * bsz:] = act_lens_c
    d = ops.upload_small(packed, dev)
    return ops.ctc_loss_grad(acts.contiguous().float(), d[:nlab], d[nlab:nlab + bsz], d[nlab + bsz:nlab + 2 * bsz],
                             d[nlab + 2 * bsz:], max_len, grad_scale, zero_batch_if_inf)


MWER_KEYS = ('nbest', 'beam_width', 'ctc_weight', 'risk')
MWER_MAX_LABEL_LEN = 511                 # ds2_ctc_mwer_grad's (and ds2_ctc_loss_grad's) longest label row


def mwer_costs_and_grad(acts, targets, act_lens, target_sizes, space_id, nbest=4, beam_width=8, ctc_weight=0.01,
                        risk='word', grad_scale=1.0, zero_batch_if_inf=False, max_workspace_gb=4):
    """Minimum-word-error-rate loss of a minibatch and its gradient (include/ds2hip.h "MWER"; README "MWER fine-tuning").

    acts (T,B,A) un-normalised device activations; targets, act_lens, target_sizes as for ``ctc_costs_and_grad`` (one
    ``upload_small``, the same host-side refusals).  On the device, in stream order: ``ops.softmax_rows`` -> (B,T,A) ->
    ``ops.ctc_beam_search_nbest`` (no LM, no boost) -> ``ops.edit_stats`` of every row against its utterance's reference (the
    word or the character distance is the row's risk) -> ``ops.ctc_mwer_grad``.

    Returns ``(loss (B,), grad (T,B,A), info)``: loss_b = expected risk + ctc_weight * reference CTC cost, grad =
    grad_scale * d(sum_b loss_b)/d acts, and ``info`` the device tensors ``exp_risk``, ``ref_costs``, ``posterior``, ``count``
    and ``dropped`` (and the search's ``hyp`` (B,N,T), ``hyp_len`` and the rows' ``risk``).  ONE small readback per call: the largest hypothesis length, which sizes ``max_label_len`` (and with it
    the workspace) -- the host waits for the search there.  A workspace above ``max_workspace_gb`` is refused with the size
    it would need."""
    if risk not in ('word', 'char'):
        raise ValueError('mwer: risk must be \'word\' or \'char\', got %r' % (risk,))
    if risk == 'word' and int(space_id) < 0:
        raise ValueError('mwer: risk = \'word\' needs the label of the space (space_id); this alphabet has none')
    nbest, beam_width = int(nbest), int(beam_width)
    if not 1 <= beam_width <= ops.MWER_MAX_NBEST or not 1 <= nbest <= beam_width:
        raise ValueError('mwer: beam_width must lie in 1..%d and nbest in 1..beam_width; got nbest %d, beam_width %d'
                         % (ops.MWER_MAX_NBEST, nbest, beam_width))
    dev = acts.device
    label_lens_c = torch.as_tensor(target_sizes).to('cpu', torch.int32).reshape(-1)
    act_lens_c = torch.as_tensor(act_lens).to('cpu', torch.int32).reshape(-1)
    labels_c = torch.as_tensor(targets).to('cpu', torch.int32).reshape(-1)
    bsz = label_lens_c.numel()
    max_ref = int(label_lens_c.max().item()) if bsz else 0
    if acts.dim() != 3 or bsz != acts.shape[1] or act_lens_c.numel() != bsz or bsz == 0:
        raise ValueError('mwer: acts must be (T, B, A) with B = %d lengths; got acts %s, %d act_lens'
                         % (bsz, tuple(acts.shape), act_lens_c.numel()))
    if int(label_lens_c.min()) < 0 or int(label_lens_c.sum()) > labels_c.numel():
        raise ValueError('mwer: label_lens must be >= 0 and sum to no more than the %d labels given' % labels_c.numel())
    if labels_c.numel() and not (0 <= int(labels_c.min()) and int(labels_c.max()) < acts.shape[2]):
        raise ValueError('mwer: labels must lie in 0 .. %d (the alphabet of acts)' % (acts.shape[2] - 1))
    if max_ref > MWER_MAX_LABEL_LEN:
        raise ValueError('mwer: a reference of %d labels; the kernels take up to %d' % (max_ref, MWER_MAX_LABEL_LEN))
    t, _, a = acts.shape
    nlab = max(int(labels_c.numel()), 1)
    # labels | offsets (B) | label_lens (B) | act_lens clamped to T (B) | the reference of each of the B*N rows
    packed = torch.zeros(nlab + 3 * bsz + bsz * nbest, dtype=torch.int32)
    packed[:labels_c.numel()] = labels_c
    if bsz > 1:
        packed[nlab + 1:nlab + bsz] = torch.cumsum(label_lens_c, 0)[:-1]
    packed[nlab + bsz:nlab + 2 * bsz] = label_lens_c
    packed[nlab + 2 * bsz:nlab + 3 * bsz] = act_lens_c.clamp(0, t)
    packed[nlab + 3 * bsz:] = torch.arange(bsz, dtype=torch.int32).repeat_interleave(nbest)
    d = ops.upload_small(packed, dev)
    ref, offs, lens = d[:nlab], d[nlab:nlab + bsz], d[nlab + bsz:nlab + 2 * bsz]
    sizes, ref_index = d[nlab + 2 * bsz:nlab + 3 * bsz], d[nlab + 3 * bsz:]
    acts = acts.contiguous().float()
    probs = ops.softmax_rows(acts, t * bsz, a).transpose(0, 1).contiguous()                 # (B,T,A)
    hyp, _, hyp_len, _, _, _, count = ops.ctc_beam_search_nbest(probs, sizes, beam_width, nbest)
    stats = ops.edit_stats(hyp.view(bsz * nbest, t), hyp_len.view(-1), ref, offs, lens, max_ref, int(space_id),
                           ref_index=ref_index)
    col = ops.EDIT_FIELDS.index('word_dist' if risk == 'word' else 'char_dist')
    risks = stats[:, col].to(torch.float32).view(bsz, nbest).contiguous()
    max_hyp = int(hyp_len.max().item())                        # the call's one readback (rows past the count have length 0)
    max_len = min(max(max_ref, max_hyp), MWER_MAX_LABEL_LEN)   # (a longer hypothesis is dropped by the kernel and counted)
    need = ops.ctc_mwer_ws_bytes(t, bsz, a, nbest, max_len)
    if need > float(max_workspace_gb) * (1 << 30):
        raise RuntimeError('mwer: the workspace for T = %d, B = %d, nbest = %d, %d labels is %d bytes (%.2f GiB), above '
                           'max_workspace_gb = %s: lower nbest or the batch size' % (t, bsz, nbest, max_len, need,
                                                                                     need / float(1 << 30), max_workspace_gb))
    ref_costs, _, posterior, exp_risk, dropped, grad = ops.ctc_mwer_grad(
        acts, sizes, hyp, hyp_len, count, risks, ref, offs, lens, max_len, ctc_weight, grad_scale, zero_batch_if_inf)
    loss = exp_risk + float(ctc_weight) * ref_costs if float(ctc_weight) != 0.0 else exp_risk
    return loss, grad, dict(exp_risk=exp_risk, ref_costs=ref_costs, posterior=posterior, count=count, dropped=dropped,
                            hyp=hyp, hyp_len=hyp_len, risk=risks)


class _MWERFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, labels, act_lens, label_lens, module):
        loss, grad, info = mwer_costs_and_grad(acts, labels, act_lens, label_lens, module.space_id, **module.kwargs)
        module.last_info = info
        ctx.save_for_backward(grad)
        return loss.sum().reshape(1)

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output.reshape(1, 1, 1), None, None, None, None


class MWERLoss(torch.nn.Module):
    """``CTCLoss``'s call signature with the MWER loss behind it: the SUM over the batch of loss_b, differentiable w.r.t.
    acts only; the gradient is produced in the same pass and handed to autograd in backward.  Keywords as
    ``mwer_costs_and_grad`` (nbest, beam_width, ctc_weight, risk, max_workspace_gb); ``last_info`` holds the last call's
    device tensors (``exp_risk``, ...)."""

    def __init__(self, space_id, **kwargs):
        super().__init__()
        unknown = sorted(set(kwargs) - set(MWER_KEYS) - {'max_workspace_gb'})
        if unknown:
            raise ValueError('MWERLoss: unknown keyword(s) %s; it takes %s' % (', '.join(unknown), ', '.join(MWER_KEYS)))
        self.space_id, self.kwargs, self.last_info = int(space_id), dict(kwargs), None

    def forward(self, acts, labels, act_lens, label_lens):
        return _MWERFunction.apply(acts, labels, act_lens, label_lens, self)


class _CTCFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, labels, act_lens, label_lens):
        costs, grad = ctc_costs_and_grad(acts, labels, act_lens, label_lens)
        ctx.save_for_backward(grad)
        return costs.sum().reshape(1)

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output.reshape(1, 1, 1), None, None, None


class CTCLoss(torch.nn.Module):
    """Drop-in for ``warpctc_pytorch.CTCLoss()`` as used by the reference."""

    def forward(self, acts, labels, act_lens, label_lens):
        return _CTCFunction.apply(acts, labels, act_lens, label_lens)
