"""Float64 statement of ``ds2_ctc_mwer_grad`` (include/ds2hip.h "MWER"): TEST INFRASTRUCTURE ONLY, no GPU in here.

Built on ``oracle.ctc.ctc_loss_and_grad_fast``: each label row of an utterance (its hypotheses, then its reference) is run
as a batch of one over that utterance's column of acts; the rows' costs give the posteriors, the expected risk and the row
weights; the gradient is the weighted sum of the rows' own CTC gradients.  The rules are the header's:
  a row of infinite cost has P = 0 and no gradient; a row longer than ``max_label_len`` is dropped (counted, P = 0);
  no finite row: E = 0 and only the CTC term; an infeasible reference: no gradient from that utterance at all;
  ``zero_batch_if_inf``: an infeasible reference zeroes the whole batch's gradient; frames at or past act_lens get 0.
"""
import numpy as np

from oracle import ctc as octc


def row_cost_and_grad(acts_b, tl, lab):
    """(-log p, d(-log p)/d acts (T,A)) of one label row on one utterance's (T,A) activations; (+inf, 0) when infeasible."""
    t_max, nalpha = acts_b.shape
    tl = max(min(int(tl), t_max), 0)
    lab = np.asarray(lab, dtype=np.int32).reshape(-1)
    a = np.zeros((t_max, 1, nalpha), dtype=np.float64)
    a[:tl, 0] = np.asarray(acts_b, dtype=np.float64)[:tl]          # what lies past tl (NaN included) is not looked at
    cost, grad = octc.ctc_loss_and_grad_fast(a, lab, np.array([tl]), np.array([len(lab)]))
    g = np.array(grad[:, 0], dtype=np.float64)
    g[tl:] = 0.0
    if not np.isfinite(cost[0]):
        return np.inf, np.zeros_like(g)
    return float(cost[0]), g


def mwer(acts, act_lens, hyps, risks, refs, ctc_weight=0.0, grad_scale=1.0, zero_batch_if_inf=False, max_label_len=None):
    """acts (T,B,A); hyps[b] a list of label sequences, risks[b] their risks, refs[b] the reference.  Returns a dict of
    float64 arrays / lists: hyp_costs[b] (list), ref_costs (B,), posterior[b] (list), exp_risk (B,), loss (B,), dropped (B,),
    weights[b] (the w_n, zeros where the reference is infeasible) and grad (T,B,A)."""
    acts = np.asarray(acts)
    t_max, bsz, nalpha = acts.shape
    out = {'hyp_costs': [], 'posterior': [], 'weights': [], 'ref_costs': np.zeros(bsz), 'exp_risk': np.zeros(bsz),
           'loss': np.zeros(bsz), 'dropped': np.zeros(bsz, dtype=np.int64), 'grad': np.zeros((t_max, bsz, nalpha))}
    for b in range(bsz):
        col = acts[:, b]
        costs, grads = [], []
        for lab in hyps[b]:
            if max_label_len is not None and len(lab) > max_label_len:
                out['dropped'][b] += 1
                c, g = np.inf, None
            else:
                c, g = row_cost_and_grad(col, act_lens[b], lab)
            costs.append(c)
            grads.append(g)
        costs = np.array(costs, dtype=np.float64).reshape(-1)
        w_risk = np.array(risks[b], dtype=np.float64).reshape(-1)[:len(costs)]
        finite = np.isfinite(costs)
        post = np.zeros(len(costs))
        if finite.any():
            ll = -costs[finite]
            e = np.exp(ll - ll.max())
            post[finite] = e / e.sum()
        exp_risk = float(np.sum(post[finite] * w_risk[finite])) if finite.any() else 0.0
        c_ref, g_ref = row_cost_and_grad(col, act_lens[b], refs[b])
        if max_label_len is not None and len(refs[b]) > max_label_len:
            c_ref, g_ref = np.inf, np.zeros_like(g_ref)
        w = np.zeros(len(costs))
        if np.isfinite(c_ref):
            w[finite] = -post[finite] * (w_risk[finite] - exp_risk)
            g = ctc_weight * g_ref
            for n in np.nonzero(finite)[0]:
                g = g + w[n] * grads[n]
            out['grad'][:, b] = grad_scale * g
        out['hyp_costs'].append(costs)
        out['posterior'].append(post)
        out['weights'].append(w)
        out['ref_costs'][b] = c_ref
        out['exp_risk'][b] = exp_risk
        out['loss'][b] = exp_risk + (ctc_weight * c_ref if ctc_weight != 0.0 else 0.0)
    if zero_batch_if_inf and not np.all(np.isfinite(out['ref_costs'])):
        out['grad'][:] = 0.0
    return out


def expected_risk(acts, act_lens, hyps, risks):
    """The expected risk (B,) alone: what the descent test looks at."""
    acts = np.asarray(acts)
    refs = [np.zeros(0, np.int32)] * acts.shape[1]
    return mwer(acts, act_lens, hyps, risks, refs)['exp_risk']


def grad_condition(res, b, risks_b, ctc_weight, tl, family_bounds):
    """The issue's derived condition for utterance b: |dgrad| / grad_scale <= S_w * G + 2 * dW * (2 * C), with G the CTC
    gradient bound, C = cost_per_frame * tl the CTC cost bound, S_w = ctc_weight + sum_n P_n |W_n - E| and dW the spread of
    the utterance's risks (over its rows of finite cost)."""
    post, costs = res['posterior'][b], res['hyp_costs'][b]
    finite = np.isfinite(costs)
    w_risk = np.asarray(risks_b, dtype=np.float64)[:len(costs)]
    s_w = ctc_weight + float(np.sum(post[finite] * np.abs(w_risk[finite] - res['exp_risk'][b])))
    spread = float(w_risk[finite].max() - w_risk[finite].min()) if finite.any() else 0.0
    return s_w * family_bounds['grad_max'] + 2.0 * spread * (2.0 * family_bounds['cost_per_frame'] * max(int(tl), 1))
