"""Oracle: CTC loss and gradient (TEST INFRASTRUCTURE ONLY).

The reference calls ``warpctc_pytorch.CTCLoss()(acts, labels, act_lens,
label_lens)`` (``train.py:12,179``; ``codes/engine.py:22``;
``codes/metrics.py:43,51``).  warp-ctc is an external, un-pinned dependency
(SeanNaren fork cloned at HEAD, ``docker/Dockerfile:54-66``) that is absent from
the reference tree, so this file restates the *published* algorithm (Graves et
al. 2006, as implemented by warp-ctc):

  * acts are UN-normalised (T,B,A) activations; a softmax over A is applied
    inside the loss (reference README.md:168);
  * blank index 0 (``codes/utils/io_utils.py:3,17-25``);
  * labels are a flat 1-D int array of sum(label_lens) entries;
  * the result is the SUM over the batch of -log p(labels | acts) and the
    gradient with respect to the un-normalised acts:
        grad[t,b,k] = softmax[t,b,k] - (1/p_b) * sum_{s: l'_s = k} alpha_t(s) beta_t(s) / y_t(k)
    with zero gradient for frames t >= act_lens[b];
  * an infeasible alignment (label_len + repeats > act_len) gives p = 0: this
    restatement returns cost +inf there like torch's ctc_loss; the reference
    guards the training loop against it at ``codes/engine.py:27-30``.

Pins: ``ctc_brute_force`` enumerates every alignment in float64 for tiny cases;
``ctc_torch`` wraps torch.nn.functional.ctc_loss.  Parity with warp-ctc's own
binary is "unpinned" (it cannot be built here).
"""
import itertools

import numpy as np


def _log_softmax(a):
    m = a.max(axis=-1, keepdims=True)
    e = a - m
    return e - np.log(np.exp(e).sum(axis=-1, keepdims=True))


def ctc_loss_and_grad(acts, labels, act_lens, label_lens, blank=0):
    """float64 alpha/beta CTC.  Returns (costs (B,), grad (T,B,A))."""
    acts = np.asarray(acts, dtype=np.float64)
    t_max, bsz, nalpha = acts.shape
    logp = _log_softmax(acts)
    grad = np.zeros_like(acts)
    costs = np.zeros(bsz, dtype=np.float64)
    off = 0
    neg_inf = -np.inf
    for b in range(bsz):
        tl = int(act_lens[b])
        ll = int(label_lens[b])
        lab = np.asarray(labels[off:off + ll], dtype=np.int64)
        off += ll
        s_len = 2 * ll + 1
        ext = np.full(s_len, blank, dtype=np.int64)
        ext[1::2] = lab
        lp = logp[:tl, b, :]
        alpha = np.full((tl, s_len), neg_inf)
        beta = np.full((tl, s_len), neg_inf)
        if tl == 0:
            costs[b] = 0.0 if ll == 0 else np.inf
            continue
        alpha[0, 0] = lp[0, blank]
        if s_len > 1:
            alpha[0, 1] = lp[0, ext[1]]
        for t in range(1, tl):
            for s in range(s_len):
                terms = [alpha[t - 1, s]]
                if s >= 1:
                    terms.append(alpha[t - 1, s - 1])
                if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                    terms.append(alpha[t - 1, s - 2])
                m = max(terms)
                if m > neg_inf:
                    alpha[t, s] = m + np.log(sum(np.exp(x - m) for x in terms)) + lp[t, ext[s]]
        beta[tl - 1, s_len - 1] = lp[tl - 1, blank]
        if s_len > 1:
            beta[tl - 1, s_len - 2] = lp[tl - 1, ext[s_len - 2]]
        for t in range(tl - 2, -1, -1):
            for s in range(s_len):
                terms = [beta[t + 1, s]]
                if s + 1 < s_len:
                    terms.append(beta[t + 1, s + 1])
                if s + 2 < s_len and ext[s] != blank and ext[s] != ext[s + 2]:
                    terms.append(beta[t + 1, s + 2])
                m = max(terms)
                if m > neg_inf:
                    beta[t, s] = m + np.log(sum(np.exp(x - m) for x in terms)) + lp[t, ext[s]]
        tail = [alpha[tl - 1, s_len - 1]]
        if s_len > 1:
            tail.append(alpha[tl - 1, s_len - 2])
        m = max(tail)
        ll_total = m + np.log(sum(np.exp(x - m) for x in tail)) if m > neg_inf else neg_inf
        costs[b] = -ll_total
        if ll_total == neg_inf:
            continue  # p = 0: gradient left at zero (loss is inf; the caller zeroes it)
        y = np.exp(lp)
        occ = np.zeros((tl, nalpha))
        ab = alpha + beta
        for s in range(s_len):
            finite = ab[:, s] > neg_inf
            occ[finite, ext[s]] += np.exp(ab[finite, s] - ll_total - lp[finite, ext[s]])
        grad[:tl, b, :] = y - occ
    return costs, grad


def _lse_rows(stack):
    """log-sum-exp over axis 0 of (n, S) float64 with -inf entries allowed; all -inf gives -inf."""
    m = stack.max(axis=0)
    safe = np.where(m > -np.inf, m, 0.0)
    with np.errstate(divide='ignore'):
        return np.where(m > -np.inf, safe + np.log(np.exp(stack - safe).sum(axis=0)), -np.inf)


def ctc_loss_and_grad_fast(acts, labels, act_lens, label_lens, blank=0):
    """``ctc_loss_and_grad`` restated with the states of a frame as one numpy vector (one Python loop over t per utterance):
    the same float64 recursion, the same conventions (blank, +inf cost and zero gradient when infeasible, the tl = 0 rule),
    fast enough for training-size batches (T = 746, L = 511 in ~0.05 s).  tests/test_ctc_ref_cpu.py ties it to the loop
    version, to ``ctc_brute_force`` and to torch's ctc_loss in float64."""
    acts = np.asarray(acts, dtype=np.float64)
    t_max, bsz, nalpha = acts.shape
    logp = _log_softmax(acts)
    grad = np.zeros_like(acts)
    costs = np.zeros(bsz, dtype=np.float64)
    off = 0
    neg_inf = -np.inf
    for b in range(bsz):
        tl = int(act_lens[b])
        ll = int(label_lens[b])
        lab = np.asarray(labels[off:off + ll], dtype=np.int64)
        off += ll
        s_len = 2 * ll + 1
        ext = np.full(s_len, blank, dtype=np.int64)
        ext[1::2] = lab
        if tl == 0:
            costs[b] = 0.0 if ll == 0 else np.inf
            continue
        lp = logp[:tl, b, :]
        em = lp[:, ext]                                                   # (tl, S): log p of each state's symbol
        skip = np.zeros(s_len, dtype=bool)                                # state s may be entered from s - 2
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        skip_b = np.zeros(s_len, dtype=bool)                              # state s may be entered from s + 2 (beta)
        skip_b[:-2] = (ext[:-2] != blank) & (ext[:-2] != ext[2:])
        alpha = np.full((tl, s_len), neg_inf)
        beta = np.full((tl, s_len), neg_inf)
        alpha[0, :2] = em[0, :2]
        stack = np.full((3, s_len), neg_inf)
        for t in range(1, tl):
            prev = alpha[t - 1]
            stack[0] = prev
            stack[1, 1:] = prev[:-1]
            stack[2, 2:] = np.where(skip[2:], prev[:-2], neg_inf)
            alpha[t] = _lse_rows(stack) + em[t]
        beta[tl - 1, -2:] = em[tl - 1, -2:]
        stack = np.full((3, s_len), neg_inf)
        for t in range(tl - 2, -1, -1):
            nxt = beta[t + 1]
            stack[0] = nxt
            stack[1, :-1] = nxt[1:]
            stack[2, :-2] = np.where(skip_b[:-2], nxt[2:], neg_inf)
            beta[t] = _lse_rows(stack) + em[t]
        ll_total = float(_lse_rows(alpha[tl - 1, -2:].reshape(-1, 1))[0])
        costs[b] = -ll_total
        if ll_total == neg_inf:
            continue
        ab = alpha + beta
        with np.errstate(invalid='ignore'):
            post = np.where(ab > neg_inf, np.exp(ab - ll_total - em), 0.0)   # (tl, S)
        occ = np.zeros((tl, nalpha))
        for k in np.unique(ext):
            occ[:, k] = post[:, ext == k].sum(axis=1)
        grad[:tl, b, :] = np.exp(lp) - occ
    return costs, grad


def ctc_brute_force(acts_tb, label, blank=0):
    """-log p(label | acts) by enumerating every length-T path (tiny T, A only)."""
    acts_tb = np.asarray(acts_tb, dtype=np.float64)
    t_len, nalpha = acts_tb.shape
    p = np.exp(_log_softmax(acts_tb))
    total = 0.0
    label = list(label)
    for path in itertools.product(range(nalpha), repeat=t_len):
        collapsed = []
        prev = None
        for c in path:
            if c != prev and c != blank:
                collapsed.append(c)
            prev = c
        if collapsed == label:
            total += np.prod([p[t, c] for t, c in enumerate(path)])
    return -np.log(total) if total > 0 else np.inf


def ctc_torch(acts, labels, act_lens, label_lens, blank=0):
    """Sum-reduced CTC on un-normalised acts via torch CPU; returns (loss, grad)."""
    import torch
    import torch.nn.functional as F
    a = torch.as_tensor(np.asarray(acts), dtype=torch.float32).clone().requires_grad_(True)
    loss = F.ctc_loss(a.log_softmax(-1), torch.as_tensor(np.asarray(labels), dtype=torch.long),
                      torch.as_tensor(np.asarray(act_lens), dtype=torch.long),
                      torch.as_tensor(np.asarray(label_lens), dtype=torch.long),
                      blank=blank, reduction='sum', zero_infinity=False)
    loss.backward()
    return float(loss.item()), a.grad.numpy()
