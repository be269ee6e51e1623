"""Pure-Python CTC prefix beam search with n-gram LM fusion: the contract of the device search
(``ds2_ctc_beam_search_batch``, csrc/ctc_beam.hip), written for clarity, not speed.

Per frame every beam prefix proposes its stay (blank, or a repeat of its last symbol) and its extensions; an extension
that reaches a prefix already in the beam is merged into that prefix's stay.  The candidates are ranked by
``log(p_b + p_nb) + alpha * LM + beta * N``; ties go to the lower candidate index ``i * A + c`` (beam slot ``i``,
symbol ``c``; the stay of slot ``i`` is ``i * A + blank``), and the new beam is kept in candidate-index order.
"""
import math

import numpy as np

NEG_INF = -1e300


def log_add(x, y):
    if x <= NEG_INF:
        return y
    if y <= NEG_INF:
        return x
    m = x if x > y else y
    return m + math.log1p(math.exp(-abs(x - y)))


def frame_log_probs(probs, log_input):
    """(T, A) float32 -> list of lists of doubles, as the host and the device search convert them."""
    out = []
    for row in np.asarray(probs, dtype=np.float32):
        if log_input:
            out.append([float(v) for v in row])
        else:
            out.append([math.log(float(v)) if v > 0 else NEG_INF for v in row])
    return out


class _Lm(object):
    """The LM part of a prefix's state and its updates (mirrors lm_delta / lm_end in csrc/ctc_beam.hip)."""

    def __init__(self, lm, alpha, beta, space_id):
        self.lm, self.space_id = lm, space_id
        self.alpha = float(np.float32(alpha))
        self.beta = float(np.float32(beta))

    def start(self):
        return ((self.lm.bos_id,) if self.lm.order > 1 else (), ())

    def _push(self, ctx, tok):
        if self.lm.order == 1:
            return ()
        ctx = ctx + (tok,)
        return ctx[len(ctx) - (self.lm.order - 1):] if len(ctx) > self.lm.order - 1 else ctx

    def _word(self, ctx, chars):
        lp, tok = self.lm.log_prob_ids(ctx, self.lm.word_id(list(chars)))
        return self.alpha * lp + self.beta, self._push(ctx, tok)

    def append(self, state, c):
        """-> (delta, new state) for appending label c."""
        ctx, chars = state
        if self.lm.unit == 'char':
            lp, tok = self.lm.log_prob_ids(ctx, c)
            return self.alpha * lp + self.beta, (self._push(ctx, tok), ())
        if c == self.space_id:
            if not chars:
                return 0.0, (ctx, ())
            d, ctx = self._word(ctx, chars)
            return d, (ctx, ())
        return 0.0, (ctx, chars + (c,))

    def end(self, lmacc, state):
        ctx, chars = state
        e = lmacc
        if self.lm.unit == 'word' and chars:
            d, ctx = self._word(ctx, chars)
            e = e + d
        lp, _ = self.lm.log_prob_ids(ctx, self.lm.eos_id)
        return e + self.alpha * lp


def beam_search(lp, blank, beam_width, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    """lp: (T, A) list of double log-probs (frame_log_probs).  Returns (labels, offsets, fused score, ctc log p)."""
    A = len(lp[0]) if lp else 0
    L = _Lm(lm, alpha, beta, space_id) if lm is not None else None
    # beam entries: [prefix tuple, pb, pnb, lmacc, lm state, born tuple]
    beam = [[(), 0.0, NEG_INF, 0.0, L.start() if L else None, ()]]
    for t, row in enumerate(lp):
        slot = {b[0]: i for i, b in enumerate(beam)}
        cands = []                                            # (score, index, entry)
        for i, (pre, pb, pnb, acc, st, born) in enumerate(beam):
            tot = log_add(pb, pnb)
            last = pre[-1] if pre else -1
            npb = log_add(NEG_INF, tot + row[blank])
            npnb = log_add(NEG_INF, pnb + row[last]) if last >= 0 else NEG_INF
            p = slot.get(pre[:-1]) if pre else None
            if p is not None and row[last] > NEG_INF:
                ppre, ppb, ppnb = beam[p][0], beam[p][1], beam[p][2]
                frm = ppb if (ppre and ppre[-1] == last) else log_add(ppb, ppnb)
                if frm > NEG_INF:
                    npnb = log_add(npnb, frm + row[last])
            cands.append((log_add(npb, npnb) + acc, i * A + blank, [pre, npb, npnb, acc, st, born]))
            for c in range(A):
                if c == blank or row[c] <= NEG_INF or (pre + (c,)) in slot:
                    continue
                frm = pb if c == last else tot
                if frm <= NEG_INF:
                    continue
                v = frm + row[c]
                nacc, nst = acc, st
                if L is not None:
                    d, nst = L.append(st, c)
                    nacc = acc + d
                cands.append((log_add(NEG_INF, v) + nacc, i * A + c, [pre + (c,), NEG_INF, v, nacc, nst, born + (t,)]))
        cands.sort(key=lambda x: (-x[0], x[1]))
        keep = sorted(cands[:beam_width], key=lambda x: x[1])
        beam = [e for _, _, e in keep]
    best, best_v, best_tot = None, NEG_INF, NEG_INF
    for pre, pb, pnb, acc, st, born in beam:
        tot = log_add(pb, pnb)
        v = tot + (L.end(acc, st) if L else 0.0)
        if v > best_v:
            best, best_v, best_tot = (pre, born), v, tot
    if best is None:
        return [], [], float(np.float32(NEG_INF)), float(np.float32(NEG_INF))
    return list(best[0]), list(best[1]), best_v, best_tot


def lm_score(lm, labels, alpha, beta, space_id):
    """alpha * LM(l) + beta * N(l) with the end-of-utterance terms, for a whole labelling (the exhaustive test)."""
    L = _Lm(lm, alpha, beta, space_id)
    st, acc = L.start(), 0.0
    for c in labels:
        d, st = L.append(st, c)
        acc = acc + d
    return L.end(acc, st)
