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


def _cut_stats(scores, k):
    """(exact tie at the cut, smallest relative gap) for keeping the k best of ``scores`` (sorted best first): the tie is
    ``scores[k-1] == scores[k]``; the gap is min |s - tau| / max(1, |tau|) over the scores s != tau (inf if none)."""
    tau = scores[k - 1]
    tie = len(scores) > k and scores[k] == tau
    gap = math.inf
    if math.isfinite(tau):
        for s in scores:
            if s != tau:
                gap = min(gap, abs(s - tau) / max(1.0, abs(tau)))
    return tie, gap


def beam_search(lp, blank, beam_width, lm=None, alpha=0.0, beta=0.0, space_id=-1, stats=None):
    """lp: (T, A) list of double log-probs (frame_log_probs).  Returns (labels, offsets, fused score, ctc log p).

    ``stats``: a dict to fill with what the tie tests need.  ``stats['cut']`` gets one ``(tie, gap)`` per frame at which
    more than ``beam_width`` candidates compete (_cut_stats of the ranked scores at the W-th); ``stats['pick']`` the same
    for the final pick of the best entry (k = 1).  A ``gap`` far above the rounding differences of two libms means that
    the selection does not depend on them."""
    A = len(lp[0]) if lp else 0
    L = _Lm(lm, alpha, beta, space_id) if lm is not None else None
    # prefixes are interned: id 0 = the empty prefix, parent[id] and last[id] describe the others
    parent, last_of, child = [-1], [-1], {}
    # beam entries: (prefix id, pb, pnb, lmacc, lm state, born) with born = (frame, born of the parent) or None
    beam = [(0, 0.0, NEG_INF, 0.0, L.start() if L else None, None)]
    if stats is not None:
        stats['cut'] = []
    for t, row in enumerate(lp):
        slot = {e[0]: i for i, e in enumerate(beam)}
        cands = []                                            # (score, index, entry or (slot, symbol, pnb, lmacc, state))
        for i, (pid, pb, pnb, acc, st, born) in enumerate(beam):
            tot = log_add(pb, pnb)
            last = last_of[pid]
            npb = log_add(NEG_INF, tot + row[blank])
            npnb = log_add(NEG_INF, pnb + row[last]) if last >= 0 else NEG_INF
            p = slot.get(parent[pid]) if pid else None
            if p is not None and row[last] > NEG_INF:
                ppid, ppb, ppnb = beam[p][0], beam[p][1], beam[p][2]
                frm = ppb if (ppid and last_of[ppid] == last) else log_add(ppb, ppnb)
                if frm > NEG_INF:
                    npnb = log_add(npnb, frm + row[last])
            cands.append((log_add(npb, npnb) + acc, i * A + blank, (pid, npb, npnb, acc, st, born)))
            for c in range(A):
                if c == blank or row[c] <= NEG_INF or child.get((pid, c)) in slot:
                    continue
                frm = pb if c == last else tot
                if frm <= NEG_INF:
                    continue
                v = frm + row[c]
                nacc, nst = acc, st
                if L is not None:
                    d, nst = L.append(st, c)
                    nacc = acc + d
                cands.append((log_add(NEG_INF, v) + nacc, i * A + c, (i, c, v, nacc, nst)))
        cands.sort(key=lambda x: (-x[0], x[1]))
        if stats is not None and len(cands) > beam_width:
            stats['cut'].append(_cut_stats([x[0] for x in cands], beam_width))
        keep = sorted(cands[:beam_width], key=lambda x: x[1])
        nbeam = []
        for _, _, e in keep:
            if len(e) == 5:                                   # an extension: intern its prefix
                i, c, v, nacc, nst = e
                ppid = beam[i][0]
                pid = child.get((ppid, c))
                if pid is None:
                    pid = child[(ppid, c)] = len(parent)
                    parent.append(ppid)
                    last_of.append(c)
                e = (pid, NEG_INF, v, nacc, nst, (t, beam[i][5]))
            nbeam.append(e)
        beam = nbeam
    best, best_v, best_tot, ends = None, NEG_INF, NEG_INF, []
    for pid, pb, pnb, acc, st, born in beam:
        tot = log_add(pb, pnb)
        v = tot + (L.end(acc, st) if L else 0.0)
        ends.append(v)
        if v > best_v:
            best, best_v, best_tot = (pid, born), v, tot
    if stats is not None:
        stats['pick'] = _cut_stats(sorted(ends, reverse=True), 1)
    if best is None:
        return [], [], -math.inf, -math.inf                  # NEG_INF as the device's float32 outputs
    labels, offsets = [], []
    pid, born = best
    while pid:
        labels.append(last_of[pid])
        offsets.append(born[0])
        pid, born = parent[pid], born[1]
    return labels[::-1], offsets[::-1], best_v, best_tot


def lm_score(lm, labels, alpha, beta, space_id):
    """alpha * LM(l) + beta * N(l) with the end-of-utterance terms, for a whole labelling (the exhaustive test)."""
    L = _Lm(lm, alpha, beta, space_id)
    st, acc = L.start(), 0.0
    for c in labels:
        d, st = L.append(st, c)
        acc = acc + d
    return L.end(acc, st)
