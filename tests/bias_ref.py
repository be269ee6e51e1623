"""Phrase boosting, stated plainly (include/ds2hip.h "phrase boosting"): V and F by the definition, the context graph's
tables by running that definition on every (node, label), and ``beam_ref``'s search with the bias term -- the contract of
``ds2_ctc_beam_search_bias`` (csrc/ctc_beam.hip).  Written for clarity, not speed."""
import math

import numpy as np

from tests.beam_ref import NEG_INF, _cut_stats, _Lm, frame_log_probs, log_add  # noqa: F401  (frame_log_probs: for callers)


def _scan(y, phrases, pending):
    """The leftmost-longest, non-overlapping scan of y -> (count, the pending string it stopped at or ())."""
    y = tuple(y)
    phrases = {tuple(p) for p in phrases}
    nodes = {p[:k] for p in phrases for k in range(len(p) + 1)} | {()}
    i = m = 0
    while i < len(y):
        if pending and y[i:] in nodes:
            return m + len(y) - i, y[i:]
        l = max([len(p) for p in phrases if y[i:i + len(p)] == p], default=0)
        if l > 0:
            m += l
            i += l
        else:
            i += 1
    return m, ()


def V(y, phrases):
    return _scan(y, phrases, True)[0]


def F(y, phrases):
    return _scan(y, phrases, False)[0]


def tables(phrases, n_labels, blank):
    """(paths, next, gain, final): the trie's nodes in BFS order (children in ascending label order, root = 0) and, entry
    by entry from the definition, next[s][c] = the node of the pending string of path(s) + c, gain[s][c] =
    V(path(s) + c) - depth(s), final[s] = F(path(s)) - depth(s).  The blank column holds zeros."""
    phrases = [tuple(p) for p in phrases]
    kids = {}
    for p in phrases:
        for k in range(len(p)):
            kids.setdefault(p[:k], set()).add(p[k])
    paths, head = [()], 0
    while head < len(paths):                                   # breadth first, a queue
        p = paths[head]
        head += 1
        paths.extend(p + (c,) for c in sorted(kids.get(p, ())))
    ident = {p: s for s, p in enumerate(paths)}
    nxt = np.zeros((len(paths), n_labels), np.int32)
    gain = np.zeros((len(paths), n_labels), np.int32)
    final = np.zeros(len(paths), np.int32)
    for s, p in enumerate(paths):
        final[s] = F(p, phrases) - len(p)
        for c in range(n_labels):
            if c != blank:
                v, rest = _scan(p + (c,), phrases, True)
                nxt[s, c], gain[s, c] = ident[rest], v - len(p)
    return paths, nxt, gain, final


def pack(nxt, gain):
    """The (S, A) int32 table the kernel reads: next in the low 16 bits, the signed gain in the high 16."""
    return (np.asarray(nxt, np.int32) | (np.asarray(gain, np.int32) << 16)).astype(np.int32)


def sanitised(trans, n_states):
    """The table as the kernel takes it: a next node outside [0, n_states) is the root; the gain stays."""
    trans = np.asarray(trans, np.int32)
    nxt = trans & 0xFFFF
    return (np.where(nxt < n_states, nxt, 0) | (trans & ~np.int32(0xFFFF))).astype(np.int32)


def beam_search_bias(lp, blank, beam_width, trans, final, weight, lm=None, alpha=0.0, beta=0.0, space_id=-1, stats=None):
    """``beam_ref.beam_search`` with ``w * V(prefix)`` in the rank and ``w * F`` at the end.  trans (S, A) packed and
    final (S) as the kernel reads them (sanitise a malformed table first).  Every beam entry carries (state, count); the
    term is ``w * count``, added after ``log p + acc``; at the end ``w * (count + final[state])`` joins the LM end terms.
    Returns (labels, offsets, fused score, ctc log p, count + final[state] of the labelling); fills ``stats`` as
    ``beam_search`` does."""
    A = len(lp[0]) if lp else 0
    L = _Lm(lm, alpha, beta, space_id) if lm is not None else None
    w = float(np.float32(weight))
    trans = np.asarray(trans, np.int32)
    step = lambda st, cnt, c: (int(trans[st, c]) & 0xFFFF, cnt + (int(trans[st, c]) >> 16))      # noqa: E731
    parent, last_of, child = [-1], [-1], {}
    # beam entries: (prefix id, pb, pnb, lmacc, lm state, born, bias state, bias count)
    beam = [(0, 0.0, NEG_INF, 0.0, L.start() if L else None, None, 0, 0)]
    if stats is not None:
        stats['cut'] = []
    for t, row in enumerate(lp):
        slot = {e[0]: i for i, e in enumerate(beam)}
        cands = []
        for i, (pid, pb, pnb, acc, st, born, bst, bcnt) in enumerate(beam):
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
            cands.append((log_add(npb, npnb) + acc + w * float(bcnt), i * A + blank,
                          (pid, npb, npnb, acc, st, born, bst, bcnt)))
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
                nbst, nbcnt = step(bst, bcnt, c)
                cands.append((log_add(NEG_INF, v) + nacc + w * float(nbcnt), i * A + c, (i, c, v, nacc, nst, nbst, nbcnt)))
        cands.sort(key=lambda x: (-x[0], x[1]))
        if stats is not None and len(cands) > beam_width:
            stats['cut'].append(_cut_stats([x[0] for x in cands], beam_width))
        keep = sorted(cands[:beam_width], key=lambda x: x[1])
        nbeam = []
        for _, _, e in keep:
            if len(e) == 7:                                   # an extension: intern its prefix
                i, c, v, nacc, nst, nbst, nbcnt = e
                ppid = beam[i][0]
                pid = child.get((ppid, c))
                if pid is None:
                    pid = child[(ppid, c)] = len(parent)
                    parent.append(ppid)
                    last_of.append(c)
                e = (pid, NEG_INF, v, nacc, nst, (t, beam[i][5]), nbst, nbcnt)
            nbeam.append(e)
        beam = nbeam
    best, best_v, best_tot, best_f, ends = None, NEG_INF, NEG_INF, 0, []
    for pid, pb, pnb, acc, st, born, bst, bcnt in beam:
        tot = log_add(pb, pnb)
        f = bcnt + int(final[bst])
        v = tot + ((L.end(acc, st) if L else 0.0) + w * float(f))
        ends.append(v)
        if v > best_v:
            best, best_v, best_tot, best_f = (pid, born), v, tot, f
    if stats is not None:
        stats['pick'] = _cut_stats(sorted(ends, reverse=True), 1)
    if best is None:
        return [], [], -math.inf, -math.inf, 0
    labels, offsets = [], []
    pid, born = best
    while pid:
        labels.append(last_of[pid])
        offsets.append(born[0])
        pid, born = parent[pid], born[1]
    return labels[::-1], offsets[::-1], best_v, best_tot, best_f
