"""N-best lists, stated plainly (include/ds2hip.h ``ds2_ctc_beam_search_nbest``): the loop of ``bias_ref.beam_search_bias``
frame by frame -- with no graph, the root-only one, which adds ``0.0 * 0`` and so leaves ``beam_ref.beam_search`` -- and at
the end the valid entries of the final beam ranked by their end-adjusted score, each traced back on its own lineage.
Written for clarity, not speed."""
import numpy as np

from tests.beam_ref import NEG_INF, _cut_stats, _Lm, log_add


def beam_search_nbest(lp, blank, beam_width, nbest, trans=None, final=None, weight=0.0, lm=None, alpha=0.0, beta=0.0,
                      space_id=-1, stats=None):
    """lp: (T, A) list of double log-probs.  Returns ``(rows, count)``: ``rows[n] = (labels, offsets, fused score, ctc log p,
    count + final[state])`` for n < count = min(nbest, valid entries), best first; an entry is valid if its end-adjusted
    score v > -1e300; a higher v comes first and an exact tie goes to the lower slot.  ``stats['cut']`` as
    ``beam_ref.beam_search``; ``stats['rank']`` = ``_cut_stats`` of the ranked valid end scores at every k = 1 .. count."""
    A = len(lp[0]) if lp else 0
    L = _Lm(lm, alpha, beta, space_id) if lm is not None else None
    if trans is None:
        trans, final, weight = np.zeros((1, max(A, 1)), np.int32), np.zeros(1, np.int32), 0.0
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
    # the end: every slot's end-adjusted score, the valid ones ranked (sorted() is stable: a tie keeps the slot order)
    valid = []
    for pid, pb, pnb, acc, st, born, bst, bcnt in beam:
        tot = log_add(pb, pnb)
        f = bcnt + int(final[bst])
        v = tot + ((L.end(acc, st) if L else 0.0) + w * float(f))
        if v > NEG_INF:
            valid.append((v, tot, f, pid, born))
    ranked = sorted(valid, key=lambda e: -e[0])
    count = min(nbest, len(ranked))
    if stats is not None:
        stats['rank'] = [_cut_stats([e[0] for e in ranked], k) for k in range(1, count + 1)]
    rows = []
    for v, tot, f, pid, born in ranked[:count]:
        labels, offsets = [], []
        while pid:
            labels.append(last_of[pid])
            offsets.append(born[0])
            pid, born = parent[pid], born[1]
        rows.append((labels[::-1], offsets[::-1], v, tot, f))
    return rows, count
