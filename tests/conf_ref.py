"""The definition of ds2_ctc_unit_posterior (include/ds2hip.h, "unit posterior") in plain Python: unit finding, row
validation, spans, and the linear CTC forward with power-of-two rescaling in float64 -- plus an exact variant on
fractions.Fraction and a brute-force enumeration of alignments.  No GPU, no library."""
import itertools
import math
from fractions import Fraction

import numpy as np

MAX_LABELS = 64          # DS2_UNIT_MAX_LABELS


def find_units(labels, space_id):
    """[(first, length)] in row order.  space_id >= 0: the maximal runs of labels other than space_id; -1: every label."""
    labels = [int(c) for c in labels]
    if space_id < 0:
        return [(i, 1) for i in range(len(labels))]
    units, start = [], None
    for i, c in enumerate(labels + [space_id]):
        if c == space_id:
            if start is not None:
                units.append((start, i - start))
            start = None
        elif start is None:
            start = i
    return units


def row_valid(labels, offsets, length, stride, utt, n_utt, sizes, t_max, n_alpha, blank):
    """The device's row check: lens in 0..stride, utt in [0, B), labels in [0, A) and not blank, offsets strictly increasing
    inside [0, min(sizes[utt], T))."""
    if not 0 <= length <= stride or not 0 <= utt < n_utt:
        return False
    lim = min(max(int(sizes[utt]), 0), t_max)
    prev = -1
    for c, o in zip(labels[:length], offsets[:length]):
        c, o = int(c), int(o)
        if not 0 <= c < n_alpha or c == blank or o <= prev or o >= lim:
            return False
        prev = o
    return True


def _clean(p, exact):
    if exact:
        return Fraction(float(p)) if p == p and p > 0 else Fraction(0)
    p = float(p)
    return p if p > 0.0 else 0.0            # NaN and negative count as 0


def forward(span, unit, blank, exact=False):
    """span: (n, A) probabilities of the unit's frames; unit: its labels.  Returns ln P as a float (-inf for P = 0) -- or,
    with ``exact``, P itself as a Fraction.  The float64 form rescales all alphas by the power of two of their maximum
    whenever it leaves 2^-200 .. 2^200 and sums the exponent."""
    ext = [blank]
    for c in unit:
        ext += [int(c), blank]
    n_states = len(ext)
    zero = Fraction(0) if exact else 0.0
    alpha = [zero] * n_states
    alpha[0] = Fraction(1) if exact else 1.0        # before the first frame: all mass in the leading blank
    e2 = 0
    for t in range(len(span)):
        new = [zero] * n_states
        for s in range(n_states):
            acc = alpha[s]
            if s >= 1:
                acc = acc + alpha[s - 1]
            if s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2]:
                acc = acc + alpha[s - 2]
            new[s] = _clean(span[t][ext[s]], exact) * acc
        alpha = new
        if not exact:
            top = max(alpha)
            if top > 0.0 and math.isfinite(top) and not 2.0 ** -200 <= top <= 2.0 ** 200:
                e = math.frexp(top)[1] - 1
                alpha = [math.ldexp(a, -e) for a in alpha]
                e2 += e
    total = alpha[-1] + alpha[-2]
    if exact:
        return total
    return (math.log(total) if total > 0.0 else -math.inf) + e2 * math.log(2.0)


def brute_force(span, unit, blank):
    """P by enumeration of every alignment of the span's frames (Fractions): collapse repeats, drop blanks, compare."""
    n, n_alpha = len(span), len(span[0])
    want, total = [int(c) for c in unit], Fraction(0)
    for path in itertools.product(range(n_alpha), repeat=n):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if out == want:
            w = Fraction(1)
            for t, c in enumerate(path):
                w *= _clean(span[t][c], True)
            total += w
    return total


def unit_posterior(probs, sizes, labels, offsets, lens, utt=None, space_id=-1, blank=0, max_units=None, exact=False):
    """The entry point's outputs as numpy arrays: unit_first, unit_len (R,max_units) int32, unit_logp (R,max_units)
    float64, n_units, dropped (R,) int32.  With ``exact`` the values are ln of the exact P (for inputs whose P is a double)."""
    probs = np.asarray(probs)
    n_utt, t_max, n_alpha = probs.shape
    labels, offsets = np.asarray(labels), np.asarray(offsets)
    rows, stride = labels.shape
    if max_units is None:
        max_units = stride if space_id < 0 else (stride + 1) // 2
    first = np.full((rows, max_units), -1, np.int32)
    length = np.full((rows, max_units), -1, np.int32)
    logp = np.full((rows, max_units), np.nan, np.float64)
    n_units, dropped = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    for r in range(rows):
        u = r if utt is None else int(utt[r])
        n = int(lens[r])
        if not row_valid(labels[r], offsets[r], n, stride, u, n_utt, sizes, t_max, n_alpha, blank):
            n_units[r] = -1
            continue
        units = find_units(labels[r, :n], space_id)
        n_units[r] = len(units)
        dropped[r] = sum(1 for _, ln in units if ln > MAX_LABELS)
        for k, (i, ln) in enumerate(units[:max_units]):
            first[r, k], length[r, k] = i, ln
            if ln > MAX_LABELS:
                continue
            span = probs[u, int(offsets[r, i]):int(offsets[r, i + ln - 1]) + 1]
            if exact:
                p = forward(span, labels[r, i:i + ln], blank, exact=True)
                assert Fraction(float(p)) == p, 'P is not a double'
                logp[r, k] = math.log(float(p)) if p > 0 else -math.inf
            else:
                logp[r, k] = forward(span, labels[r, i:i + ln], blank)
    return first, length, logp, n_units, dropped


def bound(n_frames, logp):
    """|dlogp| between two float64 evaluations: three roundings per frame on non-negative terms, on either side, and the
    final logarithm and exponent sum."""
    mag = max(1.0, abs(logp)) if math.isfinite(logp) else 1.0
    return 2.0 * (3 * n_frames + 4) * 2.0 ** -53 + 4.0 * 2.0 ** -52 * mag
