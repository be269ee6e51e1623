"""Numpy restatement of the SpecAugment stage (``ds2_spec_augment``, include/ds2hip.h "SpecAugment"), the reference the
device kernel is held to.  One clip at a time:

    warp    t <  c2: num = t c,               den = c2,      base = 0
            t >= c2: num = (t - c2) (T - c),  den = T - c2,  base = c
            i0 = base + num // den, i1 = min(i0 + 1, T - 1), frac = (num % den) / den
            y[t] = x[i0] + frac (x[i1] - x[i0])                     float64, from the same integers as the kernel
    masks   frequency, then time, clamped into [0, 161) and [0, T): the cells are SET to mask_value       exact
    padding frames t >= T are 0

Nothing here imports the product."""
import numpy as np

NB = 161


def warp_rows(T, c, c2):
    """(i0, i1, num % den, den) as int64 arrays over the output frames 0..T-1."""
    T, c, c2 = int(T), int(c), int(c2)
    assert 0 <= c < T and 0 <= c2 < T
    t = np.arange(T, dtype=np.int64)
    left = t < c2
    num = np.where(left, t * c, (t - c2) * (T - c))
    den = np.where(left, max(c2, 1), T - c2)
    i0 = np.where(left, 0, c) + num // den
    assert i0.min() >= 0 and i0.max() <= T - 1
    return i0, np.minimum(i0 + 1, T - 1), num % den, den


def masked_cells(T, fmask, tmask):
    """Boolean (T, 161): the cells some mask covers.  fmask: (f0, f) pairs, tmask: (t0, t) pairs; a width <= 0 is no mask."""
    m = np.zeros((int(T), NB), bool)
    for f0, f in (fmask if fmask is not None else []):
        lo, hi = max(int(f0), 0), min(int(f0) + max(int(f), 0), NB)
        if hi > lo:
            m[:, lo:hi] = True
    for t0, w in (tmask if tmask is not None else []):
        lo, hi = max(int(t0), 0), min(int(t0) + max(int(w), 0), int(T))
        if hi > lo:
            m[lo:hi, :] = True
    return m


def spec_augment_ref(x32, T, warp=None, fmask=None, tmask=None, mask_value=0.0):
    """One clip.  x32: (t_max, 161) float32; T its valid frames; warp (c, c2) or None.  Returns (out float64 (t_max, 161),
    bound float64 of the same shape: the largest error three float32 roundings of the warp formula can leave -- 0 wherever
    the cell is a copy, a mask or padding)."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    T = int(T)
    assert x.ndim == 2 and x.shape[1] == NB and 1 <= T <= x.shape[0]
    out, bound = np.zeros_like(x), np.zeros_like(x)
    if warp is None:
        out[:T] = x[:T]
    else:
        i0, i1, rem, den = warp_rows(T, warp[0], warp[1])
        x0, x1 = x[i0], x[i1]
        with np.errstate(invalid='ignore'):
            y = x0 + (rem / den.astype(np.float64))[:, None] * (x1 - x0)
            b = 2.0 ** -24 * (3.0 * np.abs(x1 - x0) + np.maximum(np.abs(x0), np.abs(x1)))
        copy = rem == 0                              # frac == 0: the frame is x[i0] itself, bit for bit
        y[copy], b[copy] = x0[copy], 0.0
        out[:T], bound[:T] = y, b
    m = masked_cells(T, fmask, tmask)
    out[:T][m] = np.float64(np.float32(mask_value))
    bound[:T][m] = 0.0
    return out, bound


def batch_ref(x32, frames, warp=None, fmask=None, tmask=None, mask_value=0.0):
    """The batch: x32 (B, t_max, 161); per-clip tables as ``ds2hip.ops.spec_augment`` takes them."""
    outs = [spec_augment_ref(x32[b], frames[b], None if warp is None else warp[b], None if fmask is None else fmask[b],
                             None if tmask is None else tmask[b], mask_value) for b in range(len(frames))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
