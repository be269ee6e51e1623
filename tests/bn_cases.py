"""Cases, operand builders, float64 references, derived bounds and a mirror of the launchers' form choice for the BatchNorm
edge suite (csrc/bn.hip: ds2_bn2d_stats / _apply_htanh / _htanh_bwd, ds2_bn1d_stats / _apply / _bwd).

Pure numpy, no GPU, no torch: tests/test_bn_cases_cpu.py proves on the CPU that the cases are what they claim to be,
tests/test_bn_edges_gpu.py runs them through the C ABI.

Operands.  Every tensor handed to an entry point lives in a flat fp32 buffer of its own (Flat, the 1-D sibling of
gemm_cases.Embedded): GUARD floats in front, `offset` floats (0..3) off 16-byte alignment, GUARD floats behind.  Inputs are
surrounded by NaN, outputs by a finite sentinel, the workspace is NaN throughout, exactly ds2_bn_ws_bytes(C) long, with a
sentinel guard behind it.  A NaN in a result therefore means a read outside an operand or a partial sum that no block wrote;
a changed guard means a write outside an output.

References.  All of them work on channel-major float64 arrays (C, N): the conv flavour's (B, C, inner) becomes
(C, B inner), the sequence flavour's (rows, F) becomes (F, rows), x = xa + xb exactly.  stats: mean, biased variance,
invstd = 1 / sqrt(var + eps), the running buffers as torch updates them (momentum, unbiased variance, biased when N = 1 as
the kernel does).  apply and backward take mean_invstd as GIVEN fp32 numbers (the ABI's input) and treat them as exact.

Bounds, with u = 2^-24 (one fp32 rounding is a relative error of at most u).  Nothing here is fitted to a result.

  Sums.  A thread adds at most n terms in fp32 (n - 1 roundings, each relative to a partial sum that is at most sum |term|),
  the partials are combined in fp64, and the result is rounded to fp32 once: with one or two roundings inside a term
  (x * x, dy * xhat with xhat = (x - mu) * invstd, each relative to the term) the error is at most (n + 2) u sum |term|.
  n comes from the launch geometry: conv flavour n <= 5 ceil(B ceil(inner / 1024) / 64) (a block takes every 64th of the
  B ceil(inner / 1024) chunks, a thread four elements of a chunk, or a quad and one head / tail element in the 16-byte
  form); sequence flavour n <= ceil(rows / 256) (64 blocks x 4 row lanes).  That bounds mean, E[x^2], dbeta and dgamma.
  The count is first-order (n u is far below 1: n <= 21 here) and takes the last product of a term as fused into the
  accumulation, which is how the 16-byte forms are compiled; the scalar forms are compiled with the product and the sum
  apart, one rounding more inside a term, so that over every pattern of roundings their worst case is n + 3.  The
  constant stays the stated n + 2 for every form; a thread with a single term (n = 1) is where it binds hardest, and the
  GPU suite's docstring lists how far the kernels reach into it.
  One term does not fit that pattern: with xb the kernels form x = fl(xa + xb), an ABSOLUTE error of u |x| that the
  subtraction of the mean does not shrink, so dgamma gets u sum |dy| |x| invstd on top, and the elementwise magnitudes
  below carry |x| beside |x - mu|.
  Variance: var = E[x^2] - mean^2, so t = b(E[x^2]) + 2 |mean| b(mean) + b(mean)^2 bounds its error (the fp64 arithmetic
  of the finalise kernel adds 2^-50 E[x^2]; clamping a negative variance to 0 only moves it towards the true one).
  invstd is held to the interval [1 / sqrt(var + t + eps), 1 / sqrt(max(var - t, 0) + eps)], widened by one rounding: no
  first-order estimate, so few-row channels need no band of their own.
  Running buffers: the update is fp64 on the fp32 buffer, rounded once: momentum b(mean) + u |new| for the mean,
  momentum t N / (N - 1) + u |new| for the variance.  Eval: mean_invstd[c] is the running mean bit for bit, invstd the fp64
  value rounded once, and the buffers keep every bit.
  Elementwise: K u M, M the sum of the magnitudes of the expression's terms, K its operation count (no contraction assumed).
    apply:  x * sc + (beta - mu * sc), sc = gamma * invstd: K = 5, M = gamma invstd (|x| + |mu|) + |beta| (both flavours; the
            sequence flavour's (fl(xa + xb) - mu) * sc + beta has five operations too and |x - mu| <= |x| + |mu|).
    dx:     gamma * invstd * (g - mg - xhat * mgx): K = 7 (8 with xb), M = gamma invstd (|g| + |mg| + (|x| + |mu|) invstd |mgx|),
            plus what the two means it reads may be off by: gamma invstd (b(dbeta) / N + |xhat| b(dgamma) / N).
  Borderline.  The backward's y = gamma * xhat + beta carries at most 4 u (|gamma xhat| + |beta|) (two roundings in xhat,
  one product, one sum); an element whose float64 pre-activation lies that close to 0 or 20 may fall on either side of the
  mask in fp32.  Such elements are left out of the dx comparison, their |dy| and |dy xhat| are added to b(dbeta) and
  b(dgamma) (and so, divided by N, to b(dx)); a case may have at most max(2, 1e-4 N) of them (BORDER_CAP).
"""
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from tests.gemm_cases import SENTINEL, cdiv

U = 2.0 ** -24
EPS = float(np.float32(1e-5))                # the ABI takes eps and momentum as float
MOMENTUM = float(np.float32(0.1))
NPART = 64
GUARD = 64                                   # floats in front of and behind every view (a multiple of 4)
NAN_BITS = 0xFFFFFFFF                        # a NaN as fp32 and, two of them, as fp64 (the workspace holds doubles)
ENTRIES = ('bn2d_stats', 'bn2d_apply', 'bn2d_bwd', 'bn1d_stats', 'bn1d_apply', 'bn1d_bwd')
EDGE_VALUES = np.array([-1.0, -0.0, 0.0, 1.0, np.nextafter(np.float32(20), np.float32(0)), 20.0,
                        np.nextafter(np.float32(20), np.float32(np.inf)), 25.0], np.float32)


# --------------------------------------------------------------------------------------------- embedded views
class Flat:
    """n floats, `offset` floats (0..3) off 16-byte alignment, inside a flat fp32 buffer whose every other float is `fill`:
    'nan' or 'sentinel'."""

    def __init__(self, n, offset=0, fill='nan'):
        assert n >= 1 and 0 <= offset < 4 and fill in ('nan', 'sentinel')
        self.n, self.offset, self.fill = n, offset, fill
        self.start = GUARD + offset
        self.size = cdiv(self.start + n + GUARD, 4) * 4
        self.bits = NAN_BITS if fill == 'nan' else SENTINEL
        self.buf = np.empty(self.size, np.float32)
        self.buf.view(np.uint32)[:] = self.bits

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.start:self.start + self.n]

    def put(self, arr):
        self.view()[...] = np.asarray(arr, np.float32).reshape(-1)
        return self

    def inside(self):
        mask = np.zeros(self.size, bool)
        mask[self.start:self.start + self.n] = True
        return mask

    def outside_intact(self, buf):
        """every float outside the view still holds the fill's bit pattern"""
        return bool(np.all(np.asarray(buf).view(np.uint32)[~self.inside()] == self.bits))


def ws_floats(c):
    """ds2_bn_ws_bytes(C) / 4: NPART fp64 pairs per channel, then two fp32 coefficients per channel"""
    return (c * NPART * 2 * 8 + c * 2 * 4) // 4


# --------------------------------------------------------------------------------------------- the launchers' choice
def form(entry, off, F=4, tbf=False):
    """'vec' or 'scalar' (or 'tbf'): which kernels an entry point launches, from csrc/bn.hip's host code.  off: operand name
    -> offset in floats off 16-byte alignment (missing = 0; a NULL xb counts as aligned, as in vec4_ok).  The conv flavour
    looks at the big tensors only (aligned16), the sequence flavour at F % 4 and at every pointer its 16-byte kernels read
    through float4 (vec4_ok)."""
    def aligned(*names):
        return all(off.get(nm, 0) % 4 == 0 for nm in names)
    if entry == 'bn2d_stats':
        ok = aligned('x')
    elif entry == 'bn2d_apply':
        if tbf:
            return 'tbf'
        ok = aligned('x', 'y')
    elif entry == 'bn2d_bwd':
        ok = aligned('x', 'dy', 'dx')
    elif entry == 'bn1d_stats':
        ok = F % 4 == 0 and aligned('xa', 'xb')
    elif entry == 'bn1d_apply':
        ok = F % 4 == 0 and aligned('xa', 'xb', 'y', 'gamma', 'beta', 'mi')
    elif entry == 'bn1d_bwd':
        ok = F % 4 == 0 and aligned('xa', 'xb', 'dy', 'dx', 'gamma', 'mi')
    else:
        raise ValueError(entry)
    return 'vec' if ok else 'scalar'


# --------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Conv:
    """conv flavour: x (B, C, D, T), inner = D T.  kind: 'fp64' (3 N + 5, both clamps populated), 'count' (integers: every sum
    exact), 'edge' (the clamp's and the mask's edge values, y = x exactly).  off: ((operand, offset), ...)."""
    section: str
    B: int
    C: int
    D: int
    T: int
    off: tuple = ()
    kind: str = 'fp64'
    tbf: bool = False           # run the (T, B, C D) layout as well
    running: bool = True        # training with running buffers (and then eval); False: without
    bump: int = 0               # another seed, should a case exceed BORDER_CAP

    flavour = 'conv'

    @property
    def inner(self):
        return self.D * self.T

    @property
    def channels(self):
        return self.C

    @property
    def count(self):
        return self.B * self.inner

    @property
    def n_run(self):
        return 5 * cdiv(self.B * cdiv(self.inner, 1024), NPART)

    @property
    def name(self):
        s = '%s-%dx%dx%dx%d-%s' % (self.section, self.B, self.C, self.D, self.T, self.kind)
        s += ''.join('-%s%d' % kv for kv in self.off)
        return s + ('' if self.running else '-norun')

    def offs(self):
        return dict(self.off)

    def forms(self):
        o = self.offs()
        return {e: form(e, o) for e in ENTRIES[:3]}

    def seed(self):
        return zlib.crc32(self.name.encode()) + self.bump

    def cm(self, a):
        """(B, C, inner) -> channel-major (C, B inner)"""
        return np.ascontiguousarray(np.asarray(a).reshape(self.B, self.C, self.inner).transpose(1, 0, 2)).reshape(self.C, -1)

    def nat(self, a):
        """channel-major -> (B, C, inner)"""
        return np.ascontiguousarray(a.reshape(self.C, self.B, self.inner).transpose(1, 0, 2))

    def tbf_of(self, y):
        """(B, C, D, T) -> (T, B, C D)"""
        return np.ascontiguousarray(y.reshape(self.B, self.C * self.D, self.T).transpose(2, 0, 1))


@dataclass(frozen=True)
class Seq:
    """sequence flavour: x = xa (+ xb), (rows, F)"""
    section: str
    rows: int
    F: int
    off: tuple = ()
    kind: str = 'fp64'
    xb: bool = True
    running: bool = True
    bump: int = 0

    flavour = 'seq'
    tbf = False

    @property
    def channels(self):
        return self.F

    @property
    def count(self):
        return self.rows

    @property
    def n_run(self):
        return cdiv(self.rows, 4 * NPART)

    @property
    def name(self):
        s = '%s-%dx%d-%s' % (self.section, self.rows, self.F, self.kind)
        s += ''.join('-%s%d' % kv for kv in self.off)
        return s + ('' if self.xb else '-noxb') + ('' if self.running else '-norun')

    def offs(self):
        o = dict(self.off)
        if not self.xb:
            o.pop('xb', None)
        return o

    def forms(self):
        o = self.offs()
        return {e: form(e, o, self.F) for e in ENTRIES[3:]}

    def seed(self):
        return zlib.crc32(self.name.encode()) + self.bump

    def cm(self, a):
        return np.ascontiguousarray(np.asarray(a).reshape(self.rows, self.F).T)

    def nat(self, a):
        return np.ascontiguousarray(a.T)


X1, X2, X3 = (('x', 1),), (('x', 2),), (('x', 3),)
DY1 = (('dy', 1),)
OUT1 = (('y', 1), ('dx', 1))
PARAMS = (('gamma', 1), ('beta', 2), ('mi', 3), ('rm', 1), ('rv', 2), ('dgamma', 3), ('dbeta', 1))      # the flat-buffer views


def conv_cases():
    out = []
    # rows of the (b, c) planes start at every base & 3: inner odd
    out += [Conv('rowstart', 5, 1, 3, 3, tbf=True), Conv('rowstart', 3, 3, 1, 5, tbf=True), Conv('rowstart', 2, 32, 1, 3, tbf=True)]
    # head / body / tail of a plane shorter than two quads
    out += [Conv('inner', 3, 3, 1, i) for i in (1, 2, 3, 4, 5, 7, 8)]
    out += [Conv('inner', 3, 3, 1, 7, off=X1)]
    # the reduction's chunk of 1024 elements
    out += [Conv('chunk', 2, 3, 1, i) for i in (1023, 1024, 1025, 1027, 1028, 2049)]
    out += [Conv('chunk', 2, 3, 1, i, off=X1) for i in (1024, 1025)]
    # B * chunks around NPART
    out += [Conv('items', b, 2, 1, 9) for b in (1, 63, 64, 65, 129)]
    out += [Conv('items', 21, 1, 1, 2049), Conv('items', 13, 1, 1, 4097), Conv('items', 43, 1, 1, 2049),
            Conv('items', 65, 2, 1, 9, off=X1), Conv('items', 43, 1, 1, 2049, off=X2)]
    # past the elementwise kernels' cap of 64 blocks per plane
    out += [Conv('cap', 2, 2, 1, 65541), Conv('cap', 2, 2, 1, 16387, off=X1)]
    # offsets: each of the last five must fall to the scalar form (PARAMS must not: the conv flavour reads them scalar)
    out += [Conv('offset', 3, 3, 1, 1027, off=o) for o in ((), X1, X2, X3, DY1, OUT1, PARAMS)]
    out += [Conv('offset', 3, 3, 1, 1027, off=o, running=False) for o in ((), X3)]
    # (T, B, C D): the channel changes inside a 32-row tile
    out += [Conv('tbf', 1, 1, 31, 31, tbf=True), Conv('tbf', 3, 2, 16, 32, tbf=True), Conv('tbf', 1, 3, 11, 33, tbf=True),
            Conv('tbf', 3, 3, 21, 33, tbf=True), Conv('tbf', 1, 3, 61, 31, tbf=True), Conv('tbf', 3, 2, 61, 32, tbf=True),
            Conv('tbf', 3, 3, 21, 33, off=X1 + PARAMS, tbf=True)]
    out += [Conv('real', 2, 32, 61, 75, tbf=True)]
    # exact: every element counted once
    out += [Conv('once', 3, 3, 1, 1027, kind='count'), Conv('once', 3, 3, 1, 1027, off=X1, kind='count'),
            Conv('once', 65, 2, 1, 1025, kind='count'), Conv('once', 65, 2, 1, 1025, off=X3, kind='count'),
            Conv('once', 2, 2, 1, 65541, kind='count'), Conv('once', 2, 2, 1, 16387, off=X1, kind='count'),
            Conv('once', 3, 3, 21, 33, kind='count', tbf=True)]
    # exact: the clamp's and the mask's edges
    out += [Conv('edges', 2, 3, 1, 1027, kind='edge'), Conv('edges', 2, 3, 1, 1027, off=X1, kind='edge'),
            Conv('edges', 3, 3, 21, 33, kind='edge', tbf=True), Conv('edges', 3, 3, 1, 7, kind='edge'),
            Conv('edges', 3, 3, 1, 7, off=OUT1, kind='edge')]
    return out


def seq_cases():
    out = []
    out += [Seq('F', 257, f) for f in (1, 30, 63, 64, 65)]                    # scalar: F % 4 (64: the full block)
    out += [Seq('F', 257, 64, off=(('xa', 1),))]
    out += [Seq('F4', 257, f) for f in (36, 252, 256, 260)] + [Seq('F4', 530, 800)]      # 9 / 63 / 64 / 65 / 200 quads
    out += [Seq('rows', r, f) for r in (1, 2, 3, 255, 256, 257, 530) for f in (30, 36)]
    out += [Seq('noxb', 257, 260, xb=False), Seq('noxb', 257, 65, xb=False), Seq('noxb', 3, 36, xb=False)]
    out += [Seq('offset', 257, 260, off=((nm, o),)) for nm, o in (('xb', 1), ('xa', 2), ('dy', 3), ('y', 1), ('dx', 2),
                                                                   ('beta', 1), ('mi', 2))]
    out += [Seq('offset', 530, 800, off=(('gamma', 1),))]                     # a view into a flat parameter buffer
    out += [Seq('offset', 257, 260, off=(('rm', 1), ('rv', 2), ('dgamma', 3), ('dbeta', 1)))]     # none of these decides
    out += [Seq('cap', 1311, 801), Seq('cap', 5243, 800)]                     # past 4096 blocks
    out += [Seq('norun', 257, 260, running=False), Seq('norun', 257, 65, running=False)]
    out += [Seq('once', 257, 65, kind='count'), Seq('once', 530, 260, kind='count'), Seq('once', 1311, 801, kind='count'),
            Seq('once', 5243, 800, kind='count'), Seq('once', 255, 36, kind='count', xb=False)]
    return out


def all_cases():
    return conv_cases() + seq_cases()


# pairs for "the 16-byte sequence kernels give the scalar kernels' bits": the same data, aligned and at offset 1
VEC_SCALAR_SHAPES = [(257, 36), (530, 260), (3, 256), (1311, 800)]

BORDER_CAP = lambda n: max(2, int(1e-4 * n))        # noqa: E731


# --------------------------------------------------------------------------------------------- references and bounds
def stats_ref(xc, n_run, eps=EPS):
    """xc (C, N) float64.  mean, var, invstd and their bounds (module docstring)."""
    n = xc.shape[1]
    mean = xc.sum(1) / n
    var = ((xc - mean[:, None]) ** 2).sum(1) / n
    e2 = (xc * xc).sum(1) / n
    b_mean = (n_run + 2) * U * np.abs(xc).sum(1) / n
    b_e2 = (n_run + 2) * U * e2
    t = b_e2 + 2 * np.abs(mean) * b_mean + b_mean ** 2 + 2.0 ** -50 * e2
    invstd = 1 / np.sqrt(var + eps)
    lo = 1 / np.sqrt(var + t + eps) * (1 - U)
    hi = 1 / np.sqrt(np.maximum(var - t, 0) + eps) * (1 + U)
    return SimpleNamespace(n=n, mean=mean, var=var, invstd=invstd, b_mean=b_mean, t=t, lo=lo, hi=hi)


def running_ref(st, rm, rv, momentum=MOMENTUM):
    """the buffers after one training step, and their bounds"""
    n = st.n
    k = n / (n - 1) if n > 1 else 1.0
    rm1 = (1 - momentum) * rm.astype(np.float64) + momentum * st.mean
    rv1 = (1 - momentum) * rv.astype(np.float64) + momentum * st.var * k
    b_rm = momentum * st.b_mean
    b_rv = momentum * st.t * k
    return SimpleNamespace(rm=rm1, rv=rv1, b_rm=b_rm + U * (np.abs(rm1) + b_rm), b_rv=b_rv + U * (np.abs(rv1) + b_rv))


def eval_ref(rm, rv, eps=EPS):
    """(mean bit for bit, invstd, its bound: fp64 arithmetic and one rounding)"""
    invstd = 1 / np.sqrt(rv.astype(np.float64) + eps)
    return rm.copy(), invstd, (U + 2.0 ** -50) * invstd


def apply_ref(xc, xabs, mi, gamma, beta, clamp):
    """y (C, N) and its bound under the given fp32 mean_invstd (2C)"""
    c = xc.shape[0]
    mu, inv = mi[:c].astype(np.float64)[:, None], mi[c:].astype(np.float64)[:, None]
    ga, be = gamma.astype(np.float64)[:, None], beta.astype(np.float64)[:, None]
    pre = ga * ((xc - mu) * inv) + be
    y = np.clip(pre, 0.0, 20.0) if clamp else pre
    bound = 5 * U * (np.abs(ga * inv) * (xabs + np.abs(mu)) + np.abs(be))
    return SimpleNamespace(pre=pre, y=y, bound=bound)


def bwd_ref(xc, xabs, dyc, mi, gamma, beta, clamp, n_run, xb_rounds, exact_mask=False):
    """dx (C, N), dgamma, dbeta (C) and their bounds; keep = the elements of dx that are compared (not borderline)"""
    c, n = xc.shape
    mu, inv = mi[:c].astype(np.float64)[:, None], mi[c:].astype(np.float64)[:, None]
    ga = gamma.astype(np.float64)[:, None]
    xh = (xc - mu) * inv
    if clamp:
        be = beta.astype(np.float64)[:, None]
        pre = ga * xh + be
        inside = (pre > 0) & (pre < 20)
        w = 4 * U * (np.abs(ga * xh) + np.abs(be))
        border = np.zeros_like(inside) if exact_mask else (np.abs(pre) <= w) | (np.abs(pre - 20) <= w)
        g = np.where(inside, dyc, 0.0)
    else:
        border = np.zeros(xc.shape, bool)
        g = dyc
    slack0 = np.where(border, np.abs(dyc), 0.0).sum(1)
    slack1 = np.where(border, np.abs(dyc * xh), 0.0).sum(1)
    dbeta, dgamma = g.sum(1), (g * xh).sum(1)
    b_dbeta = (n_run + 2) * U * np.abs(g).sum(1) + slack0
    b_dgamma = (n_run + 2) * U * np.abs(g * xh).sum(1) + slack1
    if xb_rounds:
        b_dgamma = b_dgamma + U * (np.abs(g) * xabs * np.abs(inv)).sum(1)
    mg, mgx = (dbeta / n)[:, None], (dgamma / n)[:, None]
    dx = ga * inv * (g - mg - xh * mgx)
    k = 8 if xb_rounds else 7
    b_dx = k * U * np.abs(ga * inv) * (np.abs(g) + np.abs(mg) + (xabs + np.abs(mu)) * np.abs(inv) * np.abs(mgx))
    b_dx = b_dx + np.abs(ga * inv) * ((b_dbeta / n)[:, None] + np.abs(xh) * (b_dgamma / n)[:, None])
    return SimpleNamespace(dx=dx, dgamma=dgamma, dbeta=dbeta, b_dx=b_dx, b_dgamma=b_dgamma, b_dbeta=b_dbeta, keep=~border,
                           borderline=int(border.sum()), g=g, xh=xh)


# --------------------------------------------------------------------------------------------- operand builders
def make(case, mi=None):
    """Everything one case needs: fp32 operands in the ABI's layout, the given mean_invstd (mi overrides it: a chained run hands
    apply and backward the statistics kernel's own output), float64 references in the same layout and their bounds."""
    rng = np.random.default_rng(case.seed())
    c, n = case.channels, case.count
    shape = (case.B, case.C, case.inner) if case.flavour == 'conv' else (case.rows, case.F)
    p = SimpleNamespace(case=case, shape=shape, xb=None)
    if case.kind == 'fp64':
        if case.flavour == 'conv':
            p.x = (3 * rng.standard_normal(shape) + 5).astype(np.float32)
            p.gamma = rng.uniform(7, 9, c).astype(np.float32)
            p.beta = rng.uniform(9, 11, c).astype(np.float32)
        else:
            if case.xb:                         # the sum has mean 5 and standard deviation 3 again
                p.x = (2 * rng.standard_normal(shape) + 2).astype(np.float32)
                p.xb = (2.2 * rng.standard_normal(shape) + 3).astype(np.float32)
            else:
                p.x = (3 * rng.standard_normal(shape) + 5).astype(np.float32)
            p.gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
            p.beta = rng.uniform(-1, 1, c).astype(np.float32)
        if 2 <= n < 30:
            # few elements per channel: a chance pair of near-equal draws would leave the variance to round-off.  Standardise
            # the draw per channel, so that mean / std = 5 / 3 here as well (the sum xa + xb when there are two).
            z = case.cm(rng.standard_normal(shape))
            z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
            target = case.nat(5 + 3 * z).reshape(shape)
            if p.xb is None:
                p.x = target.astype(np.float32)
            else:
                p.xb = (target - p.x).astype(np.float32)
        p.dy = rng.standard_normal(shape).astype(np.float32)
    elif case.kind == 'count':
        ints = lambda top: (rng.integers(1, top + 1, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float32)   # noqa: E731
        p.x = ints(4) if not (case.flavour == 'seq' and case.xb) else ints(2)
        if case.flavour == 'seq' and case.xb:
            other = ints(2)
            p.xb = np.where(p.x + other == 0, p.x, other).astype(np.float32)        # xa + xb in +-1..+-4, never 0
        p.dy = ints(3)
        p.gamma, p.beta = np.ones(c, np.float32), np.full(c, 10, np.float32)
    elif case.kind == 'edge':
        idx = np.arange(int(np.prod(shape))).reshape(shape)
        p.x = EDGE_VALUES[idx % len(EDGE_VALUES)]
        p.dy = rng.standard_normal(shape).astype(np.float32)
        p.gamma, p.beta = np.ones(c, np.float32), np.zeros(c, np.float32)
    else:
        raise ValueError(case.kind)
    p.rm0 = (0.5 * rng.standard_normal(c) + 1).astype(np.float32)
    p.rv0 = rng.uniform(0.5, 2, c).astype(np.float32)

    x64 = p.x.astype(np.float64) + (p.xb.astype(np.float64) if p.xb is not None else 0.0)
    xabs = np.abs(p.x.astype(np.float64)) + (np.abs(p.xb.astype(np.float64)) if p.xb is not None else 0.0)
    xc, xabs_c, dyc = case.cm(x64), case.cm(xabs), case.cm(p.dy.astype(np.float64))
    p.xc, p.dyc = xc, dyc
    p.st = stats_ref(xc, case.n_run)
    p.run = running_ref(p.st, p.rm0, p.rv0)
    if mi is not None:
        p.mi = np.asarray(mi, np.float32)
    elif case.kind == 'fp64':
        p.mi = np.concatenate([p.st.mean, p.st.invstd]).astype(np.float32)
    else:
        p.mi = np.concatenate([np.zeros(c), np.ones(c)]).astype(np.float32)
    clamp = case.flavour == 'conv'
    p.ap = apply_ref(xc, xabs_c, p.mi, p.gamma, p.beta, clamp)
    p.bw = bwd_ref(xc, xabs_c, dyc, p.mi, p.gamma, p.beta, clamp, case.n_run, xb_rounds=p.xb is not None,
                   exact_mask=case.kind == 'edge')
    return p


# --------------------------------------------------------------------------------------------- checks (CPU emulation and GPU alike)
def _ratio(err, bound):
    """max err / bound, with 0 / 0 = 0"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    return float(r.max()) if r.size else 0.0


def stats_ratios(p, mi):
    """how far into their bounds a computed mean_invstd (2C, fp32) reaches: <= 1 means inside"""
    c = p.case.channels
    mean, inv = mi[:c].astype(np.float64), mi[c:].astype(np.float64)
    st = p.st
    above = (inv - st.invstd) / (st.hi - st.invstd)
    below = (st.invstd - inv) / (st.invstd - st.lo)
    return {'mean': _ratio(np.abs(mean - st.mean), st.b_mean), 'invstd': float(np.maximum(above, below).max())}


def running_ratios(p, rm, rv):
    return {'running_mean': _ratio(np.abs(rm.astype(np.float64) - p.run.rm), p.run.b_rm),
            'running_var': _ratio(np.abs(rv.astype(np.float64) - p.run.rv), p.run.b_rv)}


def apply_ratios(p, y):
    """y in the ABI's plain layout"""
    return {'y': _ratio(np.abs(p.case.cm(y.astype(np.float64)) - p.ap.y), p.ap.bound)}


def bwd_ratios(p, dx, dgamma, dbeta):
    bw = p.bw
    err = np.abs(p.case.cm(dx.astype(np.float64)) - bw.dx)
    return {'dx': _ratio(err[bw.keep], bw.b_dx[bw.keep]),
            'dgamma': _ratio(np.abs(dgamma.astype(np.float64) - bw.dgamma), bw.b_dgamma),
            'dbeta': _ratio(np.abs(dbeta.astype(np.float64) - bw.dbeta), bw.b_dbeta)}


def exact_expectations(p):
    """what the exact cases fix bit for bit (fp32 arrays in the ABI's plain layout)"""
    case = p.case
    out = SimpleNamespace()
    if case.kind == 'count':
        s = p.xc.sum(1)
        out.mean = (s / case.count).astype(np.float32)
        out.invstd = (1 / np.sqrt((p.xc * p.xc).sum(1) / case.count - (s / case.count) ** 2 + EPS)).astype(np.float32)
        out.dbeta = p.dyc.sum(1).astype(np.float32)                     # g = dy: beta = 10 keeps every element interior
        out.dgamma = (p.dyc * p.xc).sum(1).astype(np.float32)           # xhat = x under mean_invstd = (0, 1)
        out.y = case.nat(p.xc + 10.0).astype(np.float32)                # an integer in 6..14
    elif case.kind == 'edge':
        x = p.x
        out.y = np.where(x > 0, np.minimum(x, np.float32(20)), np.float32(0)).astype(np.float32)      # +0 for -1, -0 and 0
        out.inside = (x > 0) & (x < 20)                                 # strict on both sides
    return out
