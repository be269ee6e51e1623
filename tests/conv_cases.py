"""Cases, operand builders, references and a mirror of the launchers' form choice for the convolution edge suite.

Pure numpy, no GPU: tests/test_conv_cases_cpu.py proves on the CPU that the cases are what they claim to be,
tests/test_conv_edges_gpu.py runs them through ds2_conv_fwd, ds2_conv2_dgrad and ds2_conv_wgrad (csrc/conv.hip,
csrc/conv_split.hip).

The mirror (fwd_form, dgrad_form, wgrad_form) follows the host code of the RELEASE library line by line.  There ds2_tune_env
returns null, so DS2_CONV_NT, DS2_CONV_KS, DS2_CONV_SPLIT_KS / NT, DS2_CONV*_WGRAD_SPLIT and DS2_CONV_SPLIT_DGRAD_MIN are inert;
what a test can switch are the getenv ones: DS2_CONV_SPLIT = 0 / 6 / 9, DS2_CONV_SPLIT_DGRAD = 0 / 1, DS2_CONV_DGRAD_ROWS,
DS2_CONV_DGRAD_MERGE, DS2_CONV_WGRAD_LDS, DS2_CONV_WGRAD_BF16.  Instantiations that only the tuning build reaches are out of
scope: conv2_dgrad_kernel other than <21, 2, 4> and conv2's direct forward kernel with NT = 1.  The GPU suite asserts results
only, never which kernel ran: if the mirror drifts from the launchers it can understate coverage, it cannot hide a failure.
(When the table was written, a kernel trace of one launch per (entry point, shape, environment) of it showed the kernel
template, the grid and the number of launches the mirror names, for all 123 of them.)

References (the first two need no tolerance):
  'int'   small-integer operands with 2 max|a| max|b| K + max|bias| < 2^24, K every accumulated term (cin kf kt forward and
          data gradient, B fout tout for the weight gradient): every partial product of every split term and every partial
          sum in any order is an exactly representable integer (the argument is tests/gemm_cases.py's), so the result is exact
          in every kernel form, through the LDS shares of a K split and under float atomics;
  'sel'   arbitrary fp32 data (24-bit significands, exponents over [2^-100, 2^100)) against a one-hot +-1 operand: every
          output is +- one element of the data, or 0 in the padding, bit for bit; all three bf16 planes of the data are needed.
          Forward: one +-1 tap per output channel.  Data gradient: one +-1 tap per output channel, the chosen input channels a
          permutation, so no two terms meet.  Weight gradient: d_out holds one +-1 per channel, so d_weight[co] is +- a window
          of the (padded) input and d_bias is +-1;
  'fp64'  operands in the training ranges against float64 under
              |c - ref| <= (K + S + 2) 2^-24 (|a| * |b| (+ |bias|)),            (* = the same convolution of the moduli)
          derived as for the GEMMs: every accumulated term costs one rounding of relative size <= 2^-24 of a partial sum that
          sum |a||b| bounds -- K counts the slots of the longest accumulation, those that multiply a zero included (12 padded
          time taps, tap groups of 8, 64-step chunks) --, every extra addition (S: the K shares added through LDS, the
          pieces added by float atomics) one more, the split products are within 2^-24 of a b (csrc/split_bf16.h,
          tests/test_split_cpu.py), and the bias one more.  K and S come from the mirror's form; nothing is fitted.

Operands live in Flat buffers (tests/bn_cases.py): GUARD = 64 floats of NaN around every input, of a sentinel around every
output, at an offset of 0..3 floats off 16-byte alignment (the kernels read through f32x4u and raw buffer loads: 4-byte
alignment is the contract).  No kernel may read behind an operand at all: input rows are read through buffer descriptors of
exactly the row's or the tensor's length or through clamped indices, and the 16-byte loads of the weight-gradient kernels
start only where 8 elements are left in the row.  The furthest address a WRONG tap could form without leaving the checked
range of a neighbouring row is one filter row's 12 padded taps plus a 16-byte run = 15 floats behind an operand, so 64 floats
hold it and no case can leave its own allocations."""
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from tests.bn_cases import GUARD, NAN_BITS, SENTINEL, Flat  # noqa: F401  (re-exported for the two test modules)
from tests.gemm_cases import full_significand_matrix

Geom = namedtuple('Geom', 'cin kf kt sf st padt fin fout')
GEOM = {1: Geom(1, 41, 11, 2, 2, 10, 161, 61), 2: Geom(32, 21, 11, 2, 1, 0, 61, 21)}
KTP = 12                                     # time taps padded to 12 in the direct kernels
BUF_LIMIT = 0x7FFFFFF0


def cdiv(a, b):
    return (a + b - 1) // b


def conv_tout(which, tin):
    """conv_tout of csrc/conv.hip for tin > 0"""
    return (tin + 9) // 2 + 1 if which == 1 else tin - 10


def wt_ws_floats(which):
    g = GEOM[which]
    direct = max(32, g.cin) * g.kf * KTP * 32
    split = 1024 + (16 * 32 + 4) * 3 * 32 * 16 // 2 + 4096 if which == 2 else 0
    return max(direct, split)


def tap_groups(nrows):
    return 3 * (nrows // 2) + 2 * (nrows & 1)


def dgrad_ws_floats(b, t1):
    img = [(16 * tap_groups(n) + 4) * 3 * 32 * 16 // 2 for n in (11, 10)]
    return max(wt_ws_floats(2), 1024 + img[0] + img[1] + b * 32 * 41 * (t1 + 10) + 64)


# --------------------------------------------------------------------------------------------- the launchers' choice
@dataclass(frozen=True)
class Form:
    kernel: str             # 'gather6-nt2', 'direct-nt2-ks4', 'conv1-nt1', 'wgrad-direct', 'wgrad-lds', 'wgrad-split', ...
    K: int                  # slots of the longest accumulation chain (zero slots included)
    S: int                  # extra additions per output: LDS shares, atomic pieces
    info: tuple = ()        # sorted (key, value) pairs: what the coverage assertions look at

    def get(self, key, default=None):
        return dict(self.info).get(key, default)


def _form(kernel, K, S, **info):
    return Form(kernel, K, S, tuple(sorted(info.items())))


def plan_gather(M, nstep, may_split):
    nt = 2 if cdiv(M, 64) >= 1536 else 1
    tiles = cdiv(M, 128 * nt)
    waves = tiles * 4
    ks = 1 if not may_split else (1 if waves >= 1024 else (2 if waves >= 512 else 3))
    per = cdiv(nstep, ks)
    return nt, tiles, cdiv(nstep, per)


def _split_mode(env):
    v = int(env.get('DS2_CONV_SPLIT', '6'))
    return v if v in (6, 9) else 0


def fwd_form(which, B, tin, env=None):
    """ds2_conv_fwd"""
    env = env or {}
    g = GEOM[which]
    tout = conv_tout(which, tin)
    mode = _split_mode(env)
    if which == 2 and mode and 4 * B * 32 * 61 * tin < BUF_LIMIT and B * 32 * 21 * tout < BUF_LIMIT:
        M = B * 21 * tout
        nt, tiles, _ = plan_gather(M, 512, False)
        return _form('gather%d-nt%d' % (mode, nt), 16 * 32 * 16, 1, tiles=tiles, tiles8=tiles % 8, M=M, ragged=M % (128 * nt) != 0,
                     side=cdiv(M, 64) - 1536)
    def rounds(nt):
        return cdiv(B * cdiv(tout, 32 * nt) * g.fout, 1024) * nt
    nt = 2 if which == 2 else (1 if rounds(1) < rounds(2) else 2)
    ttiles = cdiv(tout, 32 * nt)
    ntiles = B * ttiles * g.fout
    ks = 1 if which == 1 else (4 if ntiles < 700 else (2 if ntiles < 4096 else 1))
    return _form('%s-nt%d-ks%d' % ('conv1' if which == 1 else 'direct', nt, ks), g.cin * g.kf * KTP, ks - 1, ntiles=ntiles,
                 empty_slots=(-ntiles) % (4 // ks), ragged=tout % (32 * nt) != 0, pad_only=which == 1 and tin < 11)


def dgrad_form(B, t1, env=None):
    """ds2_conv2_dgrad with a workspace of ds2_conv2_dgrad_ws_floats(B, T1)"""
    env = env or {}
    mode = _split_mode(env)
    on = env.get('DS2_CONV_SPLIT_DGRAD')
    gather = mode != 0 and (on[0] == '1' if on else B * t1 >= 1000)
    if gather and (4 * B * 32 * 41 * (t1 + 10) >= BUF_LIMIT or B * 32 * 61 * t1 >= BUF_LIMIT):
        gather = False
    if not gather:
        ntiles = B * cdiv(t1, 64) * 61
        return _form('dgrad-direct-nt2-ks4', 32 * 11 * KTP, 3, ntiles=ntiles, ragged=t1 % 64 != 0, side=B * t1 - 1000)
    rows_on = env.get('DS2_CONV_DGRAD_ROWS', '1')[0] != '0'
    merge_on = env.get('DS2_CONV_DGRAD_MERGE', '1')[0] != '0'
    plans = [plan_gather(B * rh * t1, 16 * tap_groups(nr), True) for rh, nr in ((31, 11), (30, 10))]
    nsplit = (plans[0][2], plans[1][2])
    merged = merge_on and nsplit == (1, 1)
    nts = (plans[0][0], plans[0][0]) if merged else (plans[0][0], plans[1][0])
    walk = tuple(rows_on and s == 1 for s in nsplit)
    spans, two_b = [], False
    for par, rh in enumerate((31, 30)):                 # the rows a workgroup's positions span, and whether they cross a batch element
        if not walk[par]:
            spans.append(0)
            continue
        M, wg = B * rh * t1, 128 * nts[par]
        m0 = np.arange(0, M, wg)
        ri0, ri1 = m0 // t1, (np.minimum(m0 + wg, M) - 1) // t1
        same = ri0 // rh == ri1 // rh
        two_b = two_b or bool((~same).any())
        spans.append(int((ri1 - ri0 + 1)[same].max()) if same.any() else 0)
    return _form('dgrad-gather%d' % mode, 16 * 17 * 16, max(nsplit), nsplit=nsplit, plan_nt=(plans[0][0], plans[1][0]), nts=nts,
                 merged=merged, zero_fill=max(nsplit) > 1, walk=walk, max_rows=max(spans), two_batch=two_b,
                 tiles8=tuple(cdiv(B * rh * t1, 128 * n) % 8 for rh, n in zip((31, 30), nts)), side=B * t1 - 1000)


WGRAD_ENV = {'direct': {'DS2_CONV_WGRAD_LDS': '0'}, 'lds-f32': {'DS2_CONV_WGRAD_LDS': '1', 'DS2_CONV_WGRAD_BF16': '0'},
             'split': {'DS2_CONV_WGRAD_LDS': '1', 'DS2_CONV_WGRAD_BF16': '1'}}


def wgrad_form(which, B, tin, env=None):
    """ds2_conv_wgrad"""
    env = env or {}
    g = GEOM[which]
    tout = conv_tout(which, tin)
    rows, ntot = B * g.fout, g.cin * g.kf * g.kt
    lds = env.get('DS2_CONV_WGRAD_LDS', '1')[0] != '0'
    bf16 = lds and env.get('DS2_CONV_WGRAD_BF16', '1')[0] != '0'
    common = dict(tout=tout, rows=rows, pad_only=which == 1 and tin < 11)
    if not lds:
        want = cdiv(2048, cdiv(ntot, 32))
        nsplit = max(min(want, cdiv(rows, 4)), 1)
        myrows = cdiv(cdiv(rows, 4), nsplit)            # rows a wave walks: every 4 nsplit-th
        return _form('wgrad%d-direct' % which, myrows * cdiv(tout, 16) * 16, nsplit, nsplit=nsplit, clamp=want - cdiv(rows, 4),
                     tail8=tout % 16, **common)
    want = 256 if which == 1 else 105
    split = max(min(want, rows), 1)
    myrows = (cdiv(rows, split), rows // split)
    tchunks = cdiv(tout, 64)
    return _form('wgrad%d-%s' % (which, 'split' if bf16 else 'lds'), myrows[0] * tchunks * 64, split, split=split, clamp=want - rows,
                 uneven=myrows[0] != myrows[1], tchunks=tchunks, ragged=tout % 64, **common)


# --------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    entry: str              # 'fwd', 'dgrad', 'wgrad'
    which: int
    B: int
    T: int                  # t_in_frames (fwd, wgrad) or T1 (dgrad)
    ref: str = 'int'
    env: tuple = ()         # sorted (name, value) pairs
    off: int = 0            # floats off 16-byte alignment of the big operands (0..3)

    @property
    def name(self):
        e = ','.join('%s=%s' % (k.replace('DS2_CONV_', ''), v) for k, v in self.env)
        return '%s%d-%dx%d-%s%s%s' % (self.entry, self.which, self.B, self.T, self.ref, '-' + e if e else '',
                                      '-off%d' % self.off if self.off else '')

    def envd(self):
        return dict(self.env)

    def form(self):
        if self.entry == 'fwd':
            return fwd_form(self.which, self.B, self.T, self.envd())
        if self.entry == 'dgrad':
            return dgrad_form(self.B, self.T, self.envd())
        return wgrad_form(self.which, self.B, self.T, self.envd())

    def key(self):
        """what the operands depend on: cases that differ in the environment or the alignment only share them"""
        return (self.entry, self.which, self.B, self.T, self.ref)

    def seed(self):
        return zlib.crc32(repr(self.key()).encode())

    def tout(self):
        return conv_tout(2, self.T) if self.entry == 'dgrad' else conv_tout(self.which, self.T)

    def K(self):
        """every accumulated term of one output (the integer cap's K)"""
        g = GEOM[self.which]
        return self.B * g.fout * self.tout() if self.entry == 'wgrad' else g.cin * g.kf * g.kt

    def shapes(self):
        """(data, one-hot-able other operand, result) shapes: fwd (x, w, out), dgrad (d_out, w, d_in), wgrad (x, d_out, d_w)"""
        g, b, t, to = GEOM[self.which], self.B, self.T, self.tout()
        wshape = (32, g.cin, g.kf, g.kt)
        if self.entry == 'fwd':
            return (b, g.cin, g.fin, t), wshape, (b, 32, g.fout, to)
        if self.entry == 'dgrad':
            return (b, 32, 21, to), wshape, (b, 32, 61, t)
        return (b, g.cin, g.fin, t), (b, 32, g.fout, to), wshape


def _env(**kw):
    return tuple(sorted(('DS2_CONV_' + k, str(v)) for k, v in kw.items()))


REFS = ('int', 'sel', 'fp64')
# forward, gather kernel: the 64-positions-per-wave threshold (cdiv(M, 64) = 1535 | 1536), 24 batch elements on its far side, one
# partly filled workgroup, tile counts 20, 23 and 9 (not multiples of 8: the XCD deal's uneven shares)
FWD_GATHER = [(2, 2349), (1, 4689), (24, 205), (1, 11), (3, 50), (5, 37), (2, 38)]
# forward, direct conv2: K shares 4 | 2 at 700 tiles, 2 | 1 at 4096, an odd tile count under KS = 2, ntiles % 4 = 1 under KS = 1,
# several time tiles with a ragged last one
FWD_DIRECT = [(33, 11), (34, 11), (35, 11), (195, 11), (196, 11), (197, 20), (2, 139)]
FWD_CONV1 = [(2, 629), (2, 630), (1, 1), (1, 2), (1, 11), (9, 120), (3, 64)]
# data gradient, gather kernel: K splits 2 | 3, 1 | 2, plans NT 2 | 1 under a merged launch, row walks across batch elements, one
# parity walking while the other splits, K split 3 on both, 256 positions over 24 rows (B = 289: NT = 2 at T1 = 11)
DGRAD_GATHER = [(1, 530), (5, 106), (1, 1060), (2, 1600), (10, 320), (100, 11), (96, 11), (3, 11), (289, 11), (12, 90)]
DGRAD_DEFAULT = [(1, 999), (1, 1000), (3, 11), (9, 111), (7, 143)]      # B T1 = 999 | 1000 | 33 | 999 | 1001
DGRAD_DIRECT = [(3, 11), (1, 530), (2, 139), (1, 64), (1, 65)]
# weight gradients: (B, T_in)
WGRAD2 = [(1, 11), (1, 17), (1, 18), (1, 73), (1, 74), (1, 75), (2, 75), (4, 21), (5, 23), (6, 19)]
WGRAD1 = [(1, 1), (1, 2), (1, 3), (1, 5), (1, 10), (2, 115), (1, 117), (1, 118), (1, 119), (4, 30), (5, 33), (8, 21), (9, 21)]


def fwd_cases():
    out = []
    for i, (b, t) in enumerate(FWD_GATHER):
        big = b * t > 4000
        out += [Case('fwd', 2, b, t, r, off=i % 4) for r in REFS]
        out += [Case('fwd', 2, b, t, r, _env(SPLIT=9), off=(i + 1) % 4) for r in (('int', 'sel') if big else REFS)]
    for i, (b, t) in enumerate(FWD_DIRECT):
        out += [Case('fwd', 2, b, t, r, _env(SPLIT=0), off=i % 4) for r in REFS]
    for i, (b, t) in enumerate(FWD_CONV1):
        out += [Case('fwd', 1, b, t, r, off=i % 4) for r in REFS]
    return out


def dgrad_cases():
    out = []
    for i, (b, t) in enumerate(DGRAD_GATHER):
        out += [Case('dgrad', 2, b, t, r, _env(SPLIT_DGRAD=1), off=i % 4) for r in REFS]
    for b, t in ((1, 530), (100, 11), (2, 1600), (3, 11)):
        out += [Case('dgrad', 2, b, t, r, _env(SPLIT_DGRAD=1, SPLIT=9), off=1) for r in ('int', 'sel')]
    out += [Case('dgrad', 2, 100, 11, r, _env(SPLIT_DGRAD=1, DGRAD_ROWS=0), off=2) for r in ('int', 'sel')]
    out += [Case('dgrad', 2, 100, 11, r, _env(SPLIT_DGRAD=1, DGRAD_MERGE=0), off=3) for r in ('int', 'sel')]
    for i, (b, t) in enumerate(DGRAD_DEFAULT):
        out += [Case('dgrad', 2, b, t, r, off=i % 4) for r in REFS]
    for i, (b, t) in enumerate(DGRAD_DIRECT):
        out += [Case('dgrad', 2, b, t, r, _env(SPLIT_DGRAD=0), off=i % 4) for r in REFS]
    return out


def wgrad_cases():
    out = []
    for which, shapes in ((2, WGRAD2), (1, WGRAD1)):
        for i, (b, t) in enumerate(shapes):
            for fname, env in WGRAD_ENV.items():
                out += [Case('wgrad', which, b, t, r, tuple(sorted(env.items())), off=i % 4) for r in REFS]
    return out


def all_cases():
    return fwd_cases() + dgrad_cases() + wgrad_cases()


# --------------------------------------------------------------------------------------------- references
def padded(which, x, dtype):
    """x (B, cin, fin, T) with PADT zero columns in front and PADT + 1 behind (the + 1 is room for a tap shifted by one)"""
    g = GEOM[which]
    return np.pad(np.asarray(x, dtype), ((0, 0), (0, 0), (0, 0), (g.padt, g.padt + 1)))


def _win(which, xp, kf, kt, tout, shift=0):
    """the input elements filter tap (kf, kt) meets, one per output position: (B, cin, fout, tout)"""
    g = GEOM[which]
    return xp[:, :, kf:kf + g.sf * (g.fout - 1) + 1:g.sf, kt + shift:kt + shift + g.st * (tout - 1) + 1:g.st]


def add_tap(entry, which, a, b, acc, kf, kt, scale=1, shift=0):
    """Add filter tap (kf, kt)'s terms, times `scale`, into acc, in acc's dtype; shift = 1 reads / writes one column off.
    fwd: a = padded x, b = w, acc = out.  dgrad: a = d_out, b = w, acc = d_in with one spare column.  wgrad: a = padded x,
    b = d_out, acc = d_w."""
    if entry == 'fwd':
        win = _win(which, a, kf, kt, acc.shape[3], shift)
        acc += scale * np.tensordot(b[:, :, kf, kt], win, axes=(1, 1)).transpose(1, 0, 2, 3)
    elif entry == 'dgrad':
        t = a.shape[3]
        acc[:, :, kf:kf + 41:2, kt + shift:kt + shift + t] += scale * np.tensordot(b[:, :, kf, kt], a, axes=(0, 1)).transpose(1, 0, 2, 3)
    else:
        win = _win(which, a, kf, kt, b.shape[3], shift)
        acc[:, :, kf, kt] += scale * np.tensordot(b, win, axes=([0, 2, 3], [0, 2, 3]))
    return acc


def prepare(entry, which, data, other, dtype):
    """(a, b, zeroed accumulator) for add_tap from the operands as the library takes them: (x, w), (d_out, w) or (x, d_out)"""
    g = GEOM[which]
    if entry == 'fwd':
        B, tout = data.shape[0], conv_tout(which, data.shape[3])
        return padded(which, data, dtype), np.asarray(other, dtype), np.zeros((B, 32, g.fout, tout), dtype)
    if entry == 'dgrad':
        B, t = data.shape[0], data.shape[3]
        return np.asarray(data, dtype), np.asarray(other, dtype), np.zeros((B, 32, 61, t + 11), dtype)
    return padded(which, data, dtype), np.asarray(other, dtype), np.zeros((32, g.cin, g.kf, g.kt), dtype)


def finish(entry, acc, bias=None):
    if entry == 'dgrad':
        return np.ascontiguousarray(acc[..., :-1])
    if entry == 'fwd' and bias is not None:
        return acc + np.asarray(bias, acc.dtype)[None, :, None, None]
    return acc


def convolve(entry, which, data, other, dtype, bias=None):
    """the plain tap loop in `dtype`: float64 is the reference, float32 the emulation"""
    g = GEOM[which]
    a, b, acc = prepare(entry, which, data, other, dtype)
    for kf in range(g.kf):
        for kt in range(g.kt):
            add_tap(entry, which, a, b, acc, kf, kt)
    return finish(entry, acc, bias)


def tampered(entry, which, data, other, clean, kind, tap, bias=None):
    """`clean` (the fp32 tap loop's result) with filter tap `tap` 'drop'ped, 'shift'ed by one column or counted 'twice'"""
    a, b, acc = prepare(entry, which, data, other, np.float32)
    kf, kt = tap
    if kind in ('drop', 'shift'):
        add_tap(entry, which, a, b, acc, kf, kt, scale=-1)
    if kind == 'shift':
        add_tap(entry, which, a, b, acc, kf, kt, shift=1)
    if kind == 'twice':
        add_tap(entry, which, a, b, acc, kf, kt)
    return clean + finish(entry, acc)


def bias_grad(d_out, dtype):
    return np.asarray(d_out, dtype).sum(axis=(0, 2, 3))


def fp64_bound(form, scale):
    return (form.K + form.S + 2) * 2.0 ** -24 * scale


def worst_ratio(err, bound):
    """max err / bound; where the bound is 0 (every term multiplies the padding) the error must be 0 too"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if (err[bound == 0] != 0).any() or not np.isfinite(err).all():
        return float('inf')
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# --------------------------------------------------------------------------------------------- operand builders
BIAS_MAX = 1000


def int_range(K):
    """v with 2 v v K + BIAS_MAX < 2^24: both operands are drawn from [-v, v]"""
    v = int(np.sqrt((2 ** 24 - 1 - BIAS_MAX) / (2.0 * K)))
    while 2 * v * v * K + BIAS_MAX >= 2 ** 24:
        v -= 1
    assert v >= 1, 'K = %d is beyond the integer builder' % K
    return min(v, 255)


def _ints(rng, shape, v):
    return rng.integers(-v, v + 1, size=shape).astype(np.float32)


def _must_then_random(rng, must, draw, n=32):
    picks = list(must)[:n]
    while len(picks) < n:
        picks.append(draw())
    order = rng.permutation(n)
    order = np.concatenate([[0], order[order != 0]])            # channel 0 keeps the first pick: the tap the CPU test tampers with
    return [picks[i] for i in order]


def _sel_filter(rng, which, permute):
    """w with one +-1 tap per output channel: the corners and the tap-group edges of the filter first, then random taps.
    permute: channel co's input channel is pi(co), a permutation (data gradient)."""
    g = GEOM[which]
    kts, kfs = (0, 3, 4, 7, 8, 10), (0, 1, g.kf - 2, g.kf - 1)
    must = [(kf, kt) for kf in kfs for kt in kts]
    taps = _must_then_random(rng, must, lambda: (int(rng.integers(g.kf)), int(rng.integers(g.kt))))
    ci = rng.permutation(32) if permute else rng.integers(0, g.cin, size=32)
    if g.cin > 1 and not permute:
        ci[:4] = (0, 1, g.cin - 2, g.cin - 1)
    sg = rng.choice(np.array([-1.0, 1.0], np.float32), size=32)
    w = np.zeros((32, g.cin, g.kf, g.kt), np.float32)
    for co in range(32):
        w[co, ci[co], taps[co][0], taps[co][1]] = sg[co]
    return w, (np.asarray(ci), taps, sg)


def _sel_dout(rng, which, B, tout):
    """d_out with one +-1 per channel: the corners of (b, d, t) and both sides of the 8-, 16- and 64-step boundaries first"""
    g = GEOM[which]
    ts = sorted({t for t in (0, 7, 8, 15, 16, 63, 64, tout - 1) if t < tout})
    must = [(b, d, t) for t in ts for b, d in ((0, 0), (B - 1, g.fout - 1))]
    pos = _must_then_random(rng, must, lambda: (int(rng.integers(B)), int(rng.integers(g.fout)), int(rng.integers(tout))))
    sg = rng.choice(np.array([-1.0, 1.0], np.float32), size=32)
    d = np.zeros((B, 32, g.fout, tout), np.float32)
    for co in range(32):
        d[pos[co][0], co, pos[co][1], pos[co][2]] = sg[co]
    return d, (pos, sg)


def make_ops(case):
    """(data, other, bias or None, extra): the operands of shapes() for the case's reference kind"""
    rng = np.random.default_rng(case.seed())
    sd, so, _ = case.shapes()
    g = GEOM[case.which]
    bias = None
    if case.ref == 'int':
        v = int_range(case.K())
        data, other = _ints(rng, sd, v), _ints(rng, so, v)
        if case.entry == 'fwd':
            bias = _ints(rng, 32, BIAS_MAX)
        return data, other, bias, v
    if case.ref == 'sel':
        data = full_significand_matrix(rng, sd)
        if case.entry == 'wgrad':
            other, extra = _sel_dout(rng, case.which, case.B, case.tout())
        else:
            other, extra = _sel_filter(rng, case.which, case.entry == 'dgrad')
        if case.entry == 'fwd':
            bias = np.zeros(32, np.float32)
        return data, other, bias, extra
    # the training ranges: conv1 reads a normalised spectrogram, conv2 the clipped-ReLU output of conv1; d(out) is small and
    # same-signed in places (tests/test_kernels_gpu.py test_conv_wgrad_families_agree)
    k = g.cin * g.kf * g.kt
    x = (lambda s: rng.standard_normal(s)) if case.which == 1 else (lambda s: rng.random(s) * 20.0)
    dy = lambda s: rng.standard_normal(s) * 1e-3 + 2e-4        # noqa: E731
    w = lambda s: rng.standard_normal(s) / np.sqrt(k)           # noqa: E731
    if case.entry == 'fwd':
        data, other, bias = x(sd), w(so), rng.standard_normal(32).astype(np.float32)
    elif case.entry == 'dgrad':
        data, other = dy(sd), w(so)
    else:
        data, other = x(sd), dy(so)
    return data.astype(np.float32), other.astype(np.float32), bias, None


def sel_reference(case, data, extra):
    """what the selection cases must give, bit for bit: a gather, no arithmetic.  wgrad: (d_w, d_bias)."""
    g = GEOM[case.which]
    _, _, sr = case.shapes()
    if case.entry == 'wgrad':
        pos, sg = extra
        xp = padded(case.which, data, np.float32)
        dw = np.stack([sg[co] * xp[b, :, g.sf * d:g.sf * d + g.kf, g.st * t:g.st * t + g.kt] for co, (b, d, t) in enumerate(pos)])
        return dw, sg.copy()
    ci, taps, sg = extra
    out = np.zeros(sr, np.float32)
    if case.entry == 'fwd':
        xp = padded(case.which, data, np.float32)
        for co in range(32):
            out[:, co] = sg[co] * _win(case.which, xp, taps[co][0], taps[co][1], sr[3])[:, ci[co]]
    else:
        t = data.shape[3]
        for co in range(32):
            kf, kt = taps[co]
            out[:, ci[co], kf:kf + 41:2, kt:kt + t] = sg[co] * data[:, co]
    return out


def tamper_tap(case, extra):
    """the filter tap the CPU test drops, shifts or doubles: one that a selection case's channel 0 uses (any tap moves an
    integer case; a tap no channel selects would leave a selection case as it is)"""
    g = GEOM[case.which]
    if case.ref == 'sel' and case.entry != 'wgrad':
        return extra[1][0]
    if case.ref == 'sel':                               # a time tap that meets a real input column from channel 0's position
        t0 = extra[0][0][2]
        kt = [k for k in range(g.kt) if g.padt <= g.st * t0 + k < g.padt + case.T][-1]
        return (g.kf - 1, kt)
    return (g.kf - 1, 8)
