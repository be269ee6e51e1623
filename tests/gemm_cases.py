"""Cases, operand builders, references and a mirror of the launcher's form choice for the GEMM edge suite.

Pure numpy, no GPU: tests/test_gemm_cases_cpu.py proves on the CPU that the cases are what they claim to be,
tests/test_gemm_edges_gpu.py runs them through ds2_gemm_f32 and ds2_gemm_f32_tn_group.

References (none of the first two needs a tolerance):
  'int'   small-integer operands with 2 max|a| max|b| K < 2^24: every partial product of every split term and every partial
          sum in any order is an exactly representable integer (the factor 2 covers bf16(a) rounding up to the next power of
          two), so the result is exact in every kernel family and under float atomics;
  'selA'  A arbitrary fp32 (24-bit significands, exponents over [2^-100, 2^100)), op(B) with exactly one +-1 per column at
          row pi(n): C[m, n] = +-op(A)[m, pi(n)] exactly ('selB': the roles exchanged);
  'fp64'  general operands against an fp64 product under |c - ref| <= (K + S + 2) 2^-24 (|a| @ |b|).

Every operand lives inside a flat buffer of its own (Embedded): a front guard, pad columns behind every row and a tail guard
of 48 ld + 64 floats, all NaN for A and B and a finite sentinel for C.  The tail guard is longer than the furthest read the
kernels issue behind an operand (two slabs of prefetch plus a partial slab = 47 rows), so no case can leave its own
allocations."""
import zlib
from dataclasses import dataclass

import numpy as np

BM = BN = 128
BK = 16
FRONT = 64                                   # floats in front of every view (a multiple of 4: keeps 16-byte alignment)
SENTINEL = 0x5A5A5A5A                        # as fp32: 1.54e16, finite
TR = ('N', 'T')


def cdiv(a, b):
    return (a + b - 1) // b


def tail_guard(ld):
    return 48 * ld + 64


# --------------------------------------------------------------------------------------------- embedded views
class Embedded:
    """A rows x cols row-major view with row pitch ld, `offset` floats (0..3) off 16-byte alignment, inside a flat fp32
    buffer whose every other float is `fill`: 'nan' or 'sentinel'."""

    def __init__(self, rows, cols, ld, offset=0, fill='nan'):
        assert rows >= 1 and cols >= 1 and ld >= cols and 0 <= offset < 4
        self.rows, self.cols, self.ld, self.offset, self.fill = rows, cols, ld, offset, fill
        self.start = FRONT + offset
        self.span = (rows - 1) * ld + cols
        self.tail = tail_guard(ld)
        self.size = cdiv(self.start + self.span + self.tail, 4) * 4
        self.buf = np.empty(self.size, np.float32)
        if fill == 'nan':
            self.buf[:] = np.nan
        else:
            self.buf.view(np.uint32)[:] = SENTINEL

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return np.lib.stride_tricks.as_strided(buf[self.start:], (self.rows, self.cols), (4 * self.ld, 4))

    def put(self, mat):
        self.view()[...] = mat
        return self

    def inside(self):
        """bool mask over the buffer: True for the floats of the view."""
        mask = np.zeros(self.size, bool)
        np.lib.stride_tricks.as_strided(mask[self.start:], (self.rows, self.cols), (self.ld, 1))[...] = True
        return mask

    def outside_intact(self, buf):
        """every float outside the view still holds the fill's bit pattern (sentinel buffers only)"""
        assert self.fill == 'sentinel'
        return bool(np.all(np.asarray(buf).view(np.uint32)[~self.inside()] == SENTINEL))


def ld_of(width, mode):
    """row pitch for a view `width` floats wide: 'tight' = width, 'pad4' = the next multiple of 4 plus 4 (pad columns, 16-byte
    rows), 'odd' = the next multiple of 4 plus 1 (for a width that is a multiple of 4: width + 1), 'pad1' = width + 1,
    'plus4' = width + 4."""
    if mode == 'tight':
        return width
    if mode == 'pad4':
        return cdiv(width, 4) * 4 + 4
    if mode == 'odd':
        return cdiv(width, 4) * 4 + 1
    if mode == 'pad1':
        return width + 1
    if mode == 'plus4':
        return width + 4
    raise ValueError(mode)


# --------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    section: str
    ta: int
    tb: int
    m: int
    n: int
    k: int
    split_k: int = 1
    beta: int = 0
    ref: str = 'int'
    lda: str = 'pad4'
    ldb: str = 'pad4'
    ldc: str = 'tight'
    a_off: int = 0
    b_off: int = 0
    families: tuple = (0, 6, 9)
    sk: str = ''            # '': m as given; 'half+1': m = 128 (slots / 2 + 1) + m; '2s-1': m = 128 ((2 slots - 1) // 3) + m
    poison: str = ''        # non-finite cases: 'nanA', 'infA', 'nanB', 'infB'
    odd_lda_family: int = -1    # stream-K section: in this family the case is run with lda = 'odd' (which lands in family 0's forms)

    @property
    def name(self):
        s = '%s-%s%s-%s%dx%dx%d' % (self.section, TR[self.ta], TR[self.tb], self.sk and self.sk + '+', self.m, self.n, self.k)
        s += '-s%d-b%d-%s' % (self.split_k, self.beta, self.ref)
        s += '-%s.%s.%s' % (self.lda, self.ldb, self.ldc)
        if self.a_off or self.b_off:
            s += '-off%d%d' % (self.a_off, self.b_off)
        if self.poison:
            s += '-' + self.poison
        return s

    def dims(self, slots=512):
        m = self.m
        if self.sk == 'half+1':
            m = BM * (slots // 2 + 1) + self.m
        elif self.sk == '2s-1':
            m = BM * ((2 * slots - 1) // 3) + self.m
        return m, self.n, self.k

    def lds(self, slots=512, family=None):
        """(lda, ldb, ldc) in floats"""
        m, n, k = self.dims(slots)
        lda = 'odd' if (family is not None and family == self.odd_lda_family) else self.lda
        return (ld_of(m if self.ta else k, lda), ld_of(k if self.tb else n, self.ldb), ld_of(n, self.ldc))

    def seed(self):
        return zlib.crc32(self.name.encode())


@dataclass(frozen=True)
class GroupCase:
    section: str
    ms: tuple
    n: int
    k: int
    lda: tuple = ()         # one ld mode per problem; () = 'pad4' for all
    ldb: str = 'pad4'
    ldc: str = 'tight'
    share_b: bool = False
    ref: str = 'int'
    families: tuple = (0, 6, 9)

    @property
    def name(self):
        s = '%s-%s-n%d-k%d-%s' % (self.section, 'x'.join(map(str, self.ms)), self.n, self.k, self.ref)
        s += '-%s.%s.%s' % ('/'.join(self.lda) or 'pad4', self.ldb, self.ldc)
        return s + ('-sharedB' if self.share_b else '')

    def lds(self):
        """per problem (lda, ldb, ldc)"""
        modes = self.lda or ('pad4',) * len(self.ms)
        return [(ld_of(m, modes[p]), ld_of(self.n, self.ldb), ld_of(self.n, self.ldc)) for p, m in enumerate(self.ms)]

    def seed(self):
        return zlib.crc32(self.name.encode())


ALL_TR = [(0, 0), (0, 1), (1, 0), (1, 1)]
EMBED_SHAPES = [(16, 1), (17, 1), (40, 1), (100, 1), (333, 1), (1000, 3), (1000, 4), (40, 4), (640, 0), (1283, 0)]  # (K, split_k)
EDGE_M = [1, 3, 127, 128, 129, 131]
EDGE_N = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 192, 193, 257]
SLAB_K = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 80]
AUTO_K = [511, 512, 639, 640, 2047, 2048, 10247]


def embedded_cases():
    """section 2: the integer reference through padded, NaN-surrounded operands and a sentinel-surrounded C"""
    return [Case('embed', ta, tb, 130, 161, k, split_k=sk, beta=beta, ldc=ldc)
            for ta, tb in ALL_TR for k, sk in EMBED_SHAPES for ldc in ('tight', 'plus4', 'pad1') for beta in (0, 1)]


def tile_edge_cases():
    out = []
    for ta, tb in ALL_TR:
        for lay in ('tight', 'pad4'):           # tight: "plain contiguous"; pad4: 16-byte rows, which the vector and split forms need
            out += [Case('edgeM', ta, tb, m, 161, 48, lda=lay, ldb=lay) for m in EDGE_M]
            out += [Case('edgeN', ta, tb, 129, n, 48, lda=lay, ldb=lay) for n in EDGE_N]
    return out


def slab_cases():
    return [Case('slabs', ta, tb, 129, 160, k, lda=lay, ldb=lay) for ta, tb in ALL_TR for lay in ('tight', 'pad4') for k in SLAB_K]


def fallback_cases():
    out = []
    for ta, tb in ALL_TR:
        kw = dict(families=(6, 9))
        out.append(Case('fallback', ta, tb, 130, 161, 48, lda='odd', **kw))          # lda = K + 1 for a K-contiguous A
        out.append(Case('fallback', ta, tb, 130, 161, 48, ldb='odd', **kw))
        out.append(Case('fallback', ta, tb, 130, 161, 48, a_off=1, **kw))
        out.append(Case('fallback', ta, tb, 130, 161, 48, b_off=1, **kw))
        out.append(Case('fallback', ta, tb, 130, 161, 24, **kw))                     # K % 16: TN stays in the split family
        out.append(Case('fallback', ta, tb, 130, 161, 20, **kw))
        out.append(Case('fallback', ta, tb, 130, 161, 22, **kw))                     # K % 4: out of the vector f32 form too
        out.append(Case('fallback', ta, tb, 130, 161, 1000, split_k=3, lda='odd', **kw))     # and with atomics
    return out


def auto_split_cases():
    out = []
    for ta, tb in ((1, 0), (0, 1)):
        for beta in (0, 1):
            out += [Case('auto', ta, tb, 128, 128, k, split_k=0, beta=beta, families=(0, 6)) for k in AUTO_K]
            out += [Case('auto', ta, tb, 128 * 23, 128 * 23, k, split_k=0, beta=beta, families=(0, 6)) for k in (512, 2048)]
    return out


def stream_k_cases():
    """family 0, and family 6 with lda % 4 != 0 (which lands in family 0's forms); M is sized from the device's slots"""
    kw = dict(families=(0, 6), odd_lda_family=6)
    out = [Case('streamk', ta, tb, 0, 256, 384, sk='half+1', **kw) for ta, tb in ALL_TR]
    for ta, tb in ((1, 0), (0, 1)):
        out += [
            Case('streamk', ta, tb, 0, 256, 389, sk='half+1', **kw),
            Case('streamk', ta, tb, -3, 256, 384, sk='half+1', **kw),
            Case('streamk', ta, tb, -4, 256, 384, sk='half+1', **kw),
            Case('streamk', ta, tb, 0, 225, 384, sk='half+1', **kw),
            Case('streamk', ta, tb, 0, 384, 256, sk='2s-1', **kw),
            Case('streamk', ta, tb, 0, 256, 384, sk='half+1', ldc='pad4', **kw),
            Case('streamk', ta, tb, 0, 256, 384, sk='half+1', beta=1, **kw),
            Case('streamk', ta, tb, 0, 256, 240, sk='half+1', **kw),
        ]
    return out


def selection_cases():
    return [Case('select', ta, tb, m, n, k, split_k=sk, ref=ref)
            for ta, tb in ALL_TR for m, n, k, sk in ((130, 161, 100, 1), (129, 800, 800, 1), (130, 161, 333, 3))
            for ref in ('selA', 'selB')]


def fp64_cases():
    return [Case('fp64', ta, tb, 130, 161, k, split_k=sk, ref='fp64')
            for ta, tb in ALL_TR for k, sk in ((16, 1), (32, 1), (48, 1), (1000, 3))]


STAT_CASES = [Case('stat', 1, 0, 1029, 800, 1283, split_k=0, ref='fp64'), Case('stat', 0, 0, 777, 640, 800, ref='fp64')]


def nonfinite_cases():
    return [Case('nonfinite', ta, tb, 130, 161, k, poison=p)
            for ta, tb in ((0, 1), (1, 0)) for k in (100, 96) for p in ('nanA', 'infA', 'nanB', 'infB')]


GROUP_MS = [(130,), (400, 200), (1, 129, 256), (400, 200, 400, 200)]


def group_cases():
    out = [GroupCase('group', ms, n, k) for ms in GROUP_MS for n in (200, 32, 129) for k in (100, 511, 512, 1234)]
    out.append(GroupCase('group-cap', (128,), 128, 10247))
    out.append(GroupCase('group-mixedlda', (130, 200, 64), 200, 512, lda=('pad4', 'odd', 'pad4')))
    out.append(GroupCase('group-mixedlda', (130, 200), 129, 100, lda=('odd', 'pad4')))
    out.append(GroupCase('group-sharedB', (400, 200, 400, 200), 200, 1234, share_b=True))
    out.append(GroupCase('group-sharedB', (1, 129, 256), 129, 100, share_b=True))
    out += [GroupCase('group-ldc', (400, 200), 200, k, ldc=ldc) for k in (100, 1234) for ldc in ('pad4', 'pad1')]
    out += [GroupCase('group-select', (130, 200), 161, 333, ref=ref) for ref in ('selA', 'selB')]
    return out


def single_cases():
    return (embedded_cases() + tile_edge_cases() + slab_cases() + fallback_cases() + auto_split_cases() + stream_k_cases() +
            selection_cases() + fp64_cases() + STAT_CASES + nonfinite_cases())


# --------------------------------------------------------------------------------------------- operand builders
def int_ranges(k):
    """(max|a|, max|b|) with 2 max|a| max|b| K < 2^24"""
    for amax, bmax, kmax in ((1023, 15, 546), (511, 3, 4800), (511, 1, 16384)):
        if k <= kmax:
            return amax, bmax
    raise ValueError('K = %d is beyond the integer builder' % k)


def int_matrix(rng, shape, vmax):
    return rng.integers(-vmax, vmax + 1, size=shape).astype(np.float32)


def full_significand_matrix(rng, shape):
    """fp32 values with all 24 significand bits in use (odd integer significands) and exponents over [2^-100, 2^100): every
    bf16 term of such a value is a normal number or zero, the third one is non-zero for nearly all of them (the last bit has
    to live somewhere), and no element is 0.0 or -0.0."""
    mant = (rng.integers(1 << 23, 1 << 24, size=shape) | 1).astype(np.float64)
    expo = rng.integers(-100, 100, size=shape)
    sign = rng.choice(np.array([-1.0, 1.0]), size=shape)
    return (sign * np.ldexp(mant, expo - 23)).astype(np.float32)


def boundaries(k, kper):
    """the k on both sides of every slab boundary and every split boundary, and both ends"""
    ks = {0, k - 1}
    for step in (BK, kper):
        for b in range(step, k, step):
            ks.update((b - 1, b))
    return sorted(ks)


def selection_rows(rng, ncols, k, kper):
    """pi: column -> the k it selects.  Every k when ncols >= K; otherwise both sides of every slab / split boundary and both
    ends, then other k drawn at random."""
    if ncols >= k:
        pi = np.concatenate([np.arange(k), rng.integers(0, k, size=ncols - k)])
    else:
        must = np.array(boundaries(k, kper))
        assert len(must) <= ncols, 'not enough columns for every boundary'
        rest = np.setdiff1d(np.arange(k), must)
        pi = np.concatenate([must, rng.choice(rest, size=ncols - len(must), replace=False)])
    return rng.permutation(pi)


def selection_matrix(rng, k, ncols, kper):
    """(K x ncols matrix with one +-1 per column, pi, signs)"""
    pi = selection_rows(rng, ncols, k, kper)
    sg = rng.choice(np.array([-1.0, 1.0], np.float32), size=ncols)
    sel = np.zeros((k, ncols), np.float32)
    sel[pi, np.arange(ncols)] = sg
    return sel, pi, sg


def kper_of(k, split_k):
    kper = cdiv(cdiv(k, max(split_k, 1)), BK) * BK
    return max(kper, BK)


def make_ops(ref, m, n, k, seed, kper=BK):
    """op(A) (m x k) and op(B) (k x n) for one reference kind, plus what the reference needs"""
    rng = np.random.default_rng(seed)
    if ref == 'int':
        amax, bmax = int_ranges(k)
        return int_matrix(rng, (m, k), amax), int_matrix(rng, (k, n), bmax), None
    if ref == 'selA':
        sel, pi, sg = selection_matrix(rng, k, n, kper)
        return full_significand_matrix(rng, (m, k)), sel, (pi, sg)
    if ref == 'selB':
        sel, pi, sg = selection_matrix(rng, k, m, kper)
        return np.ascontiguousarray(sel.T), full_significand_matrix(rng, (k, n)), (pi, sg)
    if ref == 'fp64':
        return rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32), None
    raise ValueError(ref)


def reference(ref, opa, opb, extra=None):
    """the expected op(A) op(B): exact for 'int' (fp64 holds every integer below 2^53; equal to the int64 product) and for the
    selections (a gather, no arithmetic), fp64 for 'fp64'"""
    if ref == 'selA':
        pi, sg = extra
        return opa[:, pi] * sg[None, :]
    if ref == 'selB':
        pi, sg = extra
        return opb[pi, :] * sg[:, None]
    return opa.astype(np.float64) @ opb.astype(np.float64)


def fp64_bound(opa, opb, k, pieces):
    """|c - ref| <= (K + S + 2) 2^-24 (|a| @ |b|): one rounding of relative size <= 2^-24 per accumulated term and per
    atomically added piece (S of them, 0 without atomics), each on a partial sum bounded by sum |a||b|; the split products are
    within 2^-24 of a b (csrc/split_bf16.h, tests/test_split_cpu.py)."""
    return (k + pieces + 2) * 2.0 ** -24 * (np.abs(opa).astype(np.float64) @ np.abs(opb).astype(np.float64))


def stored(op, trans):
    """the row-major matrix the library is handed for op(X) = X or X^T"""
    return np.ascontiguousarray(op.T) if trans else op


def c_prefill(rng, m, n):
    """integers the beta = 1 / accumulate cases start from (small against 2^23: the sum stays exact)"""
    return rng.integers(-1000, 1001, size=(m, n)).astype(np.float32)


# --------------------------------------------------------------------------------------------- the launcher's choice
@dataclass(frozen=True)
class Form:
    kernel: str             # e.g. 'bf16x6-TN', 'f32-vec-NT', 'f32-novec-NN', 'v2-vec-TN', 'group-bf16x6', 'group-f32-vec'
    atomic: bool
    zero: str               # 'none', 'linear' (ldc == N), '2d'
    bodies: tuple           # edge-tile bodies that run: 1 (<= 32 columns), 2 (<= 64), 0 (full); () for the v2 kernel
    nsplit: int             # pieces added per output (1 without atomics; for the stream-K form a nominal 2: the runs that share a tile)
    stream_k: bool = False

    def family(self):
        return self.kernel.split('-')[0]


def _bodies(n):
    tn = cdiv(n, BN)
    last = n - (tn - 1) * BN
    b = {1 if last <= 32 else 2 if last <= 64 else 0}
    if tn > 1:
        b.add(0)
    return tuple(sorted(b))


def auto_split(tiles, k, family):
    split_k = 1
    if (tiles < 512 and k >= 512) or (tiles < 2048 and k >= 2048):
        target = 1024 if family != 0 else 8192
        split_k = target // tiles
        max_split = k // 320 if k // 320 > 1 else 1
        split_k = min(split_k, max_split, 32)
    return max(split_k, 1)


def expected_form(case, family, slots=512):
    """Which kernel ds2_gemm_f32 / ds2_gemm_f32_tn_group launch for a case: a line-by-line mirror of launch() and of the group
    launcher in csrc/gemm.hip (split_k rule, the split family's conditions, the stream-K condition, kper / nsplit, vec,
    zero_rows).  The GPU suite asserts results only, never which kernel ran: if this mirror drifts from the launcher it can
    understate coverage, it cannot hide a failure.

    (launch() only starts gemm_f32_v2_kernel under the very condition that gives it stream-K pieces -- `hybrid` repeats the outer
    test -- so a v2 launch without pieces does not exist; every v2 launch has data-parallel and stream-K workgroups.)"""
    if isinstance(case, GroupCase):
        return _expected_group(case, family)
    m, n, k = case.dims(slots)
    lda, ldb, ldc = case.lds(slots, family)
    ak, bk = not case.ta, bool(case.tb)                       # K-contiguous A / B
    tr = TR[case.ta] + TR[case.tb]
    tm, tn = cdiv(m, BM), cdiv(n, BN)
    tiles = tm * tn
    split_k = case.split_k
    if split_k == 0:
        split_k = auto_split(tiles, k, family)
    split_k = max(split_k, 1)
    aligned = lda % 4 == 0 and ldb % 4 == 0 and case.a_off % 4 == 0 and case.b_off % 4 == 0
    zero = 'linear' if ldc == n else '2d'
    if family != 0 and aligned and ((not ak and not bk) or k % BK == 0):
        kper = kper_of(k, split_k)
        nsplit = cdiv(k, kper)
        atomic = nsplit > 1
        return Form('bf16x%d-%s' % (family, tr), atomic, zero if atomic and case.beta == 0 else 'none', _bodies(n), nsplit)
    vec = aligned and ((not ak and not bk) or k % 4 == 0)
    nslab = cdiv(k, BK)
    if split_k == 1 and tiles > slots and tiles % slots != 0 and nslab >= 16 and case.beta == 0:
        return Form('v2-%s-%s' % ('vec' if vec else 'novec', tr), True, zero, (), 2, stream_k=True)
    kper = kper_of(k, split_k)
    nsplit = cdiv(k, kper)
    atomic = nsplit > 1
    return Form('f32-%s-%s' % ('vec' if vec else 'novec', tr), atomic, zero if atomic and case.beta == 0 else 'none', _bodies(n),
                nsplit)


def _expected_group(case, family, accumulate=False):
    lds = case.lds()
    tn = cdiv(case.n, BN)
    vec = all(lda % 4 == 0 and ldb % 4 == 0 for lda, ldb, _ in lds)          # (the test's pointers are 16-byte aligned)
    tot_tiles = sum(cdiv(m, BM) * tn for m in case.ms)
    split_k = 1
    if tot_tiles < 512 and case.k >= 512:
        target = 1024 if family != 0 else 3072
        split_k = target // tot_tiles
        max_split = case.k // 320 if case.k // 320 > 1 else 1
        split_k = max(min(split_k, max_split, 32), 1)
    kper = kper_of(case.k, split_k)
    nsplit = cdiv(case.k, kper)
    if vec and family in (6, 9):
        kernel = 'group-bf16x%d' % family
    else:
        kernel = 'group-f32-%s' % ('vec' if vec else 'novec')
    zero = 'none' if accumulate else ('linear' if lds[0][2] == case.n else '2d')
    return Form(kernel, True, zero, _bodies(case.n), nsplit)


def pieces_per_output(form):
    """S of the fp64 bound: atomically added pieces per output"""
    return form.nsplit if form.atomic else 0
