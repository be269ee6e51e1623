"""Cases, layout helpers, operand builders, per-task float64 references and a mirror of the launchers' form choice for the
segmented BatchNorm edge suite (csrc/bn_seg.hip: ds2_bn1d_seg_stats / _apply / _bwd, the per-task head BatchNorm of
MultiTaskModel).

Pure numpy, no GPU, no torch: tests/test_bn_seg_cases_cpu.py proves on the CPU that the cases are what they claim to be,
tests/test_bn_seg_edges_gpu.py runs them through the C ABI.  Everything that tests/bn_cases.py already provides is imported
from there: Flat, the float64 references, the bounds and the ratios.  What is new here is the layout (task g owns the batch
columns [bounds[g], bounds[g + 1]) of the interleaved (T, B, F) tensors, and the contiguous (T, B_g, F) block at row
T * bounds[g] of the packed (T B, F) ones), the per-task pointer arrays and the dispatch.

Operands.  As in bn_cases: every tensor, and every task's gamma / beta / running_mean / running_var / dgamma / dbeta, lives in
a Flat buffer of its own at a chosen offset off 16-byte alignment, inputs surrounded by NaN, outputs by a sentinel.  The
workspace is exactly G * ds2_bn_ws_bytes(F) bytes of NaN with a sentinel guard behind it; both `part` (G F NPART 2 doubles)
and `coef` (G 2 F floats) fit inside it, with nothing to spare.

Values.  Every task draws from a distribution of its own: task g's x has mean 5 s_g / 3 and deviation s_g with
s_g = 3 * 2^(g - G // 2), its packed gradient has deviation 2^(g - G // 2), gamma lies in [0.5, 1.5] * 2^(g - G // 2), beta
in [-1, 1] + 4 g, running_mean in [0, 2] + 3 g, running_var in [0.5, 2] * 4^(g - G // 2).  A row or a parameter taken from
the neighbouring task is then off by a factor of two or more: far outside every bound.  G = 1 gives exactly the
distribution of bn_cases' sequence flavour.  A task of 2 to 29 rows gets bn_cases' per-channel standardised draw.
kind = 'count': integers.  Task g's x is +-(4 g + 1 .. 4 g + 4) (xa = +-(4 g + 1 .. 2) and xb = +-(1 .. 2) of the same sign
when there are two), its gradient +-(3 g + 1 .. 3 g + 3), gamma = 1, beta = 10 + g, the given mean_invstd = (0, 1): every
sum is an integer below 2^24, so mean, y, dgamma and dbeta are fixed bit for bit and invstd within 1 ulp.

Roundings, counted in csrc/bn_seg.hip (u = 2^-24).  Per task the three kernels evaluate, operation for operation, the
expressions of bn.hip's sequence flavour, so the constants of bn_cases hold unchanged and nothing here is fitted:
  bn1d_seg_reduce_kernel   thread (p, ry) of task g adds the task rows r = 4 p + ry + 256 j, at most n = ceil(T B_g / 256)
                           terms, in fp32; the four row lanes and the 64 partials are combined in fp64 and the result is
                           rounded once.  MODE 0: v = fl(xa + xb), s0 += v, s1 += v * v.  MODE 1: s0 += gr,
                           s1 += gr * (v - mu) * is, which C++ groups as (gr * (v - mu)) * is: one subtraction and one
                           product inside the term, the last product fused into the accumulation in the 16-byte form --
                           the two roundings inside a term of bn_cases' (n + 2) u sum |term|, under the same first-order
                           reading (an unfused scalar form has one rounding more inside a term; a thread with a single term
                           adds nothing to 0 and stays at three).  fl(xa + xb) is the ABSOLUTE u |x| that bwd_ref adds to
                           dgamma with xb_rounds.  The count is T B_g, a double.
  bn1d_seg_apply_kernel    (fl(xa + xb) - mu) * (gamma * is) + beta: five operations, K = 5 as bn1d_apply.
  bn1d_seg_bwd_apply_kernel  gamma * is * (dxf - cf0 - ((fl(xa + xb) - mu) * is) * cf1): eight operations with xb, seven
                           without, K = 8 / 7 as bn1d_bwd; cf = float(sum / count), one rounding each, inside the
                           b(dbeta) / N and b(dgamma) / N that bwd_ref adds.
  finalize                 fp64 throughout, as bn.hip's: mean, var = E[x^2] - mean^2 clamped at 0, the running buffers
                           updated in fp64 and rounded once, eval's invstd rounded once.
So each task's reference and bounds are stats_ref / running_ref / eval_ref / apply_ref(clamp=False) /
bwd_ref(clamp=False, xb_rounds=xb) on its own rows with n_run = ceil(T B_g / 256).
"""
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from tests import bn_cases as bc
from tests.bn_cases import EPS, MOMENTUM, NPART, U, Flat, cdiv   # noqa: F401  (re-exported for the two test modules)

ENTRIES = ('seg_stats', 'seg_apply', 'seg_bwd')
SEG_MAX = 8
PER_TASK = ('gamma', 'beta', 'rm', 'rv', 'dgamma', 'dbeta')


def ws_floats(F, G):
    """G * ds2_bn_ws_bytes(F) / 4"""
    return G * bc.ws_floats(F)


def part_floats(F, G):
    """the fp64 partials at the front of the workspace, in floats; coef (G, 2, F) floats follow them"""
    return G * F * NPART * 2 * 2


# --------------------------------------------------------------------------------------------- the launchers' choice
def form(entry, off, F, G):
    """'vec' or 'scalar': which kernels an entry point launches, from the host code of csrc/bn_seg.hip.  off: operand name ->
    offset in floats off 16-byte alignment (missing = 0; a NULL xb counts as aligned: al16(NULL)).  Each entry looks at
    F % 4 and at its own set of pointers; one misaligned gamma or beta of one task switches the whole launch."""
    def aligned(*names):
        return all(off.get(nm, 0) % 4 == 0 for nm in names)

    def per(stem):
        return [stem + str(g) for g in range(G)]
    if entry == 'seg_stats':
        ok = aligned('xa', 'xb')
    elif entry == 'seg_apply':
        ok = aligned('xa', 'xb', 'y', 'mi', *per('gamma'), *per('beta'))
    elif entry == 'seg_bwd':
        ok = aligned('xa', 'xb', 'dxf', 'dy', 'mi', *per('gamma'))
    else:
        raise ValueError(entry)
    return 'vec' if F % 4 == 0 and ok else 'scalar'


# --------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Seg:
    """x = xa (+ xb), (T, B, F) interleaved; task g owns the batch columns [bounds[g], bounds[g + 1]).  off: ((operand,
    offset), ...) with the operands xa, xb, y, mi, dxf, dy and per task gamma<g>, beta<g>, rm<g>, rv<g>, dgamma<g>, dbeta<g>.
    running: True (every task has running buffers), False (none: both host arrays NULL) or a tuple of booleans per task (a
    task without passes NULL in both host arrays at its index)."""
    section: str
    T: int
    bounds: tuple
    F: int
    off: tuple = ()
    kind: str = 'fp64'
    xb: bool = True
    running: object = True
    bump: int = 0

    @property
    def G(self):
        return len(self.bounds) - 1

    @property
    def B(self):
        return self.bounds[-1]

    def bg(self, g):
        return self.bounds[g + 1] - self.bounds[g]

    def rows(self, g):
        return self.T * self.bg(g)

    def n_run(self, g):
        return cdiv(self.rows(g), 4 * NPART)

    def has_running(self, g):
        return self.running[g] if isinstance(self.running, tuple) else bool(self.running)

    @property
    def name(self):
        s = '%s-T%d-b%s-F%d-%s' % (self.section, self.T, '.'.join(str(b) for b in self.bounds), self.F, self.kind)
        s += ''.join('-%s%d' % kv for kv in self.off)
        s += '' if self.xb else '-noxb'
        if isinstance(self.running, tuple):
            s += '-run' + ''.join(str(int(r)) for r in self.running)
        elif not self.running:
            s += '-norun'
        return s

    def offs(self):
        o = dict(self.off)
        if not self.xb:
            o.pop('xb', None)
        return o

    def forms(self):
        o = self.offs()
        return {e: form(e, o, self.F, self.G) for e in ENTRIES}

    def seed(self):
        return zlib.crc32(self.name.encode()) + self.bump

    def task(self, g):
        """task g as a single-task sequence case: bn_cases' references, bounds and ratios apply to it as they are"""
        return bc.Seq('task%d' % g, self.rows(g), self.F, kind=self.kind, xb=self.xb, running=self.has_running(g))


def check(case):
    assert 1 <= case.G <= SEG_MAX and case.bounds[0] == 0 and all(case.bg(g) >= 1 for g in range(case.G))
    assert not isinstance(case.running, tuple) or len(case.running) == case.G
    known = {'xa', 'xb', 'y', 'mi', 'dxf', 'dy'} | {s + str(g) for s in PER_TASK for g in range(case.G)}
    assert set(dict(case.off)) <= known, case.name
    return case


# --------------------------------------------------------------------------------------------- layouts
def task_rows(case, a, g):
    """task g's rows of an interleaved (T, B, F) array as (T B_g, F), in the kernel's own row order r = t * B_g + (b - b0)"""
    b0, b1 = case.bounds[g], case.bounds[g + 1]
    return np.ascontiguousarray(np.asarray(a).reshape(case.T, case.B, case.F)[:, b0:b1]).reshape(case.rows(g), case.F)


def task_cm(case, a, g):
    """... as a channel-major (F, T B_g) float64 array"""
    return np.ascontiguousarray(task_rows(case, a, g).astype(np.float64).T)


def put_task_cm(case, out, g, cm):
    """the inverse of task_cm: write a channel-major (F, T B_g) array into task g's columns of the interleaved `out`"""
    b0, b1 = case.bounds[g], case.bounds[g + 1]
    out.reshape(case.T, case.B, case.F)[:, b0:b1] = np.asarray(cm).T.reshape(case.T, b1 - b0, case.F)
    return out


def packed_block(case, packed, g):
    """task g's block of a packed (T B, F) array: rows [T bounds[g], T bounds[g + 1]), a contiguous (T B_g, F)"""
    return np.asarray(packed).reshape(case.T * case.B, case.F)[case.T * case.bounds[g]:case.T * case.bounds[g + 1]]


def pack(case, a):
    """interleaved (T, B, F) -> packed (T B, F)"""
    return np.concatenate([task_rows(case, a, g) for g in range(case.G)], 0)


def unpack(case, packed):
    """packed (T B, F) -> interleaved (T, B, F)"""
    out = np.empty((case.T, case.B, case.F), np.asarray(packed).dtype)
    for g in range(case.G):
        put_task_cm(case, out, g, packed_block(case, packed, g).T)
    return out


# --------------------------------------------------------------------------------------------- the table
TWO = (0, 3, 7)                             # T = 37: 111 and 148 rows, 259 in all
WIDE = (0, 4, 10)                           # T = 17: 68 and 102 rows, 170 in all (544 kB at F = 800)
ROWS = ((1, (0, 1, 3, 6)), (51, (0, 5, 6)), (64, (0, 4, 5)), (257, (0, 1, 3)), (171, (0, 3, 4)))
ONES8 = tuple(range(9))
UNEVEN8 = (0, 1, 3, 4, 8, 9, 12, 14, 17)
NON_DECIDING = tuple((s + str(g), o) for g in (0, 1) for s, o in (('rm', 1), ('rv', 2), ('dgamma', 3), ('dbeta', 1)))


def seg_cases():
    out = []
    # quad-column block edges of the 16-byte forms: 9 / 63 / 64 / 65 / 200 quads
    out += [Seg('F4', 37, TWO, f) for f in (36, 252, 256, 260)] + [Seg('F4', 17, WIDE, 800)]
    # scalar by F (64: the full block, 65: blockIdx.y = 1); 801 is with the cap
    out += [Seg('F', 37, TWO, f) for f in (1, 30, 63, 64, 65)]
    out += [Seg('F', 37, TWO, 64, off=(('xa', 1),))]                      # F = 64 is a multiple of four: scalar by an offset
    # scalar by offset at F % 4 == 0: one case per deciding operand
    out += [Seg('offset', 37, TWO, 260, off=((nm, o),)) for nm, o in (('xa', 1), ('xb', 2), ('y', 3), ('mi', 1), ('dxf', 2),
                                                                     ('dy', 3), ('gamma1', 1), ('beta0', 2))]
    out += [Seg('offset', 17, WIDE, 800, off=(('gamma1', 1),))]          # a view into the flat parameter buffer
    out += [Seg('offset', 37, TWO, 260, off=NON_DECIDING)]                # none of these decides
    # rows per task around the reduction's stride of 256: 1, 2, 3 / 255, 51 / 256, 64 / 257, 514 / 513, 171
    out += [Seg('rows', t, b, f) for t, b in ROWS for f in (30, 36)]
    # segment geometry
    out += [Seg('geom', 37, (0, 7), f) for f in (30, 36)]                 # G = 1
    out += [Seg('geom', 5, ONES8, f) for f in (30, 36)]                   # G = 8, one column each
    out += [Seg('geom', 3, UNEVEN8, f) for f in (30, 36)]                 # G = 8, uneven
    out += [Seg('geom', 9, (0, 6, 7, 13), f) for f in (30, 36)]           # one column between two wide tasks
    out += [Seg('geom', 9, (0, 1, 7, 8), f) for f in (30, 36)]            # one column first, one last
    # xb = NULL
    out += [Seg('noxb', 37, TWO, 260, xb=False), Seg('noxb', 37, TWO, 65, xb=False),
            Seg('noxb', 37, TWO, 260, off=(('xa', 1),), xb=False), Seg('noxb', 1, (0, 1, 3, 6), 36, xb=False)]
    # running buffers: none, mixed (all: every other case)
    out += [Seg('running', 37, TWO, 260, running=False), Seg('running', 37, TWO, 65, running=False),
            Seg('running', 9, (0, 6, 7, 13), 36, running=(True, False, True)),
            Seg('running', 37, TWO, 30, running=(False, True)),
            Seg('running', 5, ONES8, 36, running=(False, True, True, False, False, True, False, True))]
    # past the elementwise kernels' cap of 4096 blocks of 256
    out += [Seg('cap', 749, TWO, 800), Seg('cap', 437, (0, 1, 3), 801)]
    # exact: every row counted once, in its own task
    out += [Seg('once', 37, TWO, 260, kind='count'), Seg('once', 37, TWO, 65, kind='count'),
            Seg('once', 37, TWO, 260, off=(('xa', 1),), kind='count'),
            Seg('once', 37, TWO, 260, off=(('gamma1', 1),), kind='count'),
            Seg('once', 257, (0, 1, 3), 30, kind='count'), Seg('once', 257, (0, 1, 3), 36, kind='count'),
            Seg('once', 1, (0, 1, 3, 6), 36, kind='count'), Seg('once', 51, (0, 5, 6), 30, kind='count'),
            Seg('once', 5, ONES8, 36, kind='count'), Seg('once', 3, UNEVEN8, 30, kind='count'),
            Seg('once', 9, (0, 6, 7, 13), 36, kind='count'), Seg('once', 9, (0, 1, 7, 8), 30, kind='count'),
            Seg('once', 37, TWO, 36, kind='count', xb=False), Seg('once', 37, TWO, 30, kind='count', xb=False),
            Seg('once', 9, (0, 6, 7, 13), 36, kind='count', running=(True, False, True)),
            Seg('once', 37, TWO, 30, kind='count', running=False),
            Seg('once', 749, TWO, 800, kind='count'), Seg('once', 437, (0, 1, 3), 801, kind='count')]
    return [check(c) for c in out]


# cases for "a task's results do not depend on its neighbours" (bit for bit against a G = 1 launch of its columns)
ISOLATION = ['F4-T37-b0.3.7-F260-fp64', 'geom-T5-b0.1.2.3.4.5.6.7.8-F36-fp64', 'geom-T3-b0.1.3.4.8.9.12.14.17-F30-fp64',
             'rows-T257-b0.1.3-F36-fp64', 'offset-T37-b0.3.7-F260-fp64-xa1', 'geom-T9-b0.6.7.13-F36-fp64']
# shapes for "the same data aligned and with xa at offset 1"
BOTH_FORMS_SHAPES = [(51, (0, 5, 6), 36), (257, (0, 1, 3), 260)]
# cases for the chained pass through ds2hip.ops
CHAIN = [(17, WIDE, 800), (3, UNEVEN8, 30), (9, (0, 6, 7, 13), 36)]


# --------------------------------------------------------------------------------------------- operand builder
def scale(case, g):
    return 2.0 ** (g - case.G // 2)


def make(case, mi=None):
    """Everything one case needs: fp32 operands in the ABI's layouts, the given mean_invstd (G, 2F) (mi overrides it: a chained
    run hands apply and backward the statistics kernel's own output) and, per task, bn_cases' float64 references and bounds
    on the task's own rows (p.tasks[g], shaped like bn_cases.make's result for the single-task case case.task(g))."""
    rng = np.random.default_rng(case.seed())
    T, B, F, G = case.T, case.B, case.F, case.G
    xa = np.empty((T, B, F), np.float32)
    xb = np.empty((T, B, F), np.float32) if case.xb else None
    dxf = np.empty((T * B, F), np.float32)
    p = SimpleNamespace(case=case, tasks=[], gamma=[], beta=[], rm0=[], rv0=[])
    for g in range(G):
        rows, k = case.rows(g), scale(case, g)
        shape = (rows, F)
        b = None
        if case.kind == 'fp64':
            if case.xb:
                a = k * (2 * rng.standard_normal(shape) + 2)
                b = k * (2.2 * rng.standard_normal(shape) + 3)
            else:
                a = k * (3 * rng.standard_normal(shape) + 5)
            a = a.astype(np.float32)
            b = None if b is None else b.astype(np.float32)
            if 2 <= rows < 30:
                z = rng.standard_normal(shape)
                z = (z - z.mean(0, keepdims=True)) / z.std(0, keepdims=True)
                target = k * (5 + 3 * z)
                if b is None:
                    a = target.astype(np.float32)
                else:
                    b = (target - a).astype(np.float32)
            d = (k * rng.standard_normal(shape)).astype(np.float32)
            gamma = (k * rng.uniform(0.5, 1.5, F)).astype(np.float32)
            beta = (rng.uniform(-1, 1, F) + 4 * g).astype(np.float32)
        elif case.kind == 'count':
            sign = rng.choice([-1, 1], size=shape)
            if case.xb:
                a = (sign * (4 * g + rng.integers(1, 3, size=shape))).astype(np.float32)
                b = (sign * rng.integers(1, 3, size=shape)).astype(np.float32)
            else:
                a = (sign * (4 * g + rng.integers(1, 5, size=shape))).astype(np.float32)
            d = (rng.choice([-1, 1], size=shape) * (3 * g + rng.integers(1, 4, size=shape))).astype(np.float32)
            gamma, beta = np.ones(F, np.float32), np.full(F, 10 + g, np.float32)
        else:
            raise ValueError(case.kind)
        put_task_cm(case, xa, g, a.T)
        if case.xb:
            put_task_cm(case, xb, g, b.T)
        packed_block(case, dxf, g)[...] = d
        p.gamma.append(gamma)
        p.beta.append(beta)
        p.rm0.append((rng.uniform(0, 2, F) + 3 * g).astype(np.float32))
        p.rv0.append((k * k * rng.uniform(0.5, 2, F)).astype(np.float32))
    p.xa, p.xb, p.dxf = xa, xb, dxf

    x64 = xa.astype(np.float64) + (xb.astype(np.float64) if case.xb else 0.0)
    xabs = np.abs(xa.astype(np.float64)) + (np.abs(xb.astype(np.float64)) if case.xb else 0.0)
    p.mi = np.empty((G, 2 * F), np.float32)
    for g in range(G):
        t = SimpleNamespace(case=case.task(g), g=g, gamma=p.gamma[g], beta=p.beta[g], rm0=p.rm0[g], rv0=p.rv0[g])
        t.xc, xabs_c = task_cm(case, x64, g), task_cm(case, xabs, g)
        t.dyc = np.ascontiguousarray(packed_block(case, dxf, g).astype(np.float64).T)
        t.st = bc.stats_ref(t.xc, case.n_run(g))
        t.run = bc.running_ref(t.st, t.rm0, t.rv0)
        if mi is not None:
            t.mi = np.asarray(mi, np.float32).reshape(G, 2 * F)[g]
        elif case.kind == 'fp64':
            t.mi = np.concatenate([t.st.mean, t.st.invstd]).astype(np.float32)
        else:
            t.mi = np.concatenate([np.zeros(F), np.ones(F)]).astype(np.float32)
        p.mi[g] = t.mi
        t.ap = bc.apply_ref(t.xc, xabs_c, t.mi, t.gamma, t.beta, False)
        t.bw = bc.bwd_ref(t.xc, xabs_c, t.dyc, t.mi, t.gamma, t.beta, False, case.n_run(g), xb_rounds=case.xb)
        p.tasks.append(t)
    return p


# --------------------------------------------------------------------------------------------- checks (CPU emulation and GPU alike)
def _worst(per_task):
    """{key: the largest ratio over the tasks}; a non-finite ratio of any task stays non-finite"""
    out = {}
    for r in per_task:
        for key, v in r.items():
            v = v if np.isfinite(v) else np.inf
            out[key] = max(out.get(key, 0.0), v)
    return out


def stats_ratios(p, mi):
    """mi (G, 2F) fp32: every task's mean and invstd inside bn_cases' bounds for its own rows"""
    mi = np.asarray(mi).reshape(p.case.G, 2 * p.case.F)
    return _worst([bc.stats_ratios(t, mi[t.g]) for t in p.tasks])


def running_ratios(p, rms, rvs):
    """rms, rvs: per task the updated buffer (F), or None for a task without"""
    return _worst([bc.running_ratios(t, rms[t.g], rvs[t.g]) for t in p.tasks if rms[t.g] is not None])


def apply_ratios(p, y):
    """y packed (T B, F)"""
    return _worst([bc.apply_ratios(t, packed_block(p.case, y, t.g)) for t in p.tasks])


def bwd_ratios(p, dx, dgammas, dbetas):
    """dx interleaved (T, B, F); dgammas, dbetas: per task (F)"""
    return _worst([bc.bwd_ratios(t, task_rows(p.case, dx, t.g), dgammas[t.g], dbetas[t.g]) for t in p.tasks])


def exact_expectations(p):
    """what the 'count' cases fix bit for bit: per task mean, invstd (within 1 ulp), dgamma, dbeta; y packed"""
    case = p.case
    assert case.kind == 'count'
    out = SimpleNamespace(mean=[], invstd=[], dgamma=[], dbeta=[], y=np.empty((case.T * case.B, case.F), np.float32))
    for t in p.tasks:
        n = case.rows(t.g)
        s = t.xc.sum(1)
        out.mean.append((s / n).astype(np.float32))
        out.invstd.append((1 / np.sqrt((t.xc * t.xc).sum(1) / n - (s / n) ** 2 + EPS)).astype(np.float32))
        out.dbeta.append(t.dyc.sum(1).astype(np.float32))
        out.dgamma.append((t.dyc * t.xc).sum(1).astype(np.float32))            # xhat = x under mean_invstd = (0, 1)
        packed_block(case, out.y, t.g)[...] = (t.xc + (10.0 + t.g)).T           # gamma = 1, beta = 10 + g
    return out
