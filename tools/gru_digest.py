"""sha256 digests of what the persistent recurrence kernels compute on seeded inputs: one forward and one backward launch per
case, one line per case, one process for the whole list.  Two builds of the same arithmetic print the same lines:

    python tools/gru_digest.py > a.txt;  DS2_LIB_VARIANT=<other build> DS2_SKIP_BUILD_CHECK=1 python tools/gru_digest.py > b.txt

    python tools/gru_digest.py [--family 16|4] [--tuning]

--family 16 (the default): the 16x16 kernels of csrc/gru_persist16.hip (counted hand-off, fixed reduction order: deterministic).
--family 4: the 4x4x1 kernels of csrc/gru_persist.hip.  The backward pass runs twice per case, through the d(gh) hand-off
  (DS2_GRU_BWD_DH=0) and, where ds2_gru_bwd_dh_supported, through the d(h) hand-off on a forward pass that writes `coef`, which
  is digested too.  The speculative forms re-load a stale fragment and never change the order of a sum, so they are expected
  to print the same lines run after run as well.
--tuning: the cases only the tuning library reaches (DS2_LIB_VARIANT=tuning).  Family 16: the whole-batch forms with 2 and 4
  batch tiles; family 4: gru_bwd_persistent4_kernel<K, 4, 2> and <K, 2, 0> and the k-balanced 20-unit forward form."""
import hashlib, os, sys
_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(_ROOT, 'aes-lac-2018_amd')); sys.path.insert(0, _ROOT)
import torch
from ds2hip import lib
if os.environ.get('DS2_LIB_VARIANT'):
    lib.LIB_PATH = os.path.join(os.path.dirname(lib.LIB_PATH), 'libds2hip_%s.so' % os.environ['DS2_LIB_VARIANT'])
from ds2hip import ops

WHOLE = {'DS2_GRU_FWD': '16', 'DS2_GRU_BWD': '16'}
FP32 = {'DS2_GRU_P2_BF16': '0', 'DS2_GRU_P2_BF16_BWD': '0'}
BF16 = {'DS2_GRU_P2_BF16': '1', 'DS2_GRU_P2_BF16_BWD': '1'}
FOUR = {'DS2_GRU_FWD': '4', 'DS2_GRU_BWD': '4'}
KNOBS = ('DS2_GRU_FWD', 'DS2_GRU_BWD', 'DS2_GRU_P2_BF16', 'DS2_GRU_P2_BF16_BWD', 'DS2_GRU_FWD_P2', 'DS2_GRU_BWD_P2',
         'DS2_GRU_FWD_WIDE', 'DS2_GRU_PROTO', 'DS2_GRU_FWD_ROWS')


def cases16(tuning):
    """(T, B, H, env, spare_cus)"""
    if tuning:                                        # whole-batch forms, 2 (B = 32) and 4 (B = 64) batch tiles
        off = dict(WHOLE, DS2_GRU_FWD_P2='0', DS2_GRU_BWD_P2='0')
        return [(5, b, h, off, -1) for h in (64, 800) for b in (32, 64)]
    out = [(5, b, h, env, -1) for h in (32, 64, 128, 256, 384)
           for b, env in ((5, WHOLE), (17, FP32), (17, BF16), (33, FP32), (33, BF16))]
    out += [(5, 10, 800, WHOLE, -1), (5, 13, 800, {}, -1), (5, 16, 800, {}, -1)]
    out += [(5, b, 800, env, -1) for b in (17, 32, 64) for env in (FP32, BF16)]
    return out


def cases4(tuning):
    """Widths 64, 256, 384, 800: backward k groups per wave (NGI) 1, 2, 3, 5, forward 1, 1, 1, 2.  B = 3, 4: one part; 5, 7, 8:
    two parts; 9, 10, 12: three parts of one batch quad, 20 / 24 / 28 units by spare_cus 0 / 52 / 82 (backward) and 20 or,
    with DS2_GRU_FWD_WIDE=0, 24 (forward); 16, 24 (and 27 at H = 256): the counted protocol."""
    if tuning:
        out = [(5, 16, h, {'DS2_GRU_FWD': '16', 'DS2_GRU_BWD': '4', 'DS2_GRU_PROTO': '2'}, -1) for h in (64, 800)]
        out += [(5, 4, h, {'DS2_GRU_FWD': '16', 'DS2_GRU_BWD': '4', 'DS2_GRU_PROTO': '0'}, -1) for h in (64, 800)]
        return out + [(5, 10, 800, dict(FOUR, DS2_GRU_FWD_ROWS='0'), -1)]
    out = []
    for h in (64, 256, 384, 800):
        for b in (3, 4, 5, 7, 8, 9, 10, 12, 16, 24):
            out += [(5, b, h, FOUR, spare) for spare in ((0, 52, 82) if 9 <= b <= 12 else (-1,))]
        out.append((5, 10, h, dict(FOUR, DS2_GRU_FWD_WIDE='0'), -1))
    return out + [(5, 27, 256, FOUR, -1), (5, 32, 800, FOUR, -1)]


def digest(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def run(gi, w_hh, w_hh_t, d_out, t, bsz, hid, spare, dh):
    """One forward and one backward launch -> (rzn, ghn, hout, coef or None, dgi, dghn)"""
    os.environ['DS2_GRU_BWD_DH'] = '1' if dh else '0'
    g = gi.clone()
    ghn, hout, coef = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid, want_coef=True)
    assert (coef is not None) == dh
    rzn, ghn_f = g.clone(), ghn.clone()
    ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=spare, coef=coef)
    torch.cuda.synchronize()
    ops.check_async_errors()
    assert not ops._persistent_off
    return rzn, ghn_f, hout, coef, g, ghn


family = sys.argv[sys.argv.index('--family') + 1] if '--family' in sys.argv else '16'
ops.GRU_MODE = 'persistent'
for t, bsz, hid, env, spare in {'16': cases16, '4': cases4}[family]('--tuning' in sys.argv):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    torch.manual_seed(1000 * hid + bsz)
    w_hh = ((torch.rand(2, 3 * hid, hid) * 2 - 1) / hid ** 0.5).cuda()
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    gi = torch.randn(t, bsz, 2, 3 * hid).cuda()
    d_out = torch.randn(t, bsz, hid).cuda()
    rzn, ghn_f, hout, _, dgi, dghn = run(gi, w_hh, w_hh_t, d_out, t, bsz, hid, spare, False)
    name = ' '.join('%s=%s' % kv for kv in sorted(env.items())) or '-'
    if family == '4':
        name += ' spare_cus=%d' % spare
    line = 'T=%d B=%d H=%d %s | in %s %s %s | rzn %s ghn %s hout %s dgi %s dghn %s' % (
        t, bsz, hid, name, digest(w_hh), digest(gi), digest(d_out), digest(rzn), digest(ghn_f), digest(hout), digest(dgi),
        digest(dghn))
    if family == '4' and lib.query('ds2_gru_bwd_dh_supported', bsz, hid):
        rzn, ghn_f, hout, coef, dgi, dghn = run(gi, w_hh, w_hh_t, d_out, t, bsz, hid, spare, True)
        line += ' | dh: rzn %s ghn %s hout %s coef %s dgi %s dghn %s' % (
            digest(rzn), digest(ghn_f), digest(hout), digest(coef), digest(dgi), digest(dghn))
    print(line, flush=True)
