"""sha256 digests of what the 16x16 persistent recurrence kernels (csrc/gru_persist16.hip) compute on seeded inputs: one forward
and one backward launch per case, one line per case.  The kernels are deterministic (counted hand-off, fixed reduction order),
so two builds of the same arithmetic print the same lines:

    python tools/gru16_digest.py > a.txt;  DS2_LIB_VARIANT=<other build> DS2_SKIP_BUILD_CHECK=1 python tools/gru16_digest.py > b.txt

    python tools/gru16_digest.py [--tuning]

--tuning: the cases only the tuning library reaches (DS2_LIB_VARIANT=tuning: the whole-batch forms with 2 and 4 batch tiles)."""
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
KNOBS = ('DS2_GRU_FWD', 'DS2_GRU_BWD', 'DS2_GRU_P2_BF16', 'DS2_GRU_P2_BF16_BWD', 'DS2_GRU_FWD_P2', 'DS2_GRU_BWD_P2')


def cases(tuning):
    if tuning:                                        # whole-batch forms, 2 (B = 32) and 4 (B = 64) batch tiles
        off = dict(WHOLE, DS2_GRU_FWD_P2='0', DS2_GRU_BWD_P2='0')
        return [(5, b, h, off) for h in (64, 800) for b in (32, 64)]
    out = [(5, b, h, env) for h in (32, 64, 128, 256, 384)
           for b, env in ((5, WHOLE), (17, FP32), (17, BF16), (33, FP32), (33, BF16))]
    out += [(5, 10, 800, WHOLE), (5, 13, 800, {}), (5, 16, 800, {})]
    out += [(5, b, 800, env) for b in (17, 32, 64) for env in (FP32, BF16)]
    return out


def digest(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


ops.GRU_MODE = 'persistent'
for t, bsz, hid, env in cases('--tuning' in sys.argv):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    os.environ['DS2_GRU_BWD_DH'] = '0'
    torch.manual_seed(1000 * hid + bsz)
    w_hh = ((torch.rand(2, 3 * hid, hid) * 2 - 1) / hid ** 0.5).cuda()
    w_hh_t = torch.stack([ops.transpose2d(w_hh[0], 3 * hid, hid), ops.transpose2d(w_hh[1], 3 * hid, hid)], 0)
    gi = torch.randn(t, bsz, 2, 3 * hid).cuda()
    d_out = torch.randn(t, bsz, hid).cuda()
    g = gi.clone()
    ghn, hout = ops.gru_bidir_fwd(g, w_hh, t, bsz, hid)
    rzn, ghn_f = g.clone(), ghn.clone()
    ops.gru_bidir_bwd(g, ghn, hout, d_out, w_hh_t, t, bsz, hid)
    torch.cuda.synchronize()
    ops.check_async_errors()
    assert not ops._persistent_off
    print('T=%d B=%d H=%d %s | in %s %s %s | rzn %s ghn %s hout %s dgi %s dghn %s' % (
        t, bsz, hid, ' '.join('%s=%s' % kv for kv in sorted(env.items())) or '-', digest(w_hh), digest(gi), digest(d_out),
        digest(rzn), digest(ghn_f), digest(hout), digest(g), digest(ghn)), flush=True)
