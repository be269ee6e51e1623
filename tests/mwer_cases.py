"""Seeded inputs shared by tests/test_mwer_cpu.py and tests/test_mwer_gpu.py.  No GPU in here; nothing depends on a kernel's
output.  A case: acts (T,B,A) float32, act_lens, hyps[b] (lists of int32 label arrays), risks[b], refs[b], regime.
"""
import zlib

import numpy as np

from tests import ctc_cases as cc


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(('mwer',) + key).encode()))


def perturb(rng, ref, nalpha):
    """A hypothesis near ``ref``: each label substituted or deleted with probability 0.15, an insertion now and then."""
    out = []
    for v in ref:
        u = rng.random()
        if u < 0.08:
            continue
        out.append(int(rng.integers(1, nalpha)) if u < 0.16 else int(v))
        if rng.random() < 0.05:
            out.append(int(rng.integers(1, nalpha)))
    return np.asarray(out, dtype=np.int32)


def make_case(name, regime, t_max, nalpha, ref_lens, act_lens, nbest, counts=None, hyp_lens=None):
    """References of ``ref_lens`` labels; ``nbest`` hypotheses per utterance near the reference (or, with ``hyp_lens[b][n]``,
    random rows of exactly those lengths); integer risks 0..5 drawn at random, no two rows of an utterance equal where there
    is room.  acts in ``regime`` of tests/ctc_cases.py, `peaked` around the reference's alignment."""
    rng = _rng(name, regime, t_max, nalpha, tuple(ref_lens), tuple(act_lens), nbest)
    bsz = len(ref_lens)
    refs = [cc.make_labels(rng, nalpha, int(n)) for n in ref_lens]
    acts = cc.make_acts(rng, regime, t_max, nalpha, refs, act_lens)
    hyps, risks = [], []
    for b in range(bsz):
        k = nbest if counts is None else int(counts[b])
        if hyp_lens is not None:
            rows = [cc.make_labels(rng, nalpha, int(hyp_lens[b][n])) for n in range(k)]
        else:
            rows = [perturb(rng, refs[b], nalpha) for _ in range(k)]
        hyps.append(rows)
        risks.append(rng.permutation(max(k, 6))[:k].astype(np.float64))
    return {'name': name, 'regime': regime, 'acts': acts, 'act_lens': np.asarray(act_lens, np.int32), 'hyps': hyps,
            'risks': risks, 'refs': refs, 'nbest': nbest}


def descent_case():
    """The descent test's input: T = 40, B = 3, A = 29, N = 4, every utterance with four distinct risks."""
    return make_case('descent', 'random', 40, 29, [6, 9, 4], [40, 33, 25], 4)


DESCENT_LR = 0.05
