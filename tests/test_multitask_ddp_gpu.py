"""The multi-task data-parallel step at world size 2: two fresh processes on cuda:0 (tests/ddp_mt_worker.py) against a
single-process emulation of the averaged step.

Checked: DistributedBucketingSampler over a ConcatAudioDataset with the multi-task collate (ranks see bins with one task
absent and a bin with both), the heads-first bucket of the overlapped all-reduce, the zero gradient of an absent head
(a head absent on one rank and present on the other gets half the other rank's gradient), the construction-time broadcast,
and replicas that end bit-identical.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('overlap', ['1', '0'])
def test_two_rank_multitask_step_matches_the_averaged_emulation(tmp_path, overlap):
    from tests import ddp_mt_worker as w
    world = 2
    port = 29500 + (os.getpid() % 150) + (3 if overlap == '1' else 0)
    env = dict(os.environ, DS2_GRU_MODE='step', DS2_ALLREDUCE_OVERLAP=overlap)
    outs = [str(tmp_path / ('rank%d.npz' % r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'ddp_mt_worker.py'), str(r), str(world), str(port),
                               outs[r]], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            _, se = p.communicate(timeout=300)     # (a hung rank dumps its stack and exits by itself after 200 s)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(se[-3000:])
    assert all(p.returncode == 0 for p in procs), '\n'.join(logs)
    got = [np.load(o) for o in outs]
    assert int(got[0]['overlap']) == int(overlap)
    # the bins: rank 0 en / en + pt_BR / pt_BR, rank 1 en / pt_BR / en (wrapped)
    assert got[0]['present'].tolist() == [[1, 0], [1, 1], [0, 1]]
    assert got[1]['present'].tolist() == [[1, 0], [0, 1], [1, 0]]
    want_losses, want_params = w.emulate(world)
    for r in range(world):
        np.testing.assert_allclose(got[r]['losses'], want_losses[r], rtol=2e-4, err_msg='rank %d losses' % r)
        for i, p in enumerate(want_params[r]):
            np.testing.assert_allclose(got[r]['p%03d' % i], p, atol=5e-5, err_msg='rank %d param %d' % (r, i))
    for i in range(len(want_params[0])):
        assert np.array_equal(got[0]['p%03d' % i], got[1]['p%03d' % i]), 'replicas differ at parameter %d' % i
