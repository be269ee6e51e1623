#!/usr/bin/env python
"""One rank of the 2-rank data-parallel MULTI-TASK step test (started by tests/test_multitask_ddp_gpu.py as a fresh process).

    python tests/ddp_mt_worker.py RANK WORLD PORT OUT.npz

As tests/ddp_worker.py, on a two-head MultiTaskModel: both ranks share cuda:0, ``gloo`` on device tensors, rank r != 0 starts
from other weights (the trainer's construction-time broadcast must overwrite them).  The minibatches come from
``DistributedBucketingSampler`` over a ``ConcatAudioDataset`` of two in-memory corpora through the multi-task collate, so
most bins hold one task only (the other head absent on that rank) and one bin holds both.  ``emulate`` restates the
averaged step in one process: every rank's gradient from the model's own fused pass, the mean over ranks, the global-norm
clip and torch's Nesterov SGD.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'aes-lac-2018_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

MT_KW = dict(rnn_hidden_size=32, num_rnn_layers=2)
PER_TASK, BATCH = 10, 4            # 20 utterances -> 5 bins: en, en, en + pt_BR, pt_BR, pt_BR; 3 per rank at world 2
WEIGHTS = [1.0, 0.5]
LR, MOMENTUM, MAX_NORM = 2e-2, 0.9, 2.0


class _Corpus(torch.utils.data.Dataset):
    def __init__(self, offset, nalpha):
        from tests import ddp_common as dc
        self.items = []
        for i in range(PER_TASK):
            x, lab = dc.utterance(i + offset)
            self.items.append((torch.from_numpy(x), [int(v) % (nalpha - 1) + 1 for v in lab]))
        self.durations = [float(x.shape[0]) for x, _ in self.items]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def dataset():
    from codes.data import ConcatAudioDataset
    return ConcatAudioDataset([_Corpus(0, 29), _Corpus(3, 43)])


def rank_batches(rank, world):
    from codes.data import AudioDataLoader
    from codes.sampler import DistributedBucketingSampler
    ds = dataset()
    sampler = DistributedBucketingSampler(ds, batch_size=BATCH, num_replicas=world, rank=rank)
    return list(AudioDataLoader(ds, batch_sampler=sampler, num_tasks=2))


def build(seed):
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    from oracle.model import seeded_state_dict
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': dict(MT_KW)}))
    model.load_state_dict(seeded_state_dict(model, seed))
    return model.to('cuda')


def emulate(world):
    """Per-rank losses and the final parameters of every replica under the averaged step, in one process."""
    from codes.ctc import ctc_costs_and_grad
    from codes.engine import _join_tasks, sanitize_inputs
    reps = [build(7) for _ in range(world)]
    opts = [torch.optim.SGD(m.parameters(), lr=LR, momentum=MOMENTUM, nesterov=True) for m in reps]
    batches = [rank_batches(r, world) for r in range(world)]
    losses = [[] for _ in range(world)]
    for step in range(len(batches[0])):
        for r, m in enumerate(reps):
            inputs, targets, pct, sizes = batches[r][step]
            x, present = _join_tasks(inputs)
            m.train()

            def loss_fn(acts, present=present, targets=targets, pct=pct, sizes=sizes):
                costs, grads = [], []
                for (i, n), a in zip(present, acts):
                    c, d = ctc_costs_and_grad(a, targets[i], sanitize_inputs(a.shape[0], pct[i]), sizes[i],
                                              grad_scale=WEIGHTS[i] / n)
                    costs.append(float(c.sum().item()) * WEIGHTS[i] / n)
                    grads.append(d)
                return sum(costs), grads

            loss, _ = m.forward_backward(x.cuda(), present, loss_fn)
            losses[r].append(loss)
        with torch.no_grad():
            mean = sum(m.flat_grad() for m in reps) / world
            for m in reps:
                m.flat_grad().copy_(mean)
        for m, o in zip(reps, opts):
            torch.nn.utils.clip_grad_norm_(m.parameters(), MAX_NORM)
            o.step()
    torch.cuda.synchronize()
    return losses, [[p.detach().cpu().numpy().copy() for p in m.parameters()] for m in reps]


def main():
    import faulthandler
    import torch.distributed as dist
    faulthandler.dump_traceback_later(int(os.environ.get('DS2_TEST_HANG_S', '200')), exit=True)   # a hung rank says where
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from codes.ctc import CTCLoss
        from codes.engine import create_trainer
        model = build(7 if rank == 0 else 70 + rank)
        opt = torch.optim.SGD(model.parameters(), lr=LR, momentum=MOMENTUM, nesterov=True)
        trainer = create_trainer(model, opt, [CTCLoss(), CTCLoss()], 'cuda', max_norm=MAX_NORM, task_weights=WEIGHTS)
        assert trainer.distributed and trainer.world == world and trainer._fused
        losses, present = [], []
        for batch in rank_batches(rank, world):
            present.append([int(x is not None) for x in batch[0]])
            losses.append(trainer.update(batch))
        torch.cuda.synchronize()
        res = {'losses': np.asarray(losses), 'present': np.asarray(present), 'overlap': np.int32(trainer.overlap)}
        for i, p in enumerate(model.parameters()):
            res['p%03d' % i] = p.detach().cpu().numpy()
        np.savez(out, **res)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
