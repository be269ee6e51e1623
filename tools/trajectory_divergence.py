"""How far two runs of bench.py's training trajectory drift apart: the bench's first N steps (B = 10, the timed path's step
function, a host synchronisation per step), twice from the same seed and once from weights multiplied by (1 + 1e-7 * noise);
per step the relative loss / gradient-norm differences.  The backward pass reduces in float with atomics (split-K GEMMs,
conv weight gradients, CTC), so same-seed runs differ in the last bit from the first step; this prints how the trajectory
grows that.  profiles/trajectory_divergence.txt holds a run; bench.py --dump-outputs is built around it (dump_outputs).

    python tools/trajectory_divergence.py [N=25]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'aes-lac-2018_amd')]
os.environ.setdefault('DS2_GRU_STRICT', '1')

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codes.engine import Trainer  # noqa: E402
from codes.model import DeepSpeech  # noqa: E402
from codes.transforms import BatchSpectrogram  # noqa: E402


def trajectory(resident, dev, nsteps, perturb=0.0):
    torch.manual_seed(42)                                    # bench.py's model seed
    model = DeepSpeech().to(dev)
    if perturb:
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1 + perturb * torch.randn(p.shape, generator=g).to(dev))
    opt = torch.optim.SGD(model.parameters(), lr=3e-4, momentum=0.9, nesterov=True)
    trainer = Trainer(model, opt, device=dev, max_norm=400)
    front = BatchSpectrogram(device=dev)
    out = []
    for i in range(nsteps):
        flat, offs, labels, lens = resident[i % len(resident)]
        inputs, pct = front(flat, offs)
        loss = trainer.update((inputs, labels, pct, lens), defer=False)
        out.append((loss, trainer.last_grad_norm))
    return np.array(out)


def main():
    nsteps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    dev = torch.device('cuda', 0)
    plan = bench.bin_plan(10, bench.NUM_BINS)
    resident = [bench.make_resident(bench.make_bin(p), dev) for p in plan]
    a = trajectory(resident, dev, nsteps)
    b = trajectory(resident, dev, nsteps)
    c = trajectory(resident, dev, nsteps, perturb=1e-7)
    rel = lambda x, y: abs(x - y) / abs(x)                       # noqa: E731
    print('step     loss_a     loss_b   loss rel(a,b)  rel(a,perturbed)   gnorm rel(a,b)  rel(a,perturbed)')
    for i in range(nsteps):
        print('%4d %10.4f %10.4f %15.2e %17.2e %16.2e %17.2e' % (i, a[i, 0], b[i, 0], rel(a[i, 0], b[i, 0]), rel(a[i, 0], c[i, 0]),
                                                              rel(a[i, 1], b[i, 1]), rel(a[i, 1], c[i, 1])))


if __name__ == '__main__':
    main()
