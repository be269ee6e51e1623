"""Length-bucketed batch samplers (reference ``codes/sampler.py:9-30,100-135``).

Manifests are sorted by duration, so consecutive ids have similar lengths; a bin is ``batch_size``
consecutive ids.  ``DistributedBucketingSampler`` is the data-parallel partition of the hot path:
rank r consumes bins r, r+W, r+2W, ... of the (wrapped) bin list, so the global batch is W x batch_size.
``WeightedBucketingRandomSampler`` draws the multi-task epochs (``sampling``: equal / unbalanced / schedule) over a
``ConcatAudioDataset``, with the reference's seeding, so its bins equal the reference's.
"""
import math

import numpy as np
import torch
from torch.utils.data.sampler import Sampler


class BucketingSampler(Sampler):
    def __init__(self, data_source, batch_size=1):
        self.data_source = data_source
        ids = list(range(len(data_source)))
        self.bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch):
        np.random.seed(epoch)
        np.random.shuffle(self.bins)


class WeightedBucketingRandomSampler(Sampler):
    """Multi-task sampler (reference ``codes/sampler.py:33-97``): every epoch draws ``len(dataset)`` utterance ids with
    ``torch.multinomial`` under ``torch.manual_seed(epoch)``, sorts them by duration and cuts them into bins.
      equal:      weight total/count_task per utterance, with replacement (every task is drawn equally often);
      unbalanced: uniform, without replacement (one pass over the concatenated data);
      schedule:   two tasks, task 0 drawn with probability (E - epoch)/E, task 1 with the rest (``num_epochs`` = E)."""

    def __init__(self, data_source, batch_size=1, sampling='equal', num_epochs=None):
        self.data_source = data_source
        self.durations = data_source.durations
        self.batch_size = batch_size
        self.sampling = sampling
        self.num_epochs = num_epochs
        cum = list(data_source.cumulative_sizes)
        self.tasks_count = [hi - lo for lo, hi in zip([0] + cum[:-1], cum)]
        self.bins = self.draw_bins()

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def _weights(self, epoch):
        counts = self.tasks_count
        if self.sampling == 'equal':
            total = sum(counts)
            return [total / c for c in counts for _ in range(c)], True
        if self.sampling == 'unbalanced':
            return [1.0] * len(self.data_source), False
        if self.sampling == 'schedule':
            if len(counts) != 2:
                raise ValueError('sampling "schedule" needs exactly 2 datasets')
            if self.num_epochs is None:
                raise ValueError('sampling "schedule" needs num_epochs')
            prob = (self.num_epochs - epoch) / self.num_epochs
            probs = [prob, 1 - prob]
            return [1 / c * probs[k] for k, c in enumerate(counts) for _ in range(c)], True
        raise ValueError('sampling option not recognized: %r' % (self.sampling,))

    def draw_bins(self, epoch=0):
        weights, replacement = self._weights(epoch)
        torch.manual_seed(epoch)
        ids = torch.multinomial(torch.tensor(weights, dtype=torch.double), len(self.data_source), replacement)
        order = np.argsort([self.durations[i] for i in ids.tolist()])
        ids = ids[torch.from_numpy(np.asarray(order))].tolist()
        return [ids[i:i + self.batch_size] for i in range(0, len(ids), self.batch_size)]

    def shuffle(self, epoch):
        self.bins = self.draw_bins(epoch)


class DistributedBucketingSampler(Sampler):
    def __init__(self, data_source, batch_size=1, num_replicas=None, rank=None):
        if num_replicas is None:
            num_replicas = torch.distributed.get_world_size()
        if rank is None:
            rank = torch.distributed.get_rank()
        self.data_source = data_source
        ids = list(range(len(data_source)))
        self.batch_size = batch_size
        self.bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]
        self.num_replicas, self.rank = num_replicas, rank
        self.num_samples = int(math.ceil(len(self.bins) / float(num_replicas)))
        self.total_size = self.num_samples * num_replicas

    def __iter__(self):
        bins = self.bins + self.bins[:self.total_size - len(self.bins)]     # wrap so every rank gets as many
        return iter(bins[self.rank::self.num_replicas])

    def __len__(self):
        return self.num_samples

    def shuffle(self, epoch):
        g = torch.Generator()
        g.manual_seed(epoch)
        order = torch.randperm(len(self.bins), generator=g).tolist()
        self.bins = [self.bins[i] for i in order]
