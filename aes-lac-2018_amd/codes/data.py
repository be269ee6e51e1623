"""Minibatch assembly (reference ``codes/data.py:106-166``, ``AudioDataLoader._collate_fn``).

The output layout is the hot path's input contract: ``inputs (B,T_max,161)`` float32 zero padded,
``targets`` flat int32, ``input_percentages (B)`` float32 = T_i / float(T_max), ``target_sizes (B)`` int32.
Multi-task (``ConcatAudioDataset`` items carry a task index, ``collate_multitask``): the same four fields as per-task
lists in task order, ``None`` for a task with no utterance in the batch, every task padded to the BATCH-wide T_max
(reference ``codes/data.py:106-165``).  The per-task inputs are views of ONE (B,T_max,161) tensor in task order, so the
model's concatenation of the present tasks costs no copy.  The raw-audio path (``collate_audio_multitask``) hands on ONE
``RawAudioBatch`` of all clips in task order with the per-task counts (``TaskCounts``, in the input-percentage slot): the device
frontend runs once on it, and ``split_tasks`` cuts the (B,T_max,161) result into the per-task views.
"""
import bisect

import torch


def collate(batch):
    """batch: list of (spect (T_i,F) tensor, labels list[int]) -> the reference's 4-tuple (CPU tensors)."""
    longest = max(batch, key=lambda s: s[0].shape[0])[0]
    t_max, nfreq = longest.shape
    n = len(batch)
    inputs = torch.zeros(n, t_max, nfreq)
    pct = torch.zeros(n, dtype=torch.float)
    sizes = torch.zeros(n, dtype=torch.int)
    flat = []
    for i, (spect, target) in enumerate(batch):
        t_i = spect.shape[0]
        inputs[i, :t_i, :].copy_(spect)
        pct[i] = t_i / float(t_max)
        sizes[i] = len(target)
        flat.extend(target)
    return inputs, torch.tensor(flat, dtype=torch.int), pct, sizes


def collate_multitask(batch, num_tasks):
    """batch: list of (spect (T_i,F), labels list[int], task) -> (inputs, targets, input_percentages, target_sizes), each a
    list of ``num_tasks`` entries (``None`` for an absent task), utterances grouped by task in batch order."""
    t_max, nfreq = max(batch, key=lambda s: s[0].shape[0])[0].shape
    order = [[k for k, b in enumerate(batch) if b[2] == task] for task in range(num_tasks)]
    inputs = torch.zeros(len(batch), t_max, nfreq)
    out = ([None] * num_tasks, [None] * num_tasks, [None] * num_tasks, [None] * num_tasks)
    row = 0
    for task, idxs in enumerate(order):
        if not idxs:
            continue
        n = len(idxs)
        pct = torch.zeros(n, dtype=torch.float)
        sizes = torch.zeros(n, dtype=torch.int)
        flat = []
        for j, k in enumerate(idxs):
            spect, target = batch[k][0], batch[k][1]
            t_i = spect.shape[0]
            inputs[row + j, :t_i, :].copy_(spect)
            pct[j] = t_i / float(t_max)
            sizes[j] = len(target)
            flat.extend(target)
        out[0][task] = inputs[row:row + n]
        out[1][task] = torch.tensor(flat, dtype=torch.int)
        out[2][task] = pct
        out[3][task] = sizes
        row += n
    return out


class TaskCounts(tuple):
    """Per-task utterance counts of a multi-task raw-audio batch, whose clips are in task order (0: the task is absent)."""


def split_tasks(inputs, pct, counts):
    """(B,T_max,161) frontend output + input percentages of a batch in task order -> per-task lists (``None`` if absent):
    views of the batch-wide tensor, percentages relative to the batch-wide T_max (codes/data.py:132-152)."""
    xs, ps, b0 = [], [], 0
    ready, src = getattr(inputs, '_ds2_ready', None), getattr(inputs, '_ds2_src', None)
    for n in counts:
        if n == 0:
            xs.append(None)
            ps.append(None)
            continue
        v = inputs[b0:b0 + n]
        if ready is not None:                        # (a prefetcher's output: every view carries its ready event)
            v._ds2_ready, v._ds2_src = ready, src
        xs.append(v)
        ps.append(pct[b0:b0 + n])
        b0 += n
    return xs, ps


def collate_audio_multitask(batch, num_tasks):
    """batch: list of (wav or PCMClip, labels, task) -> (wavs in task order, per-task targets, TaskCounts, per-task
    target sizes); ``None`` targets / sizes for an absent task."""
    order = [[b for b in batch if b[2] == task] for task in range(num_tasks)]
    wavs, targets, sizes = collate_audio([(b[0], b[1]) for items in order for b in items])
    targets_l, sizes_l, off, row = [], [], 0, 0
    for items in order:
        if not items:
            targets_l.append(None)
            sizes_l.append(None)
            continue
        sz = sizes[row:row + len(items)]
        n = int(sz.sum())
        targets_l.append(targets[off:off + n])
        sizes_l.append(sz)
        off += n
        row += len(items)
    return wavs, targets_l, TaskCounts(len(items) for items in order), sizes_l


def collate_audio(batch):
    """batch: list of (wav, labels) -> (wavs, targets, target_sizes) for the GPU frontend.  ``wav`` is a 1-D float tensor
    (then ``wavs`` is the list of them) or a ``PCMClip`` of int16 samples (then ``wavs`` is ONE ``RawAudioBatch``)."""
    from .transforms import PCMClip, RawAudioBatch
    wavs = [b[0] for b in batch]
    if wavs and isinstance(wavs[0], PCMClip):
        wavs = RawAudioBatch.from_clips(wavs)
    flat = [int(v) for b in batch for v in b[1]]
    sizes = torch.tensor([len(b[1]) for b in batch], dtype=torch.int)
    return wavs, torch.tensor(flat, dtype=torch.int), sizes


class AudioDataset(torch.utils.data.Dataset):
    """Manifest CSV ``audio_path,transcript_path,duration`` (reference ``codes/data.py:13-70``; no zip support)."""

    def __init__(self, data_dir, manifest_filepath, transforms=None, target_transforms=None):
        import os
        self.data_dir, self.manifest_filepath = data_dir, manifest_filepath
        with open(manifest_filepath) as f:
            rows = [line.strip().split(',') for line in f if line.strip()]
        self.durations = [float(r[2]) for r in rows]
        self.data = [(os.path.join(data_dir, r[0]), os.path.join(data_dir, r[1])) for r in rows]
        self.transforms, self.target_transforms = transforms, target_transforms

    def __getitem__(self, index):
        audio, target = self.data[index]
        if self.transforms is not None:
            audio = self.transforms(audio)
        if self.target_transforms is not None:
            target = self.target_transforms(target)
        return audio, target

    def __len__(self):
        return len(self.data)


class ConcatAudioDataset(torch.utils.data.ConcatDataset):
    """Several ``AudioDataset`` (one per task) end to end; items are ``(audio, target, task_index)`` (reference
    ``codes/data.py:72-93``).  ``durations`` is every dataset's list in order, ``cumulative_sizes`` as ConcatDataset."""

    def __init__(self, datasets):
        super().__init__(datasets)
        self._durations = [d for ds in self.datasets for d in ds.durations]

    def __getitem__(self, idx):
        task = bisect.bisect_right(self.cumulative_sizes, idx)
        return tuple(super().__getitem__(idx)) + (task,)

    @property
    def durations(self):
        return self._durations


class AudioDataLoader(torch.utils.data.DataLoader):
    """DataLoader whose collate is the reference's (``codes/data.py:96-166``).

    ``raw_audio=True`` keeps clips as raw 1-D waveforms (``collate_audio``) so the spectrogram runs on the GPU
    after collate (``BatchSpectrogram``) instead of per utterance in worker processes."""

    def __init__(self, *args, **kwargs):
        raw = kwargs.pop('raw_audio', False)
        num_tasks = int(kwargs.pop('num_tasks', 1) or 1)
        if num_tasks > 1:
            import functools
            kwargs['collate_fn'] = functools.partial(_collate_raw_multitask if raw else _collate_spect_multitask,
                                                     num_tasks=num_tasks)
        else:
            kwargs['collate_fn'] = _collate_raw if raw else _collate_spect
        super().__init__(*args, **kwargs)


def _labels_list(t):
    import numpy as np
    return [int(v) for v in np.asarray(t).reshape(-1)]


def _collate_spect(batch):
    return collate([(s, _labels_list(t)) for s, t in batch])


def _collate_spect_multitask(batch, num_tasks):
    return collate_multitask([(s, _labels_list(t), int(task)) for s, t, task in batch], num_tasks)


def _collate_raw_multitask(batch, num_tasks):
    return collate_audio_multitask([(w, _labels_list(t), int(task)) for w, t, task in batch], num_tasks)


def _collate_raw(batch):
    wavs, targets, sizes = collate_audio([(w, _labels_list(t)) for w, t in batch])
    return wavs, targets, None, sizes


class DevicePrefetcher(object):
    """Iterate a loader of ``(RawAudioBatch, targets, None, sizes)`` one minibatch AHEAD, on a side stream: while the
    GPU trains on step i, the int16 samples of step i+1 cross PCIe (from page-locked memory when the loader pins) and --
    when a ``frontend`` (``BatchSpectrogram``) is attached -- are decoded, tempo-changed, gain-scaled and turned into
    the log-spectrogram there too, so the training stream never waits for an upload or for the (sequential per clip)
    WSOLA search.  What is yielded carries a ``ready`` event (``RawAudioBatch.ready`` / ``inputs._ds2_ready``) that the
    consumer's stream waits on.  Batches that are not ``RawAudioBatch`` pass through unchanged."""

    def __init__(self, loader, device='cuda', frontend=None):
        self.loader, self.device, self.frontend = loader, torch.device(device), frontend
        self.stream = torch.cuda.Stream(device=self.device)

    def __len__(self):
        return len(self.loader)

    @property
    def batch_sampler(self):
        return self.loader.batch_sampler

    def _stage(self, batch):
        from .transforms import RawAudioBatch
        wavs = batch[0]
        if not isinstance(wavs, RawAudioBatch):
            return batch
        with torch.cuda.stream(self.stream):
            dev = wavs.to(self.device, non_blocking=True)
            dev._host = wavs                         # keep the page-locked source alive until the copy has run
            if self.frontend is not None:
                inputs, pct = self.frontend(dev)
                inputs._ds2_ready = torch.cuda.Event()
                inputs._ds2_ready.record(self.stream)
                inputs._ds2_src = dev
                if isinstance(batch[2], TaskCounts):                  # multi-task: per-task views of the one batch
                    inputs, pct = split_tasks(inputs, pct, batch[2])
                return (inputs, batch[1], pct, batch[3])
            dev.ready = torch.cuda.Event()
            dev.ready.record(self.stream)
        return (dev,) + tuple(batch[1:])

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        for batch in it:
            cur, nxt = nxt, self._stage(batch)
            yield cur
        yield nxt


def wait_ready(inputs):
    """Make the current stream wait for a tensor a ``DevicePrefetcher`` produced on its side stream (no-op otherwise)."""
    ev = getattr(inputs, '_ds2_ready', None)
    if ev is not None:
        torch.cuda.current_stream().wait_event(ev)
        inputs.record_stream(torch.cuda.current_stream())
        inputs._ds2_ready = None
    return inputs
