"""Log-spectrogram frontend on the GPU (reference ``codes/transforms.py:26-127``, ``ToSpectrogram``).

The reference runs ``librosa.stft`` per utterance on CPU DataLoader workers (``codes/data.py:61-62``,
``codes/transforms.py:94-119``).  Here the same arithmetic -- centre reflect-pad 160, 320-sample frames
every 160, symmetric Hann (``librosa_compat=True`` forces ``periodic=False``, ``:52-53``), |rFFT|, log1p,
per-utterance (S - mean) / (std_unbiased + eps) -- is one HIP kernel pair (csrc/spectrogram.hip) that
processes a whole padded minibatch after collate: ``BatchSpectrogram``.  ``ToSpectrogram`` keeps the
reference's constructor and per-utterance ``__call__`` for drop-in use.
"""
import torch

from ds2hip import ops

FRAME, HOP, NBINS = 320, 160, 161


class ToSpectrogram(object):
    def __init__(self, frame_length=320, hop=160, fft_size=None, pad_end=0, normalize=True,
                 window=torch.hann_window, window_params=None, librosa_compat=False, eps=1e-9, device='cuda'):
        fft_size = fft_size or frame_length
        hop = hop if hop is not None else frame_length // 2
        window_params = dict(window_params or {})
        if librosa_compat:
            window_params.setdefault('periodic', False)
        ok = (frame_length == FRAME and hop == HOP and fft_size == FRAME and pad_end == 0 and librosa_compat and
              window is torch.hann_window and window_params == {'periodic': False})
        if not ok:
            raise NotImplementedError('the HIP frontend implements the configuration the reference trains with: '
                                      'frame 320, hop 160, symmetric Hann, librosa_compat=True '
                                      '(codes/utils/training_utils.py:19-23)')
        self.frame_length, self.hop, self.fft_size = frame_length, hop, fft_size
        self.normalize, self.pad_end, self.eps = normalize, pad_end, eps
        self.window_params, self.librosa_compat = window_params, librosa_compat
        self.device = device

    def __call__(self, x):
        """x: 1-D float tensor of samples -> (T_in, 161) on x's device (a CPU input makes a GPU round trip)."""
        assert x.dim() == 1 and isinstance(x, torch.Tensor)
        src = x.device
        wav = x.to(self.device, torch.float32).contiguous()
        assert wav.numel() > FRAME // 2, 'reflect padding needs more than 160 samples'
        offs = torch.tensor([0, wav.numel()], dtype=torch.int64, device=wav.device)
        out = ops.spectrogram(wav, offs, 1 + wav.numel() // HOP, self.normalize, self.eps)[0]
        return out.to(src)

    def __repr__(self):
        return ('{}(frame_length={}, hop={}, fft_size={}, pad_end={}, normalize={},librosa_compat={})').format(
            self.__class__.__name__, self.frame_length, self.hop, self.fft_size, self.pad_end, self.normalize,
            self.librosa_compat)


class BatchSpectrogram(object):
    """Frontend + collate for a minibatch of raw clips, entirely on the device.

    ``__call__(wavs)`` with ``wavs`` a list of 1-D tensors (or (flat, offsets)) returns
    ``inputs (B,T_max,161)`` and ``input_percentages (B)`` float32 exactly as
    ``AudioDataLoader._collate_fn`` would have (``codes/data.py:132-152``): zero padding past each
    clip's frames, percentage = T_i / float(T_max) stored as float32.
    """

    def __init__(self, normalize=True, eps=1e-9, device='cuda', scale=None, noise=None, spec_augment=None, reverb=None,
                 speed=None):
        self.normalize, self.eps, self.device = normalize, eps, device
        self.scale = ops.amplitude_scale(scale)      # int16 clips (RawAudioBatch) come out as q * scale: see ToTensor
        self.noise = noise                           # a NoiseInjection: the bank the drawn noise of a batch is mixed from
        self.spec_augment = spec_augment             # a SpecAugment: resolves and applies the draws a batch carries
        self.reverb = reverb                         # a Reverb: the bank the drawn impulse responses of a batch come from
        self.speed = speed                           # a SpeedPerturb: the tables the drawn speed factors of a batch name

    def __call__(self, wavs, offsets=None):
        spec = None
        if isinstance(wavs, RawAudioBatch):                  # int16 clips (+ drawn augmentation): decode on the device
            if wavs.noise is not None and self.noise is None:
                raise RuntimeError('the batch carries noise draws (ToTensor(noise=...)) but this BatchSpectrogram was '
                                   'built without a noise bank: pass noise=<the NoiseInjection> to it')
            if wavs.reverb is not None and self.reverb is None:
                raise RuntimeError('the batch carries reverberation draws (ToTensor(reverb=...)) but this BatchSpectrogram '
                                   'was built without an RIR bank: pass reverb=<the Reverb> to it')
            if wavs.speed is not None and self.speed is None:
                raise RuntimeError('the batch carries speed draws (ToTensor(speed=...)) but this BatchSpectrogram was built '
                                   'without the tables: pass speed=<the SpeedPerturb> to it')
            spec = wavs.spec
            if spec is not None and self.spec_augment is None:
                raise RuntimeError('the batch carries SpecAugment draws (ToTensor(spec_augment=...)) but this '
                                   'BatchSpectrogram was built without one: pass spec_augment=<the SpecAugment> to it')
            if wavs.ready is not None:               # uploaded ahead of time on the prefetcher's copy stream
                torch.cuda.current_stream().wait_event(wavs.ready)
                wavs.pcm.record_stream(torch.cuda.current_stream())
            pcm = wavs.pcm if wavs.pcm.is_cuda else wavs.pcm.to(self.device, non_blocking=True)
            offsets = wavs.offsets
            if wavs.speed is not None:               # speed factors drawn by the loader: the int16 clips are resampled first
                pcm, offsets = self.speed.apply_batch(pcm, offsets, wavs.speed)
            flat, offs = ops.decode_augment(pcm, offsets, wavs.tempos, wavs.gains_db, scale=self.scale)
            if wavs.reverb is not None:              # RIRs drawn by the loader: convolved between gain and noise
                flat = self.reverb.apply_batch(flat, offs, wavs.reverb)
            if wavs.noise is not None:               # noise drawn by the loader: mixed in place, between gain and the STFT
                self.noise.mix_batch(flat, offs, wavs.noise, self.scale)
            lens = [offs[i + 1] - offs[i] for i in range(len(offs) - 1)]
        elif offsets is None:
            lens = [int(w.numel()) for w in wavs]
            flat = torch.cat([w.reshape(-1).to(self.device, torch.float32) for w in wavs])
        else:
            flat = wavs if (wavs.is_cuda and wavs.dtype == torch.float32 and wavs.is_contiguous()) \
                else wavs.to(self.device, torch.float32).contiguous()
            offsets = offsets.tolist() if hasattr(offsets, 'tolist') else offsets     # (Python ints: numpy scalars are 10x slower)
            lens = [offsets[i + 1] - offsets[i] for i in range(len(offsets) - 1)]
        offs = [0]
        for n in lens:
            offs.append(offs[-1] + n)
        frames = [1 + n // HOP for n in lens]
        t_max = max(frames)
        # (the offsets stay on the host, in page-locked memory the two kernels read in place: ops.spectrogram)
        inputs = ops.spectrogram(flat, torch.tensor(offs, dtype=torch.int64), t_max, self.normalize, self.eps)
        if spec is not None:                         # masks (+ warp) drawn by the loader: one launch behind the normalisation
            inputs = self.spec_augment.apply_batch(inputs, frames, spec)
        pct = torch.tensor([f / float(t_max) for f in frames], dtype=torch.float32)
        return inputs, pct


# ---------------------------------------------------------------------------------------------------------
# Neighbours of the hot path: waveform loading (+ augmentation, on the device) and
# transcript -> labels (host).
# ---------------------------------------------------------------------------------------------------------
class Compose(object):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class PCMClip(object):
    """What a loader worker hands on for one utterance: the int16 samples as read from the file plus the augmentation
    DRAWN for it (tempo factor, gain in dB; None = no augmentation; ``noise``: what ``NoiseInjection.draw`` returned;
    ``spec``: what ``SpecAugment.draw`` returned; ``reverb``: what ``Reverb.draw`` returned; ``speed``: what
    ``SpeedPerturb.draw`` returned).  The arithmetic -- speed perturbation of the int16 samples, int16 ->
    float, WSOLA tempo, gain, 16-bit requantisation, reverberation, noise mixing, and behind the spectrogram the SpecAugment
    masks -- happens on the GPU after collate (``ds2hip.ops.resample_var``, ``ds2hip.ops.decode_augment``,
    ``ds2hip.ops.reverb``, ``ds2hip.ops.noise_mix``, ``ds2hip.ops.spec_augment``)."""
    __slots__ = ('pcm', 'tempo', 'gain_db', 'noise', 'spec', 'reverb', 'speed')

    def __init__(self, pcm, tempo=None, gain_db=None, noise=None, spec=None, reverb=None, speed=None):
        self.pcm, self.tempo, self.gain_db, self.noise, self.spec = pcm, tempo, gain_db, noise, spec
        self.reverb, self.speed = reverb, speed

    def numel(self):
        return int(self.pcm.numel())


class RawAudioBatch(object):
    """A collated minibatch of ``PCMClip``s: ONE int16 buffer (page-locked when the DataLoader pins) + clip offsets +
    the per-clip augmentation parameters.  2 bytes per sample cross PCIe; everything else happens on the device.
    ``noise``: the clips' ``NoiseInjection.draw`` results (None for a clip without noise), or None when no clip drew any;
    ``spec``: the same for ``SpecAugment.draw``; ``reverb``: the same for ``Reverb.draw``; ``speed``: the same for
    ``SpeedPerturb.draw``."""

    def __init__(self, pcm, offsets, tempos=None, gains_db=None, noise=None, spec=None, reverb=None, speed=None):
        self.pcm, self.offsets, self.tempos, self.gains_db, self.noise = pcm, list(offsets), tempos, gains_db, noise
        self.spec, self.reverb, self.speed = spec, reverb, speed
        self.ready = None                            # event recorded behind an asynchronous upload (DevicePrefetcher)

    @classmethod
    def from_clips(cls, clips):
        offs = [0]
        for c in clips:
            offs.append(offs[-1] + c.numel())
        pcm = torch.cat([c.pcm.reshape(-1) for c in clips]) if clips else torch.zeros(0, dtype=torch.int16)
        aug = any(c.tempo is not None or c.gain_db is not None for c in clips)
        tempos = [1.0 if c.tempo is None else float(c.tempo) for c in clips] if aug else None
        gains = [0.0 if c.gain_db is None else float(c.gain_db) for c in clips] if aug else None
        noise = [c.noise for c in clips] if any(c.noise is not None for c in clips) else None
        spec = [c.spec for c in clips] if any(c.spec is not None for c in clips) else None
        reverb = [c.reverb for c in clips] if any(c.reverb is not None for c in clips) else None
        speed = [c.speed for c in clips] if any(c.speed is not None for c in clips) else None
        return cls(pcm, offs, tempos, gains, noise, spec, reverb, speed)

    def __len__(self):
        return len(self.offsets) - 1

    def pin_memory(self):                            # torch DataLoader(pin_memory=True) calls this on custom batch types
        self.pcm = self.pcm.pin_memory()
        return self

    def to(self, device, non_blocking=False):
        out = RawAudioBatch(self.pcm.to(device, non_blocking=non_blocking), self.offsets, self.tempos, self.gains_db,
                            self.noise, self.spec, self.reverb, self.speed)
        return out


class ToTensor(object):
    """16-bit PCM mono WAV -> waveform (reference ``codes/transforms.py:130-224``).

    The reference decodes with torchaudio and, with ``augment=True``, pipes every training clip through
    ``sox ... tempo T gain G`` (T, G drawn uniformly from the ranges, printed with three decimals).  Here a loader worker
    only READS the file's int16 samples and DRAWS (tempo, gain) exactly as the reference does (``np.random.uniform``,
    tempo first): with ``defer=True`` (what the training loader uses) it returns a ``PCMClip`` and the decode + WSOLA
    tempo + gain + 16-bit requantisation run on the GPU for the whole minibatch after collate; with ``defer=False``
    (the reference's per-clip contract) the same kernels run at once and a 1-D float tensor comes back.  ``noise`` (a
    ``NoiseInjection``, default None) adds its draw behind the two above -- nothing is drawn without it, so a seeded run
    without noise keeps its tempo / gain sequence -- and the clip's noise is mixed by the same device stage.
    ``spec_augment`` (a ``SpecAugment``, default None) adds ITS draw behind the noise draw, under the same rule, and the clip
    carries it to the ``BatchSpectrogram``: it needs ``defer=True`` (a waveform cannot carry a draw; in a per-clip pipeline
    the object itself stands behind ``ToSpectrogram``, where ``get_default_transforms`` puts it).  ``reverb`` (a ``Reverb``,
    default None) adds its draw BETWEEN the gain draw and the noise draw, under the same rule -- the order of the stages on
    the device: tempo, gain, reverberation, noise, spectrogram, SpecAugment.  ``speed`` (a ``SpeedPerturb``, default None)
    adds its draw IN FRONT of the tempo draw, under the same rule, and its stage runs on the int16 samples before everything
    else: speed, tempo, gain, reverberation, noise, spectrogram, SpecAugment.  There is no
    host implementation in the product; ``oracle/audio.py`` specifies the arithmetic (sox itself is absent from the
    reference tree, so the tempo change is the published WSOLA algorithm with sox's defaults, not sox's samples).

    ``scale`` is the amplitude contract of ``torchaudio.load`` (reference ``codes/transforms.py:156-161``), which changed
    between torchaudio versions and which the log1p of the spectrogram is NOT invariant to: ``'unit'`` (default) gives
    samples in [-1, 1) (int16 / 32768); ``'int32'`` gives int16 * 65536, the un-normalised floats of the mid-2018
    torchaudio master the released checkpoints were most likely trained with (unpinned: that torchaudio build is not in the
    reference tree).  With ``defer=True`` the scale is applied by the ``BatchSpectrogram`` that decodes the minibatch.

    The non-deferred path runs device kernels, so it cannot run inside a forked DataLoader worker (the child would have
    to re-initialise the GPU): it raises there -- use ``defer=True`` (what ``get_default_transforms`` builds) or
    ``num_workers=0``."""

    def __init__(self, sample_rate=16000, augment=False, tempo_range=(0.85, 1.15), gain_range=(-6, 8), defer=False,
                 device='cuda', scale=None, noise=None, spec_augment=None, reverb=None, speed=None):
        self.sample_rate, self.augment = sample_rate, augment
        self.tempo_range, self.gain_range = tempo_range, gain_range
        self.defer, self.device = defer, device
        self.noise, self.reverb, self.speed = noise, reverb, speed
        if spec_augment is not None and not defer:
            raise ValueError('ToTensor(spec_augment=...) needs defer=True: the draw travels with the clip to the '
                             'BatchSpectrogram; in a per-clip pipeline put the SpecAugment behind ToSpectrogram')
        self.spec_augment = spec_augment
        self.scale = ops.amplitude_scale(scale)

    def _load(self, path):
        import wave

        import numpy as np
        with wave.open(path, 'rb') as w:
            assert w.getframerate() == self.sample_rate, 'sample rate mismatch'
            assert w.getsampwidth() == 2 and w.getnchannels() == 1, 'expected 16-bit mono PCM'
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
        return torch.from_numpy(pcm.astype(np.int16, copy=True))

    def __call__(self, path):
        import numpy as np
        clip = PCMClip(self._load(path))
        if self.speed is not None:
            clip.speed = self.speed.draw()
        if self.augment:
            clip.tempo = float(np.random.uniform(low=self.tempo_range[0], high=self.tempo_range[1]))
            clip.gain_db = float(np.random.uniform(low=self.gain_range[0], high=self.gain_range[1]))
        if self.reverb is not None:
            clip.reverb = self.reverb.draw()
        if self.noise is not None:
            clip.noise = self.noise.draw()
        if self.spec_augment is not None:
            clip.spec = self.spec_augment.draw()
        if self.defer:
            return clip
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('ToTensor(defer=False) decodes on the GPU and cannot run in a DataLoader worker process; '
                               'build the transform with defer=True (the minibatch is then decoded on the device after '
                               'collate) or use num_workers=0')
        batch = RawAudioBatch.from_clips([clip]).to(self.device)
        pcm, offsets = batch.pcm, batch.offsets
        if batch.speed is not None:
            pcm, offsets = self.speed.apply_batch(pcm, offsets, batch.speed)
        wav, offs = ops.decode_augment(pcm, offsets, batch.tempos, batch.gains_db, self.sample_rate, scale=self.scale)
        if batch.reverb is not None:
            wav = self.reverb.apply_batch(wav, offs, batch.reverb)
        if batch.noise is not None:
            self.noise.mix_batch(wav, offs, batch.noise, self.scale)
        return wav.cpu()

    def __repr__(self):
        return '{}(sample_rate={}, augment={}, tempo_range={}, gain_range={})'.format(
            self.__class__.__name__, self.sample_rate, self.augment, self.tempo_range, self.gain_range)


def read_wav16(path, header_only=False):
    """A 16-bit PCM WAV file of any rate and 1..8 channels -> ``(interleaved int16 numpy array, rate, channels)``.  Any other
    sample width, compressed WAV and files that are not WAV raise ValueError with the file's name.  ``header_only``: check
    the format and return ``(None, rate, channels)``."""
    import wave

    import numpy as np
    try:
        with wave.open(path, 'rb') as w:
            channels, width, rate, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getcomptype()
            raw = b'' if header_only or width != 2 or comp != 'NONE' else w.readframes(w.getnframes())
    except (wave.Error, EOFError) as e:
        raise ValueError('%s: not a PCM WAV file (%s)' % (path, e))
    if width != 2 or comp != 'NONE':
        raise ValueError('%s: %d-bit samples; only 16-bit PCM is read (8-, 24- and 32-bit and float WAV are not)'
                         % (path, 8 * width))
    if not 1 <= channels <= ops.RESAMPLE_MAX_CHANNELS:
        raise ValueError('%s: %d channels; 1 .. %d are read' % (path, channels, ops.RESAMPLE_MAX_CHANNELS))
    if header_only:
        return None, rate, channels
    pcm = np.frombuffer(raw, dtype='<i2').astype(np.int16)
    return pcm[:len(pcm) // channels * channels], rate, channels


class Resample(object):
    """Sample-rate conversion and downmix on the device (``ds2hip.ops.resample``, ``ds2_resample``): interleaved int16 of
    any supported rate and 1..8 channels -> mono int16 at ``rate_out``, as a device tensor.  The filter is
    ``ops.resample_design(rate_in, rate_out)``: a decision of this project, not parity with sox (README "Sample-rate
    conversion").  A rate it has no filter for raises ``ValueError`` with the rate in the text.  Input at ``rate_out`` already
    goes through the same launch with the identity filter: mono comes out bit for bit, several channels as their mean."""

    def __init__(self, rate_out=16000, device='cuda'):
        self.rate_out, self.device = int(rate_out), device

    def batch(self, pcm, offsets, rate_in, channels=1):
        """The flat form: clip b = pcm[offsets[b] : offsets[b + 1]] (int16 numpy array or tensor, uploaded if it is not on the
        device yet) -> ``(out, out_offsets)``, one launch."""
        ops.resample_design(rate_in, self.rate_out)                     # (an unsupported rate is refused before the upload)
        pcm = torch.as_tensor(pcm)
        if pcm.dtype != torch.int16 or pcm.dim() != 1:
            raise ValueError('Resample takes 1-D int16 samples, got %s of shape %s' % (pcm.dtype, tuple(pcm.shape)))
        return ops.resample(pcm.to(self.device).contiguous(), offsets, rate_in, self.rate_out, channels)

    def __call__(self, pcm, rate_in, channels=1):
        """One clip -> its mono int16 samples at ``rate_out`` on the device."""
        pcm = torch.as_tensor(pcm)
        return self.batch(pcm, [0, int(pcm.numel())], rate_in, channels)[0]

    def __repr__(self):
        return '{}(rate_out={})'.format(self.__class__.__name__, self.rate_out)


def resample_files(paths, formats, rate_out, device):
    """The files of a bank whose header ``formats[i] = (rate, channels)`` is not (``rate_out``, 1), converted on ``device``
    with ONE launch per (rate, channels) group -> {path: mono int16 device tensor at rate_out}.  Files that need no
    conversion are not read and not in the result."""
    import numpy as np
    groups = {}
    for p, fmt in zip(paths, formats):
        if tuple(fmt) != (rate_out, 1):
            groups.setdefault(tuple(fmt), []).append(p)
    out = {}
    resampler = Resample(rate_out, device)
    for (rate, channels), members in sorted(groups.items()):
        parts = []
        for p in members:
            pcm, r, c = read_wav16(p)
            if (r, c) != (rate, channels):
                raise ValueError('{} is now {} Hz with {} channel(s), its header said {} Hz and {}'.format(p, r, c, rate, channels))
            parts.append(pcm)
        offsets = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).tolist()
        flat, out_off = resampler.batch(np.concatenate(parts), offsets, rate, channels)
        for i, p in enumerate(members):
            out[p] = flat[out_off[i]:out_off[i + 1]]
    return out


def _converted_frames(what, path, rate, width, chans, frames, rate_out):
    """A bank file that ``resample=True`` converts: refuse by name what cannot be converted (another sample width, more than
    eight channels, a rate without a filter) and return its length in samples at ``rate_out``."""
    if width != 2 or not 1 <= chans <= ops.RESAMPLE_MAX_CHANNELS:
        raise ValueError('{} {}: {} Hz, {} bit, {} channel(s); only 16-bit PCM with 1 .. {} channels is converted'.format(
            what, path, rate, 8 * width, chans, ops.RESAMPLE_MAX_CHANNELS))
    try:
        L, M, _ = ops.resample_design(rate, rate_out)
    except ValueError as e:
        raise ValueError('{} {}: {}'.format(what, path, e))
    return ops.resample_out_len(frames, L, M)


def noise_start(u, noise_len, n):
    """First sample of the noise crop for a clip of ``n`` samples, from the uniform draw ``u`` in [0, 1): the reference's
    ``torch.rand(()) * (noise_len - signal_len)`` in samples when the recording is at least as long as the clip (the crop
    then ends inside it); any position of the recording, which then repeats, when it is shorter.  Always in [0, noise_len)."""
    noise_len, n = int(noise_len), int(n)
    if noise_len >= n:
        return max(0, min(int(float(u) * (noise_len - n)), noise_len - n, noise_len - 1))
    return max(0, min(int(float(u) * noise_len), noise_len - 1))


class NoiseInjection(object):
    """Additive background noise at a random level (reference ``codes/transforms.py:227-292``).

    The reference's class cannot run: ``noise.size`` is a method, so the energy line raises (:268-269); ``prob`` is
    documented but neither stored nor applied; ``__repr__`` reads attributes that were never set; a noise file shorter than
    the clip fails the crop.  This is its evident intent, every decision written down:

    * ``path`` is searched recursively for ``.wav`` files, in sorted order (a missing directory raises ``IOError``, as in
      the reference).  Every file must be 16-bit mono PCM at ``sample_rate``: the reference resamples and downmixes through
      sox, which is not available here, so any other file is REFUSED by name -- convert the noise set once, offline
      (tools/resample_wav.py), or pass ``resample=True``: 16-bit files at another rate or with up to eight channels are then
      converted on the device when the bank is built (``resample_files``: one launch per (rate, channels) group).  An
      empty directory and a zero-length file are refused; a set longer than ``max_bank_seconds`` (one hour = 115 MB of
      int16 per GPU) raises ``ValueError`` rather than being truncated.
    * with probability ``prob`` a clip gets noise.  ``draw()`` -- what a loader worker calls -- returns None or
      ``(file index, level, u)`` from, in this order, ``np.random.binomial(1, prob)`` and then, only on a hit,
      ``np.random.choice(n_files)``, ``np.random.uniform(*noise_levels)`` and ``torch.rand(())``: the last three are the
      reference's own draws in its order (:257-262); the binomial in front is how the torchaudio fork the reference credits
      applied ``prob`` -- from recollection, that code is not in the reference tree.
    * the crop starts at ``noise_start(u, noise_len, n)`` once the clip's length after the tempo change is known; a
      recording shorter than the clip repeats.
    * ``out = x + level * rms(x) / rms(noise) * noise`` (the reference's formula with the rms its ancestor computes,
      ``sqrt(dot / size)``); a silent crop (or clip) adds nothing.  The sum is returned as floats, not requantised to 16 bit.

    The arithmetic is one device launch for a whole minibatch (``ds2hip.ops.noise_mix``): the recordings live on the GPU as
    one int16 bank, uploaded on first use in the process that owns the GPU (never in a loader worker; the workers only
    know the files' lengths).  ``ToTensor(noise=...)`` attaches the draw to its clip and ``BatchSpectrogram(noise=...)``
    mixes after decode, tempo and gain.  ``__call__(x)`` keeps the reference's per-clip contract through the same kernel
    (a CPU tensor makes a GPU round trip); ``scale`` is the amplitude contract of the waveform it is given
    (``ops.amplitude_scale``: the noise goes through the same conversion as the speech)."""

    def __init__(self, path, sample_rate=16000, noise_levels=(0, 0.5), prob=0.4, device='cuda', max_bank_seconds=3600,
                 scale=None, resample=False):
        import os
        import threading
        import wave
        if path is None or not os.path.isdir(path):
            raise IOError('Directory does not exist: {}'.format(path))
        self.path, self.sample_rate, self.prob = path, int(sample_rate), float(prob)
        self.resample = bool(resample)
        self.noise_levels = (float(noise_levels[0]), float(noise_levels[1]))
        self.device, self.max_bank_seconds = device, max_bank_seconds
        self.scale = ops.amplitude_scale(scale)
        self.paths = sorted(os.path.join(d, f) for d, _, files in os.walk(path) for f in files
                            if f.lower().endswith('.wav'))
        if not self.paths:
            raise ValueError('no .wav file under the noise directory {}'.format(path))
        self.lengths, self.formats = [], []          # (lengths: in samples of the bank, i.e. after a conversion)
        for p in self.paths:
            try:
                with wave.open(p, 'rb') as w:
                    rate, width, chans, frames = w.getframerate(), w.getsampwidth(), w.getnchannels(), w.getnframes()
            except (wave.Error, EOFError) as e:
                raise ValueError('noise file {} is not a PCM WAV file: {}'.format(p, e))
            if self.resample and (rate != self.sample_rate or chans != 1):
                frames = _converted_frames('noise file', p, rate, width, chans, frames, self.sample_rate)
            elif rate != self.sample_rate or width != 2 or chans != 1:
                raise ValueError('noise file {}: {} Hz, {} bit, {} channel(s); the noise bank takes 16-bit mono PCM at {} Hz '
                                 'only (nothing is resampled here: convert the file)'.format(p, rate, 8 * width, chans,
                                                                                            self.sample_rate))
            if frames <= 0:
                raise ValueError('noise file {} holds no samples'.format(p))
            self.formats.append((rate, chans))
            self.lengths.append(int(frames))
        total = sum(self.lengths)
        if total > max_bank_seconds * self.sample_rate:
            raise ValueError('the noise files under {} hold {:.1f} s of audio, more than max_bank_seconds = {} (the bank lives '
                             'on the GPU, 2 bytes per sample; nothing is truncated: raise the limit or thin the set)'.format(
                                 path, total / float(self.sample_rate), max_bank_seconds))
        self.starts = [0]
        for n in self.lengths[:-1]:
            self.starts.append(self.starts[-1] + n)
        self._banks, self._lock = {}, threading.Lock()

    def __getstate__(self):                          # (a spawned loader worker gets the description, never the device bank)
        state = dict(self.__dict__)
        state['_banks'], state['_lock'] = {}, None
        return state

    def __setstate__(self, state):
        import threading
        self.__dict__.update(state)
        self._lock = threading.Lock()

    def draw(self, rng=None):
        """None (no noise for this clip) or ``(file index, level, u)``.  ``rng`` (a ``numpy.random.RandomState`` or
        ``Generator``) replaces the global ``np.random`` -- and ``torch.rand`` for ``u`` -- when given."""
        import numpy as np
        r = np.random if rng is None else rng
        if not r.binomial(1, self.prob):
            return None
        index = int(r.choice(len(self.paths)))
        level = float(r.uniform(*self.noise_levels))
        u = float(torch.rand(())) if rng is None else float(r.uniform(0.0, 1.0))
        return index, level, u

    def bank(self, device=None):
        """The int16 samples of every file, concatenated in listing order, on ``device``: read and uploaded on first use."""
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('the noise bank lives on the GPU and cannot be used in a DataLoader worker process; let the '
                               'worker draw (ToTensor(noise=..., defer=True)) and mix after collate (BatchSpectrogram(noise=...))')
        device = torch.device(self.device if device is None else device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        with self._lock:
            bank = self._banks.get(device)
            if bank is None:
                loader = ToTensor(sample_rate=self.sample_rate)
                # (resample=True: the files at another rate or channel count, one launch per (rate, channels) group)
                conv = resample_files(self.paths, self.formats, self.sample_rate, device) if self.resample else {}
                parts = [conv[p] if p in conv else loader._load(p) for p in self.paths]
                for p, part, n in zip(self.paths, parts, self.lengths):
                    if part.numel() != n:
                        raise ValueError('noise file {} holds {} samples, its header says {}'.format(p, part.numel(), n))
                bank = self._banks[device] = torch.cat([part.to(device) for part in parts]) if conv else \
                    torch.cat(parts).to(device)
        return bank

    def params(self, draws, lens):
        """Per-clip (noise_lo, noise_len, noise_start, levels) for ``ops.noise_mix`` from the clips' draws and lengths."""
        lo, ln, st, lv = [], [], [], []
        for d, n in zip(draws, lens):
            if d is None:
                lo.append(0), ln.append(0), st.append(0), lv.append(0.0)
                continue
            index, level, u = d
            lo.append(self.starts[index]), ln.append(self.lengths[index]), lv.append(float(level))
            st.append(noise_start(u, self.lengths[index], n))
        return lo, ln, st, lv

    def mix_batch(self, flat, offsets, draws, scale, return_coef=False):
        """Mix the drawn noise into the flat float clips IN PLACE, one launch pair on the current stream."""
        lens = [offsets[i + 1] - offsets[i] for i in range(len(offsets) - 1)]
        lo, ln, st, lv = self.params(draws, lens)
        return ops.noise_mix(flat, offsets, self.bank(flat.device), lo, ln, st, lv, scale, out=flat,
                             return_coef=return_coef)

    def __call__(self, x):
        """x: 1-D float tensor of samples -> the same clip with (probability ``prob``) noise added, on x's device."""
        assert isinstance(x, torch.Tensor) and x.dim() == 1, 'Only mono audio is accepted'
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('NoiseInjection mixes on the GPU and cannot run in a DataLoader worker process; let the '
                               'worker draw (ToTensor(noise=..., defer=True)) and mix after collate, or use num_workers=0')
        draw = self.draw()
        if draw is None or x.numel() == 0:
            return x
        src = x.device
        wav = x.to(self.device, torch.float32).contiguous()
        if wav.data_ptr() == x.data_ptr():
            wav = wav.clone()
        self.mix_batch(wav, [0, wav.numel()], [draw], self.scale)
        return wav.to(src)

    def __repr__(self):
        return '{}({}, sample_rate={}, noise_levels={}, prob={}, files={}, seconds={:.1f})'.format(
            self.__class__.__name__, self.path, self.sample_rate, self.noise_levels, self.prob, len(self.paths),
            sum(self.lengths) / float(self.sample_rate))


def rir_from_pcm(pcm, max_taps):
    """The bank rule for one file: int16 samples -> float32 taps.  In float64, s = int16 / 32768; p = the first index of
    max |s|; h = s[p : p + max_taps] / s[p]; trailing zeros stripped; rounded to float32.  h[0] == 1 exactly.  An all-zero
    (or empty) file has no peak: ValueError."""
    import numpy as np
    s = np.asarray(pcm, np.int16).astype(np.float64).reshape(-1) / 32768.0
    if s.size == 0 or not np.any(s):
        raise ValueError('holds no impulse: every sample is zero' if s.size else 'holds no samples')
    p = int(np.argmax(np.abs(s)))
    h = s[p:p + int(max_taps)] / s[p]
    nz = np.flatnonzero(h)
    return h[:int(nz[-1]) + 1].astype(np.float32)


class Reverb(object):
    """Reverberation: with probability ``prob`` a clip is convolved with a room impulse response (RIR) drawn from the files
    under ``path``.  The reference has nothing of the kind, so every rule here is a decision (README "Reverberation"); nobody
    has measured the defaults' effect on WER in this model.

    * ``path`` is searched recursively for ``.wav`` files, in sorted order (a missing directory raises ``IOError``).  Every
      file must be 16-bit mono PCM at ``sample_rate`` = 16000; any other file is REFUSED by name -- another rate, width or
      channel count, an empty or all-zero file -- and so is an empty directory.  Nothing is resampled, unless
      ``resample=True``: 16-bit files at another rate or with up to eight channels are then converted to 16 kHz mono on the
      device when the object is built (one launch per (rate, channels) group) and the rule below runs on the int16 result.
    * per file (``rir_from_pcm``): the RIR starts at the file's largest |sample| and is divided by it, so ``h[0] == 1`` and the
      direct path is not delayed; what precedes the peak is dropped; at most ``int(max_rir_seconds * 16000)`` taps are kept,
      trailing zeros are stripped.  A set with more than ``max_bank_seconds`` of taps in total raises ``ValueError`` rather
      than being truncated (the bank lives on the GPU, 4 bytes per tap).
    * ``draw()`` -- what a loader worker calls -- returns None or the file index from, in this order,
      ``np.random.binomial(1, prob)`` and then, only on a hit, ``np.random.choice(n_files)``.
    * ``y[n] = sum_k h[k] x[n - k]`` in fp32: the clip keeps its length (the tail is cut), and the history before its first
      sample is zero.  The output is scaled back to the clip's own energy (``ops.reverb``'s ``keep_level``: the noise stage
      behind it sets its level relative to the clip's rms), and is returned as floats, not requantised to 16 bit.

    The arithmetic is one device launch pair for a whole minibatch (``ds2hip.ops.reverb``): the RIRs live on the GPU as one
    float32 bank, built and uploaded on first use in the process that owns the GPU (never in a loader worker: the workers
    only draw).  ``ToTensor(reverb=...)`` attaches the draw to its clip and ``BatchSpectrogram(reverb=...)`` convolves after
    decode, tempo and gain, before the noise.  ``__call__(x)`` is the per-clip contract through the same kernel (a CPU
    tensor makes a GPU round trip)."""

    def __init__(self, path, sample_rate=16000, prob=0.3, max_rir_seconds=0.5, max_bank_seconds=600, device='cuda',
                 resample=False):
        import os
        import threading
        import wave
        if path is None or not os.path.isdir(path):
            raise IOError('Directory does not exist: {}'.format(path))
        if int(sample_rate) != 16000:
            raise ValueError('Reverb works at 16000 Hz only (nothing is resampled here), got sample_rate = %r' % (sample_rate,))
        if not 0.0 <= float(prob) <= 1.0:
            raise ValueError('Reverb: prob must lie in [0, 1], got %r' % (prob,))
        self.path, self.sample_rate, self.prob = path, int(sample_rate), float(prob)
        self.max_rir_seconds, self.max_bank_seconds = max_rir_seconds, max_bank_seconds
        self.device, self.resample = device, bool(resample)
        self.max_taps = int(max_rir_seconds * self.sample_rate)
        if not 1 <= self.max_taps <= ops.REVERB_MAX_TAPS:
            raise ValueError('Reverb: max_rir_seconds = %r is %d taps; the kernel takes 1..%d'
                             % (max_rir_seconds, self.max_taps, ops.REVERB_MAX_TAPS))
        self.paths = sorted(os.path.join(d, f) for d, _, files in os.walk(path) for f in files
                            if f.lower().endswith('.wav'))
        if not self.paths:
            raise ValueError('no .wav file under the RIR directory {}'.format(path))
        # headers first (every refusal names its file), then the bank rule once per file: where the peak stands and where
        # the trailing zeros begin decide a file's tap count, which the size limit and ``params`` need, and an all-zero file
        # is refused here, before training starts, not at the first batch.  The taps are not kept: the bank is built on
        # first use in the process that owns the GPU
        # resample=True: the files at another rate or channel count are converted on the device HERE, one launch per (rate,
        # channels) group, and their 16 kHz samples (an RIR is short) are kept on the host for the rule above
        self.lengths, self._converted, formats = [], {}, []
        for p in self.paths:
            try:
                with wave.open(p, 'rb') as w:
                    rate, width, chans, frames = w.getframerate(), w.getsampwidth(), w.getnchannels(), w.getnframes()
            except (wave.Error, EOFError) as e:
                raise ValueError('RIR file {} is not a PCM WAV file: {}'.format(p, e))
            if self.resample and (rate != self.sample_rate or chans != 1):
                _converted_frames('RIR file', p, rate, width, chans, frames, self.sample_rate)
            elif rate != self.sample_rate or width != 2 or chans != 1:
                raise ValueError('RIR file {}: {} Hz, {} bit, {} channel(s); the RIR bank takes 16-bit mono PCM at {} Hz '
                                 'only (nothing is resampled here: convert the file)'.format(p, rate, 8 * width, chans,
                                                                                            self.sample_rate))
            if frames <= 0:
                raise ValueError('RIR file {} holds no samples'.format(p))
            formats.append((rate, chans))
        if self.resample:
            self._converted = {p: t.cpu().numpy() for p, t in
                               resample_files(self.paths, formats, self.sample_rate, device).items()}
        for p in self.paths:
            self.lengths.append(int(self._taps(p).size))
        total = sum(self.lengths)
        if total > max_bank_seconds * self.sample_rate:
            raise ValueError('the RIR files under {} hold {:.1f} s of taps, more than max_bank_seconds = {} (the bank lives '
                             'on the GPU, 4 bytes per tap; nothing is truncated: raise the limit or thin the set)'.format(
                                 path, total / float(self.sample_rate), max_bank_seconds))
        self.starts = [0]
        for n in self.lengths[:-1]:
            self.starts.append(self.starts[-1] + n)
        self._banks, self._lock = {}, threading.Lock()

    def _taps(self, p):
        import wave

        import numpy as np
        if p in self._converted:
            pcm = self._converted[p]
        else:
            with wave.open(p, 'rb') as w:
                pcm = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
        try:
            return rir_from_pcm(pcm, self.max_taps)
        except ValueError as e:
            raise ValueError('RIR file {} {}'.format(p, e))

    def __getstate__(self):                          # (a spawned loader worker gets the description, never the device bank)
        state = dict(self.__dict__)
        state['_banks'], state['_lock'] = {}, None
        return state

    def __setstate__(self, state):
        import threading
        self.__dict__.update(state)
        self._lock = threading.Lock()

    def draw(self, rng=None):
        """None (this clip stays dry) or the file index.  ``rng`` (a ``numpy.random.RandomState`` or ``Generator``)
        replaces the global ``np.random`` when given."""
        import numpy as np
        r = np.random if rng is None else rng
        if not r.binomial(1, self.prob):
            return None
        return int(r.choice(len(self.paths)))

    def bank(self, device=None):
        """The float32 taps of every file, concatenated in listing order, on ``device``: built and uploaded on first use."""
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('the RIR bank lives on the GPU and cannot be used in a DataLoader worker process; let the '
                               'worker draw (ToTensor(reverb=..., defer=True)) and convolve after collate '
                               '(BatchSpectrogram(reverb=...))')
        import numpy as np
        device = torch.device(self.device if device is None else device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        with self._lock:
            bank = self._banks.get(device)
            if bank is None:
                parts = [self._taps(p) for p in self.paths]
                for p, part, n in zip(self.paths, parts, self.lengths):
                    if part.size != n:
                        raise ValueError('RIR file {} gives {} taps, it gave {} at construction'.format(p, part.size, n))
                bank = self._banks[device] = torch.from_numpy(np.concatenate(parts)).to(device)
        return bank

    def params(self, draws):
        """Per-clip (rir_lo, rir_len) for ``ops.reverb`` from the clips' draws."""
        lo, ln = [], []
        for d in draws:
            lo.append(0 if d is None else self.starts[d]), ln.append(0 if d is None else self.lengths[d])
        return lo, ln

    def apply_batch(self, flat, offsets, draws, return_gain=False):
        """Convolve the drawn clips of the flat float buffer, one launch pair on the current stream.  Returns the NEW flat
        buffer (the convolution is out of place; undrawn clips are copied)."""
        lo, ln = self.params(draws)
        return ops.reverb(flat, offsets, self.bank(flat.device), lo, ln, True, return_gain=return_gain)

    def __call__(self, x):
        """x: 1-D float tensor of samples -> the same clip, reverberated with probability ``prob``, on x's device."""
        assert isinstance(x, torch.Tensor) and x.dim() == 1, 'Only mono audio is accepted'
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('Reverb convolves on the GPU and cannot run in a DataLoader worker process; let the worker '
                               'draw (ToTensor(reverb=..., defer=True)) and convolve after collate, or use num_workers=0')
        draw = self.draw()
        if draw is None or x.numel() == 0:
            return x
        wav = x.to(self.device, torch.float32).contiguous()
        return self.apply_batch(wav, [0, wav.numel()], [draw]).to(x.device)

    def __repr__(self):
        return '{}({}, sample_rate={}, prob={}, max_rir_seconds={}, files={}, taps={})'.format(
            self.__class__.__name__, self.path, self.sample_rate, self.prob, self.max_rir_seconds, len(self.paths),
            sum(self.lengths))


class SpeedPerturb(object):
    """Speed perturbation (Ko et al. 2015): with probability ``prob`` a clip is resampled by one of ``factors``, so that its
    duration and its pitch move together -- a factor above 1 shortens the clip and raises its pitch.  The reference has
    nothing of the kind (its ``tempo`` keeps the pitch), so every rule here is a decision (README "Speed perturbation");
    nobody has measured the defaults' effect on WER in this model.

    * ``factors`` are taken with three decimals and must lie in 0.5 .. 2.0; at most 15 distinct ones (a launch takes 16
      tables and the identity takes one).  Factor f is the table ``ops.speed_design(f)``: the conversion from 16000 f Hz to
      16000 Hz of ``ops.resample_design``, the same Kaiser filter as everywhere else.
    * ``draw()`` -- what a loader worker calls -- returns None or the index into ``factors`` from, in this order,
      ``np.random.binomial(1, prob)`` and then, only on a hit, ``np.random.choice(len(factors))``.
    * a clip of n samples comes out with ``ceil(n L / M)`` samples, M / L = f reduced; int16 in, int16 out, rounded half to
      even and saturated.  A clip without a draw (and factor 1.0) is copied bit for bit.

    The arithmetic is ONE device launch for a whole minibatch, every clip with its own table, without a host wait
    (``ds2hip.ops.resample_var``, ``ds2_resample_var``); the tables live on the GPU as one float32 bank, uploaded on first use
    in the process that owns the GPU (never in a loader worker: the workers only draw).  ``ToTensor(speed=...)`` attaches the
    draw to its clip and ``BatchSpectrogram(speed=...)`` resamples the int16 clips before decode, tempo and gain.
    ``__call__(x)`` is the per-clip contract on a 1-D int16 tensor through the same kernel."""

    MAX_FACTORS = ops.RESAMPLE_VAR_TABLES - 1

    def __init__(self, factors=(0.9, 1.0, 1.1), prob=1.0, device='cuda'):
        try:
            factors = list(factors)
        except TypeError:
            raise ValueError('SpeedPerturb: factors must be a sequence of numbers, got %r' % (factors,))
        if not factors:
            raise ValueError('SpeedPerturb: factors is empty')
        try:
            self.factors = tuple(ops.speed_factor(f) for f in factors)
        except ValueError as e:
            raise ValueError('SpeedPerturb: factors: %s' % e)
        if len(set(self.factors)) > self.MAX_FACTORS:
            raise ValueError('SpeedPerturb: factors holds %d distinct values; at most %d (one launch takes %d tables and the '
                             'identity takes one)' % (len(set(self.factors)), self.MAX_FACTORS, ops.RESAMPLE_VAR_TABLES))
        if isinstance(prob, bool) or not 0.0 <= float(prob) <= 1.0:
            raise ValueError('SpeedPerturb: prob must lie in [0, 1], got %r' % (prob,))
        self.prob, self.device = float(prob), device
        # table 0 is the identity (clips without a draw); every distinct factor has one table, in order of first appearance
        self._distinct = [1.0] + [f for i, f in enumerate(self.factors) if f != 1.0 and f not in self.factors[:i]]
        self._table_of = tuple(self._distinct.index(f) for f in self.factors)
        self._tables = None

    def __getstate__(self):                          # (a spawned loader worker gets the description, never the tables)
        state = dict(self.__dict__)
        state['_tables'] = None
        return state

    def draw(self, rng=None):
        """None (this clip keeps its speed) or the index into ``factors``.  ``rng`` (a ``numpy.random.RandomState`` or
        ``Generator``) replaces the global ``np.random`` when given."""
        import numpy as np
        r = np.random if rng is None else rng
        if not r.binomial(1, self.prob):
            return None
        return int(r.choice(len(self.factors)))

    def tables(self):
        """The ``(L, M, taps)`` of ``ops.resample_var``: the identity, then one per distinct factor.  Designed on first use."""
        if self._tables is None:
            self._tables = [ops.speed_design(f) for f in self._distinct]
        return self._tables

    def table_ids(self, draws):
        """Per-clip table index for ``ops.resample_var`` from the clips' draws (None: the identity)."""
        return [0 if d is None else self._table_of[d] for d in draws]

    def out_len(self, n, draw):
        """Samples a clip of ``n`` samples has behind the stage."""
        L, M, _ = self.tables()[self.table_ids([draw])[0]]
        return ops.resample_out_len(n, L, M)

    def apply_batch(self, pcm, offsets, draws):
        """Resample the flat int16 clips on the device, one launch on the current stream, no host wait.  Returns the NEW flat
        int16 buffer and its offsets (a python list); clips without a draw are copied."""
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('SpeedPerturb resamples on the GPU and cannot run in a DataLoader worker process; let the '
                               'worker draw (ToTensor(speed=..., defer=True)) and resample after collate '
                               '(BatchSpectrogram(speed=...))')
        return ops.resample_var(pcm, offsets, self.table_ids(draws), self.tables())

    def __call__(self, x):
        """x: 1-D int16 tensor of samples -> the clip at the drawn speed (probability ``prob``), on x's device."""
        assert isinstance(x, torch.Tensor) and x.dim() == 1 and x.dtype == torch.int16, 'expected 1-D int16 samples'
        draw = self.draw()
        if draw is None or x.numel() == 0:
            return x
        pcm = x.to(self.device).contiguous()
        return self.apply_batch(pcm, [0, pcm.numel()], [draw])[0].to(x.device)

    def __repr__(self):
        return '{}(factors={}, prob={})'.format(self.__class__.__name__, self.factors, self.prob)


class SpecAugment(object):
    """SpecAugment (Park et al. 2019) on the log-spectrogram: a time warp, ``freq_masks`` frequency masks and ``time_masks``
    time masks per clip.  The reference has nothing of the kind -- its augmentation is tempo, gain and noise, all on the
    waveform -- so every rule here is a decision (README "SpecAugment").  The defaults are the paper's, which were defined on
    80 mel bins; here they meet 161 linear bins, and nobody has measured their effect on WER in this model.

    * with probability ``prob`` a clip is augmented.  ``draw()`` -- what a loader worker calls; it knows neither the GPU nor
      the clip's length -- returns None or a tuple of uniform variates from, in this order, ``np.random.binomial(1, prob)``
      and then, only on a hit, ONE ``np.random.uniform(0, 1, size=n)`` with n = 2 [time_warp > 0] + 2 freq_masks +
      2 time_masks: warp (centre, shift), every frequency mask (width, start), every time mask (width, start).
    * ``params(draws, frames)`` resolves them once the clip's frame count T is known (after the tempo change); every
      floor(u k) is clamped to k - 1.  Frequency: f = floor(u (freq_width + 1)), f0 = floor(u' (161 - f + 1)).  Time:
      cap = min(time_width, floor(time_ratio T)), t = floor(u (cap + 1)), t0 = floor(u' (T - t + 1)).  Warp, W = time_warp,
      only when T > 2 W (the identity otherwise): c = W + floor(u (T - 2 W)), c2 = c + floor(u' (2 W + 1)) - W -- source
      frame c lands on output frame c2, both halves resampled linearly.  A None draw is the identity warp and no mask.
    * masked cells are SET to ``mask_value`` (0 = the clip's mean after the frontend's normalisation).

    ``ToTensor(spec_augment=...)`` attaches the draw to its clip and ``BatchSpectrogram(spec_augment=...)`` applies the
    batch's draws in one launch behind the spectrogram (``ds2hip.ops.spec_augment``; in place when ``time_warp == 0``).
    ``__call__(spect)`` is the per-clip contract through the same kernel (a CPU tensor makes a GPU round trip)."""

    def __init__(self, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=0.2, time_warp=0, prob=1.0,
                 mask_value=0.0, device='cuda'):
        def whole(name, v, lo, hi=None):
            if isinstance(v, bool) or int(v) != v or v < lo or (hi is not None and v > hi):
                raise ValueError('SpecAugment: %s must be an integer %s, got %r'
                                 % (name, 'in %d..%d' % (lo, hi) if hi is not None else '>= %d' % lo, v))
            return int(v)
        self.freq_masks = whole('freq_masks', freq_masks, 0, ops.SPEC_MAX_MASKS)
        self.freq_width = whole('freq_width', freq_width, 0, NBINS)
        self.time_masks = whole('time_masks', time_masks, 0, ops.SPEC_MAX_MASKS)
        self.time_width = whole('time_width', time_width, 0)
        self.time_warp = whole('time_warp', time_warp, 0)
        for name, v in (('time_ratio', time_ratio), ('prob', prob)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError('SpecAugment: %s must lie in [0, 1], got %r' % (name, v))
        self.time_ratio, self.prob, self.mask_value, self.device = float(time_ratio), float(prob), float(mask_value), device

    def draw(self, rng=None):
        """None (this clip stays as it is) or the clip's uniform variates.  ``rng`` (a ``numpy.random.RandomState`` or
        ``Generator``) replaces the global ``np.random`` when given."""
        import numpy as np
        r = np.random if rng is None else rng
        if not r.binomial(1, self.prob):
            return None
        n = 2 * (self.time_warp > 0) + 2 * self.freq_masks + 2 * self.time_masks
        return tuple(float(u) for u in r.uniform(0, 1, size=n))

    def params(self, draws, frames):
        """(warp, fmask, tmask) for ``ops.spec_augment`` from the clips' draws and frame counts: python lists of shape
        (B, 2), (B, freq_masks, 2), (B, time_masks, 2); warp is None when ``time_warp == 0``."""
        import math

        def fl(u, k):                                # floor(u k) for u in [0, 1), never k itself
            return min(int(math.floor(float(u) * k)), k - 1)
        w = self.time_warp
        warp, fmask, tmask = ([] if w > 0 else None), [], []
        for d, t_b in zip(draws, frames):
            t_b = int(t_b)
            if d is None:
                if w > 0:
                    warp.append([0, 0])
                fmask.append([[0, 0]] * self.freq_masks), tmask.append([[0, 0]] * self.time_masks)
                continue
            u = list(d)
            if w > 0:
                uc, us = u[0], u[1]
                u = u[2:]
                if t_b > 2 * w:
                    c = w + fl(uc, t_b - 2 * w)
                    warp.append([c, c + fl(us, 2 * w + 1) - w])
                else:
                    warp.append([0, 0])
            row = []
            for m in range(self.freq_masks):
                f = fl(u[2 * m], self.freq_width + 1)
                row.append([fl(u[2 * m + 1], NBINS - f + 1), f])
            fmask.append(row)
            u = u[2 * self.freq_masks:]
            cap = min(self.time_width, int(math.floor(self.time_ratio * t_b)))
            row = []
            for m in range(self.time_masks):
                t = fl(u[2 * m], cap + 1)
                row.append([fl(u[2 * m + 1], t_b - t + 1), t])
            tmask.append(row)
        return warp, fmask, tmask

    def apply_batch(self, inputs, frames, draws):
        """Apply the clips' draws to ``inputs`` (B, t_max, 161) on the device, one launch on the current stream: in place
        when ``time_warp == 0``, into a new tensor otherwise.  Returns the tensor that holds the result."""
        warp, fmask, tmask = self.params(draws, frames)
        return ops.spec_augment(inputs, frames, warp, fmask, tmask, self.mask_value)

    def __call__(self, spect):
        """spect: (T, 161) float tensor -> the augmented spectrogram (probability ``prob``), on spect's device."""
        assert isinstance(spect, torch.Tensor) and spect.dim() == 2 and spect.shape[1] == NBINS, 'expected (T, 161)'
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError('SpecAugment masks on the GPU and cannot run in a DataLoader worker process; let the worker '
                               'draw (ToTensor(spec_augment=..., defer=True)) and mask after collate '
                               '(BatchSpectrogram(spec_augment=...)), or use num_workers=0')
        draw = self.draw()
        if draw is None or spect.shape[0] == 0:
            return spect
        src = spect.device
        x = spect.to(self.device, torch.float32).contiguous()
        if x.data_ptr() == spect.data_ptr():
            x = x.clone()                            # (the caller's tensor is not written)
        return self.apply_batch(x.unsqueeze(0), [x.shape[0]], [draw])[0].to(src)

    def __repr__(self):
        return ('{}(freq_masks={}, freq_width={}, time_masks={}, time_width={}, time_ratio={}, time_warp={}, prob={}, '
                'mask_value={})').format(self.__class__.__name__, self.freq_masks, self.freq_width, self.time_masks,
                                         self.time_width, self.time_ratio, self.time_warp, self.prob, self.mask_value)


def waveform_spec_augment(transform):
    """The ``SpecAugment`` whose draws the ``ToTensor`` stage of ``transform`` attaches to its clips (None when there is
    none): what the ``BatchSpectrogram`` that decodes those clips must be built with."""
    for t in getattr(transform, 'transforms', [transform]):
        if isinstance(t, ToTensor):
            return t.spec_augment
    return None


def waveform_speed(transform):
    """The ``SpeedPerturb`` whose draws the ``ToTensor`` stage of ``transform`` attaches to its clips (None when there is
    none): what the ``BatchSpectrogram`` that decodes those clips must be built with."""
    for t in getattr(transform, 'transforms', [transform]):
        if isinstance(t, ToTensor):
            return t.speed
    return None


def waveform_reverb(transform):
    """The ``Reverb`` whose draws the ``ToTensor`` stage of ``transform`` attaches to its clips (None when there is none):
    what the ``BatchSpectrogram`` that decodes those clips must be built with."""
    for t in getattr(transform, 'transforms', [transform]):
        if isinstance(t, ToTensor):
            return t.reverb
    return None


def waveform_noise(transform):
    """The ``NoiseInjection`` whose draws the ``ToTensor`` stage of ``transform`` attaches to its clips (None when there is
    none): what the ``BatchSpectrogram`` that decodes those clips must be built with."""
    for t in getattr(transform, 'transforms', [transform]):
        if isinstance(t, ToTensor):
            return t.noise
    return None


def waveform_scale(transform):
    """The amplitude scale of the ``ToTensor`` stage of ``transform`` (1/32768 when there is none): what the
    ``BatchSpectrogram`` that decodes its deferred clips must apply."""
    for t in getattr(transform, 'transforms', [transform]):
        if isinstance(t, ToTensor):
            return t.scale
    return ops.UNIT_SCALE


_ACCENT_FOLD = {'À': 'A', 'Á': 'A', 'Â': 'A', 'Ã': 'A', 'Ä': 'A', 'Ç': 'C', 'È': 'E', 'É': 'E', 'Ê': 'E', 'Ë': 'E',
                'Ì': 'I', 'Í': 'I', 'Î': 'I', 'Ï': 'I', 'Ñ': 'N', 'Ò': 'O', 'Ó': 'O', 'Ô': 'O', 'Õ': 'O', 'Ö': 'O',
                'Ù': 'U', 'Ú': 'U', 'Û': 'U', 'Ü': 'U'}


class ToLabel(object):
    """Transcript (string or path) -> (L,1) int array of label ids (reference ``codes/transforms.py:295-392``).

    Upper-cases, optionally folds accents (a fixed Latin-1 table stands in for ``unidecode``), drops every
    character that is not in the label set.  Number-to-words conversion (``num2words``, absent here) is NOT
    applied.  In the reference the conversion runs AFTER upper-casing (``codes/transforms.py:370-376``) and
    num2words writes lower-case words, so with the upper-case alphabets of ``data/labels.*.json`` every letter
    of the spelled-out number is filtered again and only the spaces between its words survive: "I HAVE 2 DOGS"
    becomes "I HAVE  DOGS" there and here alike; a multi-word number ("1,234") leaves a few more spaces in the
    reference than here -- a documented deviation (LibriSpeech transcripts contain no digits)."""

    def __init__(self, labels='labels.en.json', to_upper=True, one_hot=False, convert_number_to_words=True, lang=None,
                 remove_accents=True, dtype=None):
        import os

        import numpy as np

        from .preprocessing import OrderedLabelEncoder
        from .utils.io_utils import read_labels
        if one_hot:
            raise NotImplementedError('one-hot targets are not used by the CTC path')
        if isinstance(labels, str) and os.path.isfile(labels):
            labels_list = read_labels(labels)
            lang = lang or labels.split('.')[-2]
        else:
            labels_list = list(labels)
        self._labels, self._lang, self._to_upper = labels, lang, to_upper
        self._remove_accents = remove_accents
        self._dtype = dtype or np.int64
        self.label_encoder = OrderedLabelEncoder().fit(labels_list)
        self._known = set(self.label_encoder.classes_.tolist())

    def __call__(self, x):
        import os

        import numpy as np
        if isinstance(x, bytes):
            x = x.decode('utf8')
        if os.path.isfile(x):
            with open(x, 'r', encoding='utf8') as f:
                x = f.readline().strip()
        if self._to_upper:
            x = x.upper()
        if self._remove_accents:
            x = ''.join(_ACCENT_FOLD.get(c, c) for c in x)
        chars = [c for c in x if c in self._known]
        ids = np.asarray(self.label_encoder.transform(chars), dtype=self._dtype).reshape(-1)
        return ids[:, np.newaxis]
