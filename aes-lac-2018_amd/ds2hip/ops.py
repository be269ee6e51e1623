"""Tensor-level wrappers over the C ABI: allocate outputs with torch, launch HIP kernels.

Every function takes/returns ROCm device tensors (fp32 unless noted).  PyTorch is used only as
the allocator and stream owner; all arithmetic happens inside libds2hip.so.
"""
import os

import torch

from . import lib

F_BINS = 161
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _bytes_ws(nbytes, like):
    return torch.empty((int(nbytes) + 15) // 16 * 2, dtype=torch.float64, device=like.device)


def conv_out_frames(t_in):
    t1 = (t_in + 20 - 11) // 2 + 1
    return t1, t1 - 10


# ----------------------------------------------------------------------------- frontend
def spectrogram(wav, wav_offsets, t_max, normalize=True, eps=1e-9):
    """wav: concatenated clips (sum L,), wav_offsets (B+1,) int64 -> (B, t_max, 161).  ``wav_offsets`` on the device, or a
    HOST tensor: it is then staged in page-locked memory the kernels read in place (no copy; ``_PinnedRing.stage``)."""
    bsz = wav_offsets.numel() - 1
    out = _empty((bsz, t_max, F_BINS), wav)
    ws = _bytes_ws(lib.query('ds2_spectrogram_ws_bytes', bsz, t_max), wav)
    if wav_offsets.is_cuda:
        lib.call('ds2_spectrogram_fwd', wav, wav_offsets, bsz, t_max, int(normalize), float(eps), out, ws)
    else:
        slot, staged = _staged.stage(wav_offsets)
        try:
            lib.call('ds2_spectrogram_fwd', wav, staged.data_ptr(), bsz, t_max, int(normalize), float(eps), out, ws)
        finally:
            _staged.staged_done(wav_offsets.dtype, slot)
    return out



# ----------------------------------------------------------------------------- waveform decode + augmentation
WSOLA_MS = (82.0, 14.68, 12.0)          # sox `tempo` defaults: segment, search, overlap


def wsola_params(sample_rate=16000):
    seg = max(int(sample_rate * WSOLA_MS[0] / 1000.0), 4)
    ovl = max(min(int(sample_rate * WSOLA_MS[2] / 1000.0), seg // 2), 1)
    half = max(int(sample_rate * WSOLA_MS[1] / 1000.0) // 2, 1)
    return seg, ovl, half


def wsola_schedule(n, tempo, sample_rate=16000):
    """Segment schedule of one clip (data independent): int32 array of rounded ideal input positions + output length.
    ``tempo`` is used with three decimals, as on the reference's sox command line (codes/transforms.py:197-199)."""
    import numpy as np
    seg, ovl, half = wsola_params(sample_rate)
    tempo = float('{:.3f}'.format(tempo))
    if abs(tempo - 1.0) < 1e-6 or n <= seg + half:
        return np.zeros(0, np.int32), n
    hop_out = seg - ovl
    kmax = int(n / (tempo * hop_out)) + 4
    base = np.rint(np.cumsum(np.full(kmax, tempo * hop_out, dtype=np.float64))).astype(np.int64)   # running sum, half-even
    dead = np.minimum(base + half, n - seg) < np.maximum(base - half, 0)
    nseg = int(np.argmax(dead)) if dead.any() else kmax
    return base[:nseg].astype(np.int32), (nseg + 1) * hop_out + ovl


UNIT_SCALE = 1.0 / 32768.0


def amplitude_scale(spec):
    """The waveform amplitude contract (what ``torchaudio.load`` returned, reference ``codes/transforms.py:156-161``):
    ``'unit'`` / None -> 1/32768 (samples in [-1, 1)); ``'int32'`` -> 65536 (the un-normalised int32-range floats of the
    mid-2018 torchaudio master: sox hands a 16-bit sample on as a 32-bit one); or a positive number."""
    if spec is None or spec == 'unit':
        return UNIT_SCALE
    if spec == 'int32':
        return 65536.0
    scale = float(spec)
    if not scale > 0:
        raise ValueError('amplitude scale must be positive, got %r' % (spec,))
    return scale


def decode_augment(pcm, offsets, tempos=None, gains_db=None, sample_rate=16000, scale=UNIT_SCALE):
    """pcm: concatenated int16 clips on the device; offsets: python list (B+1).  Returns (float clips concatenated,
    new offsets list).  ``tempos`` / ``gains_db`` (per clip, or None): the training-set augmentation -- WSOLA tempo,
    then gain in dB and 16-bit requantisation -- entirely on the device.  ``scale``: a sample of value q (int16, or the
    requantised integer after augmentation) comes out as q * scale (``amplitude_scale``).

    The 16-bit requantisation belongs to the GAIN step (sox writes a 16-bit file at the end of ``tempo T gain G``,
    codes/transforms.py:185-218, and the reference never draws one without the other): it happens exactly when ``gains_db`` is
    given, at every amplitude scale.  A tempo-only call (a diagnostic path: the WSOLA kernel against its specification) returns
    the float WSOLA output times ``scale / UNIT_SCALE`` -- the same samples at every scale, up to that factor."""
    import numpy as np
    wav = _empty((pcm.numel(),), pcm)
    if tempos is None and gains_db is None:
        lib.call('ds2_pcm16_to_float', pcm, pcm.numel(), float(scale), wav)
        return wav, list(offsets)
    lib.call('ds2_pcm16_to_float', pcm, pcm.numel(), UNIT_SCALE, wav)      # the augmentation works on [-1, 1)
    bsz = len(offsets) - 1
    lens = [offsets[i + 1] - offsets[i] for i in range(bsz)]
    if tempos is not None:
        sched = [wsola_schedule(n, t, sample_rate) for n, t in zip(lens, tempos)]
        out_offs = [0]
        for _, m in sched:
            out_offs.append(out_offs[-1] + m)
        boffs = np.concatenate([[0], np.cumsum([len(b) for b, _ in sched])]).astype(np.int32)
        bases = np.concatenate([b for b, _ in sched] + [np.zeros(1, np.int32)]).astype(np.int32)
        # one upload: int64 offsets (in, out) then the int32 schedule viewed as int64 pairs
        meta = np.concatenate([np.asarray(offsets, np.int64), np.asarray(out_offs, np.int64)])
        meta_d = upload_small(torch.from_numpy(meta), pcm.device)
        sched_d = upload_small(torch.from_numpy(np.concatenate([boffs, bases])), pcm.device)
        seg, ovl, half = wsola_params(sample_rate)
        out = _empty((out_offs[-1],), pcm)
        lib.call('ds2_wsola_tempo', wav, meta_d[:bsz + 1], meta_d[bsz + 1:], sched_d[bsz + 1:], sched_d[:bsz + 1], bsz,
                 seg, ovl, half, out)
        wav, offsets = out, out_offs
    if gains_db is not None:
        g = torch.tensor([10.0 ** (float('{:.3f}'.format(v)) / 20.0) for v in gains_db], dtype=torch.float32)
        offs_d = upload_small(torch.tensor(list(offsets), dtype=torch.int64), pcm.device)
        lib.call('ds2_gain_requantize', wav, offs_d, upload_small(g, pcm.device), bsz, float(scale), wav)
    elif scale != UNIT_SCALE:
        wav.mul_(float(scale) / UNIT_SCALE)
    return wav, list(offsets)


NOISE_CHUNK = 4096                      # DS2_NOISE_CHUNK of include/ds2hip.h: samples per workgroup of ds2_noise_mix


def noise_mix(wav, offsets, bank, noise_lo, noise_len, noise_start, levels, noise_scale, out=None, return_coef=False,
              ws=None):
    """Additive background noise for a minibatch in one launch pair on the current stream (``ds2_noise_mix``).
    wav: the flat float clips ``decode_augment`` returns, offsets: its python list (B+1).  bank: every noise recording's
    int16 samples concatenated on the device; per clip (python sequences of length B) ``noise_lo`` / ``noise_len`` the
    recording (length 0 = no noise for this clip), ``noise_start`` the first sample of the crop, ``levels`` the drawn level.
    Returns the mixed flat buffer (``out``, which may be ``wav`` itself; a new tensor when None), and the per-clip
    coefficients (B,) float32 on the device with ``return_coef``.  ``ws``: a caller's uint8 workspace of at least
    ``ds2_noise_mix_ws_bytes`` bytes (its contents do not matter); allocated here when None."""
    import numpy as np
    bsz = len(offsets) - 1
    if not (wav.is_cuda and bank.is_cuda) or wav.dtype != torch.float32 or bank.dtype != torch.int16:
        raise RuntimeError('noise_mix takes a float32 waveform buffer and an int16 noise bank, both on the device')
    off = np.asarray(offsets, np.int64)
    lo, ln, st = (np.asarray(v, np.int64).reshape(-1) for v in (noise_lo, noise_len, noise_start))
    lv = np.asarray(levels, np.float32).reshape(-1)
    if not (len(lo) == len(ln) == len(st) == len(lv) == bsz >= 1):
        raise ValueError('noise_mix: one (noise_lo, noise_len, noise_start, level) per clip, got %d / %d / %d / %d for %d clips'
                         % (len(lo), len(ln), len(st), len(lv), bsz))
    if off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > wav.numel():
        raise ValueError('noise_mix: offsets do not describe clips inside the waveform buffer')
    drawn = ln > 0
    if (ln < 0).any() or (lo[drawn] < 0).any() or (lo[drawn] + ln[drawn] > bank.numel()).any():
        raise ValueError('noise_mix: a noise recording lies outside the bank (%d samples)' % bank.numel())
    if ((st[drawn] < 0) | (st[drawn] >= ln[drawn])).any():
        raise ValueError('noise_mix: noise_start must lie inside its recording')
    if not np.isfinite(lv).all():
        raise ValueError('noise_mix: noise levels must be finite')
    # one upload: the four int64 arrays, then the float levels viewed as int64 pairs
    lv_pad = np.zeros(2 * ((bsz + 1) // 2), np.float32)
    lv_pad[:bsz] = lv
    meta_d = upload_small(torch.from_numpy(np.concatenate([off, lo, ln, st, lv_pad.view(np.int64)])), wav.device)
    a = bsz + 1
    ws_bytes = lib.query('ds2_noise_mix_ws_bytes', bsz, int(np.diff(off).max()))
    if ws is None:
        ws = torch.empty((int(ws_bytes),), dtype=torch.uint8, device=wav.device)
    elif ws.dtype != torch.uint8 or ws.numel() < ws_bytes:
        raise ValueError('noise_mix: the workspace must be uint8 of at least %d bytes' % ws_bytes)
    if out is None:
        out = torch.empty_like(wav)
        if off[0] > 0 or off[-1] < wav.numel():          # (samples outside every clip pass through)
            out.copy_(wav)
    coef = _empty((bsz,), wav) if return_coef else None
    lib.call('ds2_noise_mix', wav, meta_d[:a], bsz, bank, meta_d[a:a + bsz], meta_d[a + bsz:a + 2 * bsz],
             meta_d[a + 2 * bsz:a + 3 * bsz], meta_d[a + 3 * bsz:].view(torch.float32), float(noise_scale), out, coef, ws,
             int(ws_bytes))
    return (out, coef) if return_coef else out


REVERB_TILE = 2048                      # DS2_REVERB_TILE of include/ds2hip.h: outputs of one clip per workgroup of ds2_reverb
REVERB_TAPS_STEP = 512                  # DS2_REVERB_TAPS_STEP: taps staged per pass
REVERB_MAX_TAPS = 65536                 # DS2_REVERB_MAX_TAPS: taps of one RIR


def reverb(wav, offsets, bank, rir_lo, rir_len, keep_level=True, out=None, return_gain=False, ws=None):
    """Reverberation for a minibatch in one launch pair on the current stream (``ds2_reverb``): every drawn clip is convolved
    with its room impulse response, keeps its length and (``keep_level``) its energy.
    wav: the flat float clips ``decode_augment`` returns, offsets: its python list (B+1).  bank: every RIR's float32 taps
    concatenated on the device; per clip (python sequences of length B) ``rir_lo`` / ``rir_len`` the RIR (length 0 = no
    draw: the clip is copied bit for bit).  Returns the new flat buffer (``out``, never ``wav`` itself; a new tensor when
    None, with the samples outside every clip copied from ``wav``), and the per-clip gains (B,) float32 on the device with
    ``return_gain``.  ``ws``: a caller's uint8 workspace of at least ``ds2_reverb_ws_bytes`` bytes (its contents do not
    matter); allocated here when None."""
    import numpy as np
    bsz = len(offsets) - 1
    if not (isinstance(wav, torch.Tensor) and isinstance(bank, torch.Tensor) and wav.is_cuda and bank.is_cuda) or \
            wav.dtype != torch.float32 or bank.dtype != torch.float32:
        raise RuntimeError('reverb takes a float32 waveform buffer and a float32 RIR bank, both on the device')
    off = np.asarray(offsets, np.int64)
    lo, ln = (np.asarray(v, np.int64).reshape(-1) for v in (rir_lo, rir_len))
    if not (len(lo) == len(ln) == bsz >= 1):
        raise ValueError('reverb: one (rir_lo, rir_len) per clip, got %d / %d for %d clips' % (len(lo), len(ln), bsz))
    if off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > wav.numel():
        raise ValueError('reverb: offsets do not describe clips inside the waveform buffer')
    drawn = ln > 0
    if (ln < 0).any() or (lo[drawn] < 0).any() or (lo[drawn] + ln[drawn] > bank.numel()).any():
        raise ValueError('reverb: an impulse response lies outside the bank (%d taps)' % bank.numel())
    if (ln > REVERB_MAX_TAPS).any():
        raise ValueError('reverb: an impulse response has %d taps, more than %d' % (int(ln.max()), REVERB_MAX_TAPS))
    if out is None:
        out = torch.empty_like(wav)
        if off[0] > 0 or off[-1] < wav.numel():          # (samples outside every clip pass through)
            out.copy_(wav)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
              and out.numel() >= int(off[-1])):
        raise ValueError('reverb: out must be a contiguous float32 device tensor that holds every clip')
    else:
        a0, a1 = wav.data_ptr(), wav.data_ptr() + 4 * wav.numel()
        b0, b1 = out.data_ptr(), out.data_ptr() + 4 * out.numel()
        if a0 < b1 and b0 < a1:
            raise ValueError('reverb: out overlaps wav; the convolution is out of place (every output reads K inputs)')
    meta_d = upload_small(torch.from_numpy(np.concatenate([off, lo, ln])), wav.device)      # one upload
    a = bsz + 1
    ws_bytes = lib.query('ds2_reverb_ws_bytes', bsz, int(np.diff(off).max()))
    if ws is None:
        ws = torch.empty((int(ws_bytes),), dtype=torch.uint8, device=wav.device)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < ws_bytes:
        raise ValueError('reverb: the workspace must be uint8 on the device, of at least %d bytes' % ws_bytes)
    gain = _empty((bsz,), wav) if return_gain else None
    lib.call('ds2_reverb', wav, meta_d[:a], bsz, bank, meta_d[a:a + bsz], meta_d[a + bsz:], int(bool(keep_level)), out, gain,
             ws, int(ws.numel()))
    return (out, gain) if return_gain else out


RESAMPLE_TILE = 1024                    # DS2_RESAMPLE_TILE of include/ds2hip.h: outputs of one clip per workgroup tile
RESAMPLE_MAX_L, RESAMPLE_MAX_M, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_CHANNELS = 1024, 4096, 1023, 8      # ds2_resample's limits
RESAMPLE_RATES = (4000, 192000)         # input rates resample_design takes

_resample_designs = {}


def resample_design(rate_in, rate_out=16000, zeros=24, rolloff=0.95, beta=9.0):
    """The polyphase filter of a conversion ``rate_in`` -> ``rate_out``: ``(L, M, taps)`` with L / M the reduced ratio and taps
    an (L, K) float32 array, K odd, for ``ds2_resample``.  A Kaiser-windowed sinc with ``zeros`` zero crossings on either
    side, cut off at ``rolloff`` times the lower Nyquist frequency; computed in float64 on the host, rounded to float32 once
    and cached per argument tuple.  The defaults are a decision of this project, not parity with sox (include/ds2hip.h)."""
    import math
    import numpy as np
    key = (rate_in, rate_out, zeros, rolloff, beta)
    if key in _resample_designs:
        return _resample_designs[key]
    if isinstance(rate_in, bool) or int(rate_in) != rate_in or not RESAMPLE_RATES[0] <= rate_in <= RESAMPLE_RATES[1]:
        raise ValueError('resample: a sample rate of %r Hz is not supported (%d .. %d Hz)' % ((rate_in,) + RESAMPLE_RATES))
    if isinstance(rate_out, bool) or int(rate_out) != rate_out or rate_out < 1 or zeros < 1 or not 0 < rolloff <= 1:
        raise ValueError('resample: cannot design a filter for %r Hz out, %r zero crossings, roll-off %r'
                         % (rate_out, zeros, rolloff))
    rate_in, rate_out = int(rate_in), int(rate_out)
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    if L > RESAMPLE_MAX_L or M > RESAMPLE_MAX_M:
        raise ValueError('resample: a sample rate of %d Hz is not supported: %d Hz is %d / %d of it, and the filter bank '
                         'takes ratios up to %d / %d' % (rate_in, rate_out, L, M, RESAMPLE_MAX_L, RESAMPLE_MAX_M))
    if L == M:                                   # equal rates: the identity (one tap of 1), so only the downmix is left
        taps = np.ones((1, 1), np.float32)
        taps.setflags(write=False)
        _resample_designs[key] = (1, 1, taps)
        return _resample_designs[key]
    c = rolloff * min(1.0, L / M)
    half = int(math.ceil(zeros / c))
    K = 2 * half + 1
    if K > RESAMPLE_MAX_TAPS:
        raise ValueError('resample: a sample rate of %d Hz is not supported: its filter has %d taps per phase, more than %d'
                         % (rate_in, K, RESAMPLE_MAX_TAPS))
    u = (np.arange(K, dtype=np.float64)[None, :] - half) - np.arange(L, dtype=np.float64)[:, None] / L
    a = np.abs(u) * c / zeros
    win = np.i0(beta * np.sqrt(np.maximum(1.0 - a * a, 0.0))) / np.i0(beta)
    taps = np.where(a > 1.0, 0.0, c * np.sinc(c * u) * win).astype(np.float32)
    taps.setflags(write=False)
    _resample_designs[key] = (L, M, taps)
    return _resample_designs[key]


def resample_out_len(n_frames, L, M):
    """ds2_resample_out_len: outputs of a clip of ``n_frames`` frames at the ratio L / M."""
    return (int(n_frames) * L + M - 1) // M


_resample_taps_dev = {}


def resample(pcm, offsets, rate_in, rate_out=16000, channels=1, taps=None):
    """Sample-rate conversion and downmix for a flat buffer of clips in one launch on the current stream (``ds2_resample``).
    pcm: 1-D int16 on the device, clip b = pcm[offsets[b] : offsets[b + 1]] with ``channels`` interleaved channels;
    offsets: python sequence (B+1), in elements.  ``taps``: None for ``resample_design(rate_in, rate_out)``, or ``(L, M, taps)``
    with taps an (L, K) float32 array or device tensor.  Returns ``(out, out_offsets)``: the mono int16 clips at ``rate_out``,
    concatenated in a new device tensor, and their offsets as a python list."""
    import numpy as np
    if not isinstance(pcm, torch.Tensor) or not pcm.is_cuda or pcm.dtype != torch.int16 or pcm.dim() != 1:
        raise RuntimeError('resample takes a 1-D int16 tensor on the device')
    if not pcm.is_contiguous():
        raise RuntimeError('ds2hip entry points take contiguous tensors')
    channels = int(channels)
    if not 1 <= channels <= RESAMPLE_MAX_CHANNELS:
        raise ValueError('resample: %d channels, not 1 .. %d' % (channels, RESAMPLE_MAX_CHANNELS))
    if taps is None:
        L, M, table = resample_design(rate_in, rate_out)
        key = (rate_in, rate_out, pcm.device)
        taps_d = _resample_taps_dev.get(key)
        if taps_d is None:
            taps_d = _resample_taps_dev[key] = torch.from_numpy(np.array(table)).to(pcm.device)
    else:
        L, M, table = taps
        L, M = int(L), int(M)
        taps_d = table if isinstance(table, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(table, np.float32))
        if taps_d.dtype != torch.float32 or taps_d.dim() != 2 or taps_d.shape[0] != L:
            raise ValueError('resample: taps must be an (L, K) float32 table, L = %d' % L)
        taps_d = taps_d.to(pcm.device).contiguous()
    K = int(taps_d.shape[1])
    if not (1 <= L <= RESAMPLE_MAX_L and 1 <= M <= RESAMPLE_MAX_M and 1 <= K <= RESAMPLE_MAX_TAPS and K % 2 == 1):
        raise ValueError('resample: ratio %d / %d with %d taps per phase; L in 1..%d, M in 1..%d, taps odd in 1..%d'
                         % (L, M, K, RESAMPLE_MAX_L, RESAMPLE_MAX_M, RESAMPLE_MAX_TAPS))
    off = np.asarray(offsets, np.int64).reshape(-1)
    bsz = len(off) - 1
    if not 1 <= bsz <= 65535:
        raise ValueError('resample: %d clips, not 1 .. 65535' % bsz)
    lens = np.diff(off)
    if off[0] < 0 or (lens < 0).any() or off[-1] > pcm.numel():
        raise ValueError('resample: offsets do not describe clips inside the sample buffer')
    if (lens % channels != 0).any():
        b = int(np.argmax(lens % channels != 0))
        raise ValueError('resample: clip %d holds %d samples, not a whole number of %d-channel frames' % (b, lens[b], channels))
    out_off = np.concatenate([[0], np.cumsum((lens // channels * L + M - 1) // M)]).astype(np.int64)
    out = torch.empty((int(out_off[-1]),), dtype=torch.int16, device=pcm.device)
    if out_off[-1] > 0:
        meta_d = upload_small(torch.from_numpy(np.concatenate([off, out_off])), pcm.device)      # one upload
        lib.call('ds2_resample', pcm, meta_d[:bsz + 1], bsz, channels, L, M, taps_d, K, out, meta_d[bsz + 1:])
    return out, [int(v) for v in out_off]


RESAMPLE_VAR_TABLES = 16                # DS2_RESAMPLE_VAR_TABLES of include/ds2hip.h: tables of one ds2_resample_var launch
SPEED_RANGE = (0.5, 2.0)                # factors speed_design takes


def speed_factor(factor):
    """A speed factor as the kernel's table is designed for it: three decimals, as the tempo draw is printed.  Outside
    ``SPEED_RANGE`` (or not a number): ValueError naming the value."""
    if isinstance(factor, bool) or not isinstance(factor, (int, float)) or not SPEED_RANGE[0] <= factor <= SPEED_RANGE[1]:
        raise ValueError('speed: a factor of %r is not supported (%s .. %s)' % ((factor,) + SPEED_RANGE))
    return float('{:.3f}'.format(factor))


def speed_design(factor):
    """The polyphase filter of speed perturbation by ``factor`` (taken with three decimals): ``(L, M, taps)`` of
    ``resample_design(16 * round(1000 * factor))`` -- a conversion from 16000 * factor Hz to 16000 Hz, so M / L = factor
    reduced, L <= 1000, and the filter, its roll-off and its cache are the existing design's.  A factor above 1 shortens the
    clip and raises its pitch; 1.0 is the identity (one tap of 1)."""
    return resample_design(16 * int(round(1000 * speed_factor(factor))))


_resample_var_banks = {}


def _resample_var_bank(tables, device):
    """(device tap bank, (T, 4) int32 host array of {L, M, K, tap_offset}) for a list of ``(L, M, taps)``.  Cached per
    (tables, device) when every taps array is read-only (what ``resample_design`` returns: its identity stands for its
    contents); a writable array is uploaded per call."""
    import numpy as np
    if not 1 <= len(tables) <= RESAMPLE_VAR_TABLES:
        raise ValueError('resample_var: %d tables, not 1 .. %d' % (len(tables), RESAMPLE_VAR_TABLES))
    frozen = all(isinstance(t[2], np.ndarray) and not t[2].flags.writeable for t in tables)
    key = (tuple((int(L), int(M), id(taps)) for L, M, taps in tables), device)
    if frozen and key in _resample_var_banks:
        return _resample_var_banks[key][:2]
    desc, parts, pos = [], [], 0
    for i, (L, M, taps) in enumerate(tables):
        L, M = int(L), int(M)
        table = np.ascontiguousarray(taps.cpu().numpy() if isinstance(taps, torch.Tensor) else taps)
        if table.dtype != np.float32 or table.ndim != 2 or table.shape[0] != L:
            raise ValueError('resample_var: table %d: taps must be an (L, K) float32 table, L = %d' % (i, L))
        K = int(table.shape[1])
        if not (1 <= L <= RESAMPLE_MAX_L and 1 <= M <= RESAMPLE_MAX_M and 1 <= K <= RESAMPLE_MAX_TAPS and K % 2 == 1):
            raise ValueError('resample_var: table %d: ratio %d / %d with %d taps per phase; L in 1..%d, M in 1..%d, taps odd in '
                             '1..%d' % (i, L, M, K, RESAMPLE_MAX_L, RESAMPLE_MAX_M, RESAMPLE_MAX_TAPS))
        desc.append((L, M, K, pos))
        parts.append(table.reshape(-1))
        pos += L * K
    bank = torch.from_numpy(np.concatenate(parts)).to(device)
    desc = np.asarray(desc, np.int32).reshape(-1, 4)
    if frozen:
        _resample_var_banks[key] = (bank, desc, [t[2] for t in tables])      # (the arrays stay alive: their ids stay theirs)
    return bank, desc


def resample_var(pcm, offsets, table_ids, tables):
    """Per-clip sample-rate conversion of a flat buffer of mono clips in ONE launch on the current stream, without a host
    wait (``ds2_resample_var``): speed perturbation.  pcm: 1-D int16 on the device, clip b = pcm[offsets[b] : offsets[b + 1]];
    offsets: python sequence (B+1); ``table_ids``: B indices into ``tables``, a list of up to 16 ``(L, M, taps)`` with taps an
    (L, K) float32 array (``speed_design`` / ``resample_design``).  Returns ``(out, out_offsets)`` as ``resample`` does; a clip's
    samples are bit for bit those of ``resample`` on that clip alone with its table."""
    import numpy as np
    if not isinstance(pcm, torch.Tensor) or not pcm.is_cuda or pcm.dtype != torch.int16 or pcm.dim() != 1:
        raise RuntimeError('resample_var takes a 1-D int16 tensor on the device')
    if not pcm.is_contiguous():
        raise RuntimeError('ds2hip entry points take contiguous tensors')
    tables = list(tables)
    bank, desc = _resample_var_bank(tables, pcm.device)
    off = np.asarray(offsets, np.int64).reshape(-1)
    ids = np.asarray(table_ids, np.int64).reshape(-1)
    bsz = len(off) - 1
    if not 1 <= bsz <= 65535:
        raise ValueError('resample_var: %d clips, not 1 .. 65535' % bsz)
    if len(ids) != bsz:
        raise ValueError('resample_var: %d table ids for %d clips' % (len(ids), bsz))
    if ((ids < 0) | (ids >= len(tables))).any():
        b = int(np.argmax((ids < 0) | (ids >= len(tables))))
        raise ValueError('resample_var: clip %d names table %d; there are %d' % (b, ids[b], len(tables)))
    lens = np.diff(off)
    if off[0] < 0 or (lens < 0).any() or off[-1] > pcm.numel():
        raise ValueError('resample_var: offsets do not describe clips inside the sample buffer')
    n_out = (lens * desc[ids, 0].astype(np.int64) + desc[ids, 1] - 1) // desc[ids, 1]
    if n_out.max() >= 2 ** 31:
        raise ValueError('resample_var: a clip of %d outputs; fewer than 2^31' % n_out.max())
    out_off = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    out = torch.empty((int(out_off[-1]),), dtype=torch.int16, device=pcm.device)
    if out_off[-1] > 0:
        ids_pad = np.zeros(2 * ((bsz + 1) // 2), np.int32)
        ids_pad[:bsz] = ids
        # one upload: the two int64 offset arrays, then the int32 ids viewed as int64 pairs
        meta_d = upload_small(torch.from_numpy(np.concatenate([off, out_off, ids_pad.view(np.int64)])), pcm.device)
        a = bsz + 1
        lib.call('ds2_resample_var', pcm, meta_d[:a], meta_d[a:2 * a], meta_d[2 * a:].view(torch.int32), bsz,
                 desc.ctypes.data, len(tables), bank, int(bank.numel()), int(n_out.max()), out)
    return out, [int(v) for v in out_off]


VAD_BLOCK = 160                        # DS2_VAD_BLOCK of include/ds2hip.h: samples per block of ds2_vad_segment (10 ms)
VAD_BINS = 192                          # DS2_VAD_BINS: level bins


def vad_segment(pcm, rank, margin_bins, min_bin, max_bin, min_speech, min_silence, pad, max_len, seg_cap=None, ws=None):
    """Speech segments of one recording on the current stream (``ds2_vad_segment``; the rule is in include/ds2hip.h).
    pcm: 1-D int16 on the device, at 16 kHz (a slice of a larger tensor is fine).  The other arguments are in blocks of 160
    samples and level bins.  Returns ``(segs, info)``: segs (n_seg, 2) int32 on the HOST, rows [start_block, end_block) in
    ascending order, and info = {n_seg, floor_bin, thr, speech_blocks, nb}; one readback brings both.  ``seg_cap``: rows
    to provide (default: the rule's bound nb // min(min_speech, h) + 1); more segments than that raise.  ``ws``: a caller's
    uint8 workspace of at least ``ds2_vad_segment_ws_bytes`` bytes (its contents do not matter); allocated here when None."""
    if not isinstance(pcm, torch.Tensor) or not pcm.is_cuda or pcm.dtype != torch.int16 or pcm.dim() != 1:
        raise RuntimeError('vad_segment takes a 1-D int16 tensor on the device')
    if not pcm.is_contiguous():
        raise RuntimeError('ds2hip entry points take contiguous tensors')
    n = int(pcm.numel())
    nb = (n + VAD_BLOCK - 1) // VAD_BLOCK
    if seg_cap is None:
        seg_cap = nb // max(min(int(min_speech), (int(max_len) + 1) // 2), 1) + 1
    seg_cap = int(seg_cap)
    ws_bytes = lib.query('ds2_vad_segment_ws_bytes', n)
    if ws is None:
        ws = torch.empty((int(ws_bytes),), dtype=torch.uint8, device=pcm.device)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < ws_bytes:
        raise ValueError('vad_segment: the workspace must be uint8 on the device, of at least %d bytes' % ws_bytes)
    out = torch.empty((8 + 2 * max(seg_cap, 0),), dtype=torch.int32, device=pcm.device)      # info, then the rows
    lib.call('ds2_vad_segment', pcm.data_ptr() if n else None, n, int(rank), int(margin_bins), int(min_bin), int(max_bin),
             int(min_speech), int(min_silence), int(pad), int(max_len), ws, ws.numel(), out[8:], seg_cap, out[:8])
    host = out.cpu()
    n_seg = int(host[0])
    if n_seg > seg_cap:
        raise RuntimeError('vad_segment: %d segments do not fit seg_cap = %d' % (n_seg, seg_cap))
    info = dict(zip(('n_seg', 'floor_bin', 'thr', 'speech_blocks', 'nb'), host[:5].tolist()))
    return host[8:].view(-1, 2)[:n_seg].clone(), info


SPEC_MAX_MASKS = 8                      # masks of one kind per clip ds2_spec_augment takes
SPEC_MAX_WARP_FRAMES = 4096             # with a warp: frame products stay exact in float (include/ds2hip.h)


def _spec_table(name, table, shape):
    """A per-clip table given as a list or a tensor -> int32 numpy of ``shape`` (one -1 allowed; None or empty: no entries)."""
    import numpy as np
    if isinstance(table, torch.Tensor):
        table = table.detach().cpu().numpy()
    arr = np.asarray([] if table is None else table)
    if arr.size == 0:
        arr = np.zeros([0 if d == -1 else d for d in shape], np.int64)
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError('spec_augment: %s must hold integers, got %s' % (name, arr.dtype))
    try:
        arr = arr.astype(np.int64).reshape(shape)
    except ValueError:
        raise ValueError('spec_augment: %s has shape %s, expected %s' % (name, arr.shape, tuple(shape)))
    if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
        raise ValueError('spec_augment: %s does not fit 32-bit integers' % name)
    return np.ascontiguousarray(arr, np.int32)


def spec_augment(x, frames, warp=None, fmask=None, tmask=None, mask_value=0.0, out=None):
    """SpecAugment for a minibatch in one launch on the current stream (``ds2_spec_augment``).
    x: (B, t_max, 161) float32 on the device, what ``spectrogram`` returns; frames: the clips' valid frames (B).  Per clip
    (python lists or tensors of integers): ``warp`` (B, 2) = (c, c2), source frame c lands on output frame c2 (c2 == c: not
    warped), or None; ``fmask`` (B, MF, 2) = (f0, f) and ``tmask`` (B, MT, 2) = (t0, t), start and width (width 0: no mask;
    masks are clamped to the clip), MF, MT <= 8, or None.  Masked cells become ``mask_value``; frames past a clip's own are 0.
    Without a warp the masks are stored IN PLACE (``out`` None or ``x``: x is returned); with a warp, or with another ``out``,
    every cell of ``out`` (allocated here when None; never ``x``) is written.  Returns the tensor that holds the result."""
    import numpy as np
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3 or \
            x.shape[2] != F_BINS or not x.is_contiguous():
        raise RuntimeError('spec_augment takes a contiguous float32 (B, t_max, %d) tensor on the device' % F_BINS)
    bsz, t_max = int(x.shape[0]), int(x.shape[1])
    if bsz < 1 or t_max < 1:
        raise ValueError('spec_augment: an empty batch')
    fr = _spec_table('frames', frames, (bsz,))
    if (fr < 1).any() or (fr > t_max).any():
        raise ValueError('spec_augment: every clip has 1..t_max = %d frames, got %s' % (t_max, fr.tolist()))
    parts = [fr]
    if warp is not None:
        wp = _spec_table('warp', warp, (bsz, 2))
        if (fr > SPEC_MAX_WARP_FRAMES).any():
            raise ValueError('spec_augment: a time warp takes clips of at most %d frames, got %d'
                             % (SPEC_MAX_WARP_FRAMES, int(fr.max())))
        if (wp < 0).any() or (wp >= fr[:, None]).any():
            raise ValueError('spec_augment: warp (c, c2) must lie inside the clip, 0 <= c, c2 < frames')
        parts.append(wp.reshape(-1))
    fm, tm = _spec_table('fmask', fmask, (bsz, -1, 2)), _spec_table('tmask', tmask, (bsz, -1, 2))
    n_f, n_t = fm.shape[1], tm.shape[1]
    if n_f > SPEC_MAX_MASKS or n_t > SPEC_MAX_MASKS:
        raise ValueError('spec_augment: %d frequency and %d time masks per clip, at most %d of a kind are taken'
                         % (n_f, n_t, SPEC_MAX_MASKS))
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()):
        raise ValueError('spec_augment: out must be a contiguous tensor like x')
    in_place = warp is None and (out is None or out.data_ptr() == x.data_ptr())
    if in_place:
        out = x
        if n_f == 0 and n_t == 0:
            return out                                   # nothing to do
    elif out is None:
        out = torch.empty_like(x)
    elif out.data_ptr() == x.data_ptr():
        raise ValueError('spec_augment: a time warp cannot work in place, out must be another tensor than x')
    # one upload: frames, then warp, fmask, tmask (int32 each)
    meta_d = upload_small(torch.from_numpy(np.concatenate(parts + [fm.reshape(-1), tm.reshape(-1)])), x.device)
    a = bsz + (2 * bsz if warp is not None else 0)
    lib.call('ds2_spec_augment', x, out, bsz, t_max, meta_d[:bsz], meta_d[bsz:a] if warp is not None else None,
             meta_d[a:a + 2 * bsz * n_f] if n_f else None, n_f,
             meta_d[a + 2 * bsz * n_f:] if n_t else None, n_t, float(mask_value))
    return out


# ----------------------------------------------------------------------------- small host <-> device transfers
class _PinnedRing(object):
    """A few reusable page-locked staging buffers per dtype: ``tensor.pin_memory()`` allocates page-locked memory
    on every call (~0.1-0.3 ms of host time each, with the GPU idle at the start of a step).  A slot is reused only
    after the copy that last read it has completed (event per slot); a slot handed out by ``stage`` is BUSY until
    ``staged_done`` and is skipped meanwhile (the ring grows if every slot is busy).  One lock per ring: frontends run on the
    prefetch thread of a loader as well as on the main thread."""

    def __init__(self, slots=4):
        import threading
        self.slots, self.ring, self.next, self.lock = slots, {}, {}, threading.Lock()

    def _slot(self, dtype, n, busy=False):
        """(under the lock) index and buffer of the next slot that is not busy; marks it busy if asked."""
        ring = self.ring.setdefault(dtype, [None] * self.slots)
        start = self.next.get(dtype, 0)
        i = None
        for d in range(len(ring)):
            j = (start + d) % len(ring)
            if ring[j] is None or not ring[j][2]:
                i = j
                break
        if i is None:                             # every slot is between stage() and staged_done(): one more
            ring.append(None)
            i = len(ring) - 1
        self.next[dtype] = (i + 1) % len(ring)
        buf, ev = (ring[i][0], ring[i][1]) if ring[i] is not None else (None, None)
        if ev is not None:
            ev.synchronize()
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(64, 2 * n), dtype=dtype).pin_memory()
        ring[i] = (buf, None, busy)
        return i, buf

    def upload(self, host_tensor, device):
        """1-D CPU tensor -> device tensor through a pinned slot, asynchronously on the current stream."""
        n = host_tensor.numel()
        with self.lock:
            i, buf = self._slot(host_tensor.dtype, n)
            buf[:n].copy_(host_tensor.reshape(-1))
            out = torch.empty(n, dtype=host_tensor.dtype, device=device)
            out.copy_(buf[:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.ring[host_tensor.dtype][i] = (buf, ev, False)
        return out

    def stage(self, host_tensor):
        """1-D CPU tensor -> a page-locked copy the DEVICE reads in place (its address is valid there): for a few dozen bytes a
        kernel reads once, the host-to-device copy costs more than the reads over the bus -- and, issued into an idle queue at
        the top of a step, ~50-80 us before it even starts (kernel trace).  Call ``staged_done(i)`` behind the last launch that
        reads it: until then the slot is busy, afterwards it is reused only once that launch has completed."""
        n = host_tensor.numel()
        with self.lock:
            i, buf = self._slot(host_tensor.dtype, n, busy=True)
            view = buf[:n]
            view.copy_(host_tensor.reshape(-1))
        return i, view

    def staged_done(self, dtype, i):
        ev = torch.cuda.Event()
        ev.record()
        with self.lock:
            self.ring[dtype][i] = (self.ring[dtype][i][0], ev, False)

    def download(self, dev_tensor):
        """1-D device tensor -> pinned host view; valid once the returned event has completed."""
        n = dev_tensor.numel()
        with self.lock:
            i, buf = self._slot(dev_tensor.dtype, n)
            buf[:n].copy_(dev_tensor.reshape(-1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.ring[dev_tensor.dtype][i] = (buf, ev, False)
        return buf[:n], ev


_pinned = _PinnedRing()
_staged = _PinnedRing()          # device-read-in-place staging has its own ring: uploads never wait behind a staged slot


def upload_small(host_tensor, device):
    return _pinned.upload(host_tensor, device)


def download_small(dev_tensor):
    return _pinned.download(dev_tensor)


def spin_wait(event):
    """Poll an event instead of a blocking ``synchronize()`` (which sleeps on an interrupt and wakes up ~0.1 ms late).
    ``sleep(0)`` hands the GIL to any other thread that wants it -- the DataLoader's pin-memory thread, a prefetcher --
    and returns at once when none does: a bare ``while not query(): pass`` starves them for the whole step."""
    import time
    while not event.query():
        time.sleep(0)


def low_priority_stream(device):
    """A torch stream object on a LOW-priority HIP stream (torch.cuda.Stream cannot create one: it clamps to [-1, 0])."""
    import ctypes
    with torch.cuda.device(device):
        out = ctypes.c_void_p()
        rc = lib.load().ds2_stream_create(1, ctypes.byref(out))
        if rc != 0:
            raise RuntimeError('ds2_stream_create failed (%d): %s' % (rc, lib.load().ds2_last_error().decode()))
        return torch.cuda.ExternalStream(out.value, device=device)

# ----------------------------------------------------------------------------- GEMM
def gemm(a, b, trans_a=False, trans_b=False, out=None, beta=0.0, m=None, n=None, k=None, lda=None, ldb=None,
         ldc=None, split_k=1):
    """C = op(a) @ op(b) (+ beta*C).  a, b 2-D row-major unless explicit dims/ld are given."""
    if m is None:
        m = a.shape[1] if trans_a else a.shape[0]
    if k is None:
        k = a.shape[0] if trans_a else a.shape[1]
    if n is None:
        n = b.shape[0] if trans_b else b.shape[1]
    if lda is None:
        lda = a.shape[-1]
    if ldb is None:
        ldb = b.shape[-1]
    if out is None:
        out = _empty((m, n), a)
    if ldc is None:
        ldc = out.shape[-1]
    lib.call('ds2_gemm_f32', int(trans_a), int(trans_b), m, n, k, a, lda, b, ldb, out, ldc, float(beta), split_k)
    return out


def gemm_split_mode(mode=-1):
    """Select the GEMM kernel family (0: f32-input MFMA, 6 / 9: bf16 split-operand kernels, include/ds2hip.h); returns the
    one in effect.  -1 only queries."""
    return int(lib.load().ds2_gemm_split_mode(int(mode)))


def gemm_raw(trans_a, trans_b, m, n, k, a_ptr, lda, b_ptr, ldb, c_ptr, ldc, beta=0.0, split_k=1):
    """Pointer-level GEMM for sub-matrix views (pointers are ints = data_ptr() + byte offsets)."""
    lib.call('ds2_gemm_f32', int(trans_a), int(trans_b), m, n, k, a_ptr, lda, b_ptr, ldb, c_ptr, ldc, float(beta),
             split_k)


def gemm_tn_group(problems, n, k, accumulate=False):
    """Up to four TN problems sharing N and K in one launch: ``problems`` = [(a_ptr, lda, m, b_ptr, ldb, c_ptr, ldc), ...]
    with device pointers as ints.  C_p[m_p, n] = A_p^T B_p (A_p stored k x m_p); ``accumulate``: C_p += instead (the caller
    has zeroed C, e.g. the whole flat gradient in one fill)."""
    import ctypes
    cnt = len(problems)
    assert 1 <= cnt <= 4
    vp, ip = ctypes.c_void_p * cnt, ctypes.c_int * cnt
    a, lda, m, b, ldb, c, ldc = zip(*problems)
    args = (vp(*a), ip(*lda), ip(*m), vp(*b), ip(*ldb), vp(*c), ip(*ldc))
    fn = lib.load().ds2_gemm_f32_tn_group
    rc = fn(cnt, *[ctypes.cast(x, ctypes.c_void_p) for x in args], int(n), int(k), int(bool(accumulate)),
            lib.stream_ptr())
    if rc != 0:
        raise lib.Ds2Error(rc, 'ds2_gemm_f32_tn_group failed (%d): %s' % (rc, lib.load().ds2_last_error().decode()))


def transpose2d(x, rows, cols, out=None):
    if out is None:
        out = _empty((cols, rows), x)
    lib.call('ds2_transpose2d', x, rows, cols, out)
    return out


def transpose2d_group(tensors, batch, rows, cols, out):
    """``tensors``: up to 8 device tensors of ``batch`` row-major (rows, cols) matrices each -> out (len, batch, cols, rows), ONE
    launch (ds2_transpose2d_group)."""
    import ctypes
    cnt = len(tensors)
    assert 1 <= cnt <= 8 and all(t.is_cuda and t.is_contiguous() and t.numel() == batch * rows * cols for t in tensors)
    assert out.is_cuda and out.is_contiguous() and out.numel() == cnt * batch * rows * cols
    ptrs = (ctypes.c_void_p * cnt)(*[t.data_ptr() for t in tensors])
    rc = lib.load().ds2_transpose2d_group(cnt, ctypes.cast(ptrs, ctypes.c_void_p), int(batch), int(rows), int(cols),
                                          out.data_ptr(), lib.stream_ptr())
    if rc != 0:
        raise lib.Ds2Error(rc, 'ds2_transpose2d_group failed (%d): %s' % (rc, lib.load().ds2_last_error().decode()))
    return out


def add2(a, b):
    out = torch.empty_like(a)
    lib.call('ds2_add2', a, b, a.numel(), out)
    return out


# ----------------------------------------------------------------------------- conv stack
def transpose_btf(x):
    bsz, t, f = x.shape
    out = _empty((bsz, f, t), x)
    lib.call('ds2_transpose_btf_to_bft', x, bsz, t, f, out)
    return out


def conv_fwd(which, inp, weight, bias, t_in):
    bsz = inp.shape[0]
    t1, t2 = conv_out_frames(t_in) if which == 1 else (None, t_in - 10)
    out = _empty((bsz, 32, 61, t1), inp) if which == 1 else _empty((bsz, 32, 21, t2), inp)
    ws = _empty((lib.query('ds2_conv_wt_ws_floats', which),), inp)
    lib.call('ds2_conv_fwd', which, inp, weight, bias, bsz, t_in, out, ws)
    return out


def conv2_dgrad(d_out, weight, t1):
    bsz = d_out.shape[0]
    d_in = _empty((bsz, 32, 61, t1), d_out)
    ws = _empty((lib.query('ds2_conv2_dgrad_ws_floats', bsz, t1),), d_out)
    lib.call('ds2_conv2_dgrad', d_out, weight, bsz, t1, d_in, ws, ws.numel())
    return d_in


def conv_wgrad(which, inp, d_out, t_in, d_weight, d_bias):
    lib.call('ds2_conv_wgrad', which, inp, d_out, inp.shape[0], t_in, d_weight, d_bias)


# ----------------------------------------------------------------------------- batch norm
def _bn_ws(c, like):
    return _bytes_ws(lib.query('ds2_bn_ws_bytes', c), like)


def bn2d_stats(x, running_mean, running_var, training):
    bsz, c = x.shape[0], x.shape[1]
    inner = x.numel() // (bsz * c)
    mi = _empty((2 * c,), x)
    lib.call('ds2_bn2d_stats', x, bsz, c, inner, BN_EPS, BN_MOMENTUM, int(not training), running_mean, running_var, mi,
             _bn_ws(c, x))
    return mi


def bn2d_apply_htanh(x, mi, gamma, beta, layout_tbf):
    bsz, c, d, t = x.shape
    y = _empty((t, bsz, c * d), x) if layout_tbf else torch.empty_like(x)
    lib.call('ds2_bn2d_apply_htanh', x, mi, gamma, beta, bsz, c, d, t, int(layout_tbf), y)
    return y


def bn2d_htanh_bwd(x, dy, mi, gamma, beta, dgamma, dbeta):
    bsz, c, d, t = x.shape
    dx = torch.empty_like(x)
    lib.call('ds2_bn2d_htanh_bwd', x, dy, mi, gamma, beta, bsz, c, d, t, dx, dgamma, dbeta, _bn_ws(c, x))
    return dx


def bn1d_stats(xa, xb, rows, feat, running_mean, running_var, training):
    mi = _empty((2 * feat,), xa)
    lib.call('ds2_bn1d_stats', xa, xb, rows, feat, BN_EPS, BN_MOMENTUM, int(not training), running_mean, running_var,
             mi, _bn_ws(feat, xa))
    return mi


def bn1d_apply(xa, xb, mi, gamma, beta, rows, feat):
    y = _empty((rows, feat), xa)
    lib.call('ds2_bn1d_apply', xa, xb, mi, gamma, beta, rows, feat, y)
    return y


def bn1d_bwd(xa, xb, dy, mi, gamma, rows, feat, dgamma, dbeta):
    dx = _empty((rows, feat), xa)
    lib.call('ds2_bn1d_bwd', xa, xb, dy, mi, gamma, rows, feat, dx, dgamma, dbeta, _bn_ws(feat, xa))
    return dx


def _host_ints(vals):
    import ctypes
    return ctypes.cast((ctypes.c_int * len(vals))(*[int(v) for v in vals]), ctypes.c_void_p)


def _host_ptrs(tensors):
    """A host array of device pointers (``None`` entries pass NULL)."""
    import ctypes
    ptrs = []
    for t in tensors:
        if t is not None:
            assert t.is_cuda and t.is_contiguous()
        ptrs.append(None if t is None else t.data_ptr())
    return ctypes.cast((ctypes.c_void_p * len(ptrs))(*ptrs), ctypes.c_void_p)


def bn1d_seg_stats(xa, xb, t, bsz, feat, bounds, running_means, running_vars, training):
    """Per-task BatchNorm statistics over the strided rows of (T,B,F) x = xa + xb: task g owns the batch columns
    [bounds[g], bounds[g+1]).  Returns mean_invstd (G, 2F) (ds2_bn1d_seg_stats)."""
    g = len(bounds) - 1
    mi = _empty((g, 2 * feat), xa)
    lib.call('ds2_bn1d_seg_stats', xa, xb, t, bsz, feat, g, _host_ints(bounds), BN_EPS, BN_MOMENTUM, int(not training),
             _host_ptrs(running_means), _host_ptrs(running_vars), mi, _bytes_ws(g * lib.query('ds2_bn_ws_bytes', feat), xa))
    return mi


def bn1d_seg_apply(xa, xb, mi, t, bsz, feat, bounds, gammas, betas):
    """Normalised rows PACKED task after task: rows [t*bounds[g], t*bounds[g+1]) of the (T*B, F) result are task g's
    contiguous (T, B_g, F) block (ds2_bn1d_seg_apply)."""
    y = _empty((t * bsz, feat), xa)
    lib.call('ds2_bn1d_seg_apply', xa, xb, mi, t, bsz, feat, len(bounds) - 1, _host_ints(bounds), _host_ptrs(gammas),
             _host_ptrs(betas), y)
    return y


def bn1d_seg_bwd(xa, xb, dxf, mi, t, bsz, feat, bounds, gammas, dgammas, dbetas):
    """Packed per-task d(xf) -> interleaved (T*B, F) d(x); each task's dgamma / dbeta overwritten (ds2_bn1d_seg_bwd)."""
    g = len(bounds) - 1
    dy = _empty((t * bsz, feat), xa)
    lib.call('ds2_bn1d_seg_bwd', xa, xb, dxf, mi, t, bsz, feat, g, _host_ints(bounds), _host_ptrs(gammas), dy,
             _host_ptrs(dgammas), _host_ptrs(dbetas), _bytes_ws(g * lib.query('ds2_bn_ws_bytes', feat), xa))
    return dy


# ----------------------------------------------------------------------------- GRU recurrence
GRU_MODE = os.environ.get('DS2_GRU_MODE', 'auto')     # 'auto' | 'persistent' | 'step'
_sync_ws = {}
fallback_count = 0                                    # persistent -> per-step fall-backs in this process (bench.py reports it)
_persistent_off = {}                                  # device key -> reason: that device runs the per-step kernels from now on


def _dev_key(dev):
    return (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())


def _gru_sync_ws(dev, bsz, hid):
    """Per-device hand-off workspace of the persistent recurrence (caller-owned, grown on demand, reused).  It is
    zeroed HERE, once: a launch that completes leaves its counters zero for the next one (include/ds2hip.h)."""
    key = _dev_key(dev)
    n = (lib.query('ds2_gru_sync_ws_bytes', bsz, hid) + 3) // 4
    if key not in _sync_ws or _sync_ws[key].numel() < n:
        old = _sync_ws.get(key)
        if old is not None:
            # a larger (B, H) needs a larger workspace: the old one's STICKY timeout flag must not be dropped unread (a
            # launch that timed out earlier in this step, or before a deferred check, left invalid results behind)
            word = lib.query('ds2_gru_sync_error_offset') // 4
            if int(old[word].item()) != 0:
                raise_async_error()
            _err_ptr_tables.clear()                   # cached pointer tables name the old workspace's flag
        _sync_ws[key] = torch.zeros(n, dtype=torch.int32, device=dev)
    return _sync_ws[key]


def _use_persistent(dev, bsz, hid):
    if GRU_MODE == 'step':
        return False
    if _dev_key(dev) in _persistent_off:
        if GRU_MODE == 'persistent':
            raise RuntimeError('persistent GRU kernels are disabled on %s: %s' % (dev, _persistent_off[_dev_key(dev)]))
        return False
    ok = bool(lib.query('ds2_gru_persistent_supported', bsz, hid))
    if GRU_MODE == 'persistent' and not ok:
        raise RuntimeError('persistent GRU kernel does not support B=%d H=%d on this device' % (bsz, hid))
    return ok


def _disable_persistent(dev, reason):
    """Same process, later launches: this device uses the launch-per-step kernels from now on (3x slower at B = 10).
    ``DS2_GRU_STRICT=1`` (set by bench.py: a benchmark must never report the fall-back's rate as the product's) makes
    the fall-back an error instead."""
    import logging
    global fallback_count
    fallback_count += 1
    if os.environ.get('DS2_GRU_STRICT', '0') == '1':
        raise RuntimeError('ds2hip: the persistent GRU kernels would fall back to the launch-per-step kernels on %s (%s) '
                           'and DS2_GRU_STRICT=1 forbids it' % (dev, reason))
    _persistent_off[_dev_key(dev)] = reason
    logging.getLogger('aes-lac-2018').warning('ds2hip: persistent GRU kernels disabled on %s (%s); using the '
                                              'launch-per-step kernels', dev, reason)


def async_error_words():
    """Device views of the STICKY timeout flags of the persistent recurrence (one int32 per device workspace)."""
    word = lib.query('ds2_gru_sync_error_offset') // 4
    return [ws[word:word + 1] for ws in _sync_ws.values()]


def raise_async_error():
    """A bounded spin timed out somewhere since the last check: results of that step are invalid.  Reset the
    workspaces (counters, flag), switch the affected devices to the per-step kernels for later launches, raise."""
    for key, ws in _sync_ws.items():
        word = lib.query('ds2_gru_sync_error_offset') // 4
        bad = int(ws[word].item()) != 0
        ws.zero_()
        if bad:
            _disable_persistent(ws.device, 'a hand-off spin timed out (were all workgroups resident?)')
    raise RuntimeError('ds2hip: persistent GRU kernel timed out waiting for a workgroup hand-off; the results of this '
                       'step are invalid')


def check_async_errors():
    """Raise if a persistent kernel's bounded spin timed out since the last check (call after a device synchronize)."""
    for w in async_error_words():
        if int(w.item()) != 0:
            raise_async_error()


_dh_supported = {}


def gru_bwd_dh_wanted(dev, bsz, hid):
    """Will ``gru_bidir_bwd`` run the d(h)-hand-off backward recurrence for this shape (so that the training forward pass
    should ask for the coefficient planes)?  Default: where the library has the form AND the forward kernel writes the planes
    itself (B = 9 .. 12 at H = 800: measured stand-alone at B = 10, us per step, d(gh) -> d(h) hand-off: 2.55 -> 2.36 on 240
    workgroups, 2.81 -> 2.67 on 174); for B = 5 .. 8 the planes would cost an extra elementwise pass that eats the
    0.03 us per step the form gains there.  ``DS2_GRU_BWD_DH`` = 0 / 1 forces it off / on wherever the form exists."""
    if not _use_persistent(dev, bsz, hid):
        return False
    key = (bsz, hid)
    if key not in _dh_supported:                      # (a shape's answer never changes: one library query per shape)
        _dh_supported[key] = bool(lib.query('ds2_gru_bwd_dh_supported', bsz, hid))
    if not _dh_supported[key]:
        return False
    e = os.environ.get('DS2_GRU_BWD_DH')
    if e in ('0', '1'):
        return e == '1'
    return bsz >= 9


def gru_bidir_fwd(gates, w_hh, t, bsz, hid, want_coef=False):
    """gates (T,B,2,3H) holds gi on entry, (r,z,n) on exit.  Returns (ghn (T,B,2,H), hout (2,T,B,H)), and with ``want_coef``
    also the (T,B,2,3H) coefficient planes of the d(h)-hand-off backward recurrence (None where that form will not run)."""
    ghn = _empty((t, bsz, 2, hid), gates)
    hout = _empty((2, t, bsz, hid), gates)
    coef = _empty((t, bsz, 2, 3 * hid), gates) if want_coef and gru_bwd_dh_wanted(gates.device, bsz, hid) else None
    if _use_persistent(gates.device, bsz, hid):
        try:
            lib.call('ds2_gru_bidir_fwd_persistent_ex', gates, ghn, hout, w_hh, coef, _gru_sync_ws(gates.device, bsz, hid), t,
                     bsz, hid)
            return (ghn, hout, coef) if want_coef else (ghn, hout)
        except lib.Ds2Error as e:               # nothing was launched: the chosen kernel's grid is not co-resident here
            if e.code != lib.ERR_UNSUPPORTED or GRU_MODE == 'persistent':
                raise
            _disable_persistent(gates.device, str(e))
    lib.call('ds2_gru_bidir_fwd', gates, ghn, hout, w_hh, t, bsz, hid)
    return (ghn, hout, None) if want_coef else (ghn, hout)     # (the launch-per-step backward kernels take no coefficients)


def gru_bwd_coef(gates, ghn, hout, t, bsz, hid):
    """(T,B,2,3H) coefficient planes of the d(h) hand-off backward recurrence from the forward pass's saved tensors."""
    coef = _empty((t, bsz, 2, 3 * hid), gates)
    lib.call('ds2_gru_bwd_coef', gates, ghn, hout, coef, t, bsz, hid)
    return coef


def gru_bidir_bwd(gates, ghn, hout, d_out, w_hh_t, t, bsz, hid, spare_cus=-1, coef=None):
    """``spare_cus``: compute units to leave free beside the launch for work queued on other streams (-1: the library's
    default; see ds2_gru_bidir_bwd_persistent_ex in include/ds2hip.h).  ``coef``: the forward pass's coefficient planes
    (``gru_bidir_fwd(.., want_coef=True)``) -> the d(h)-hand-off form; None -> the d(gh)-hand-off form."""
    if _use_persistent(gates.device, bsz, hid):
        try:
            if coef is not None:
                lib.call('ds2_gru_bidir_bwd_persistent_dh', gates, ghn, hout, d_out, w_hh_t, coef,
                         _gru_sync_ws(gates.device, bsz, hid), t, bsz, hid, int(spare_cus))
                return
            lib.call('ds2_gru_bidir_bwd_persistent_ex', gates, ghn, hout, d_out, w_hh_t,
                     _gru_sync_ws(gates.device, bsz, hid), t, bsz, hid, int(spare_cus))
            return
        except lib.Ds2Error as e:
            if e.code != lib.ERR_UNSUPPORTED or GRU_MODE == 'persistent':
                raise
            _disable_persistent(gates.device, str(e))
    ws = torch.zeros((2 * 2 * bsz * hid,), dtype=torch.float32, device=gates.device)
    lib.call('ds2_gru_bidir_bwd', gates, ghn, hout, d_out, w_hh_t, ws, t, bsz, hid)


# ----------------------------------------------------------------------------- head / decode
def softmax_rows(x, rows, a):
    y = torch.empty_like(x)
    lib.call('ds2_softmax_rows', x, rows, a, y)
    return y


def argmax_rows(x, rows, a):
    idx = _empty((rows,), x, torch.int32)
    lib.call('ds2_argmax_rows', x, rows, a, idx)
    return idx


def greedy_collapse(best, sizes, blank=0):
    bsz, t = best.shape
    ids = torch.zeros((bsz, t), dtype=torch.int32, device=best.device)
    offs = torch.zeros((bsz, t), dtype=torch.int32, device=best.device)
    lens = torch.zeros((bsz,), dtype=torch.int32, device=best.device)
    lib.call('ds2_greedy_collapse', best, sizes, bsz, t, blank, ids, offs, lens)
    return ids, offs, lens


def _require_device(name, dtype, **tensors):
    for key, x in tensors.items():
        if not x.is_cuda:
            raise RuntimeError('ds2hip entry points take device tensors; got a CPU tensor')
        if x.dtype != dtype:
            raise RuntimeError('%s: %s must be %s, got %s' % (name, key, dtype, x.dtype))


def _lm_args(lm, device, space_id, alpha, beta):
    """The LM arguments of a beam search entry, ngram_table .. oov_logp in the ABI's order, and the device tables they
    point into: keep those referenced until the call has been made.  ``alpha is None`` gives the ``_rows`` form, which has
    no scalar weights."""
    if lm is None:
        tabs, args = {}, (None, 0, None, 0, 1, 0, -1, -1, -1, -1, 0.0, 0.0, 0.0)
    else:
        tabs = lm.to(device)
        word = tabs.get('word')
        weights = (0.0, 0.0) if alpha is None else (float(alpha), float(beta))
        args = (tabs['ngram'], tabs['ngram'].shape[0], word, 0 if word is None else word.shape[0], lm.order,
                1 if lm.unit == 'char' else 2, lm.bos_id, lm.eos_id, lm.hist_unk_id, space_id) + weights + (
                    float(lm.oov_logp),)
    return tabs, (args[:10] + args[12:] if alpha is None else args)


def _bias_args(name, bias_trans, bias_final, a):
    """The context-graph arguments bias_trans, bias_final, bias_states of ``_bias`` and ``_nbest``, the shape checked."""
    _require_device(name, torch.int32, bias_trans=bias_trans, bias_final=bias_final)
    states = int(bias_final.numel())
    if bias_trans.dim() != 2 or tuple(bias_trans.shape) != (states, a):
        raise RuntimeError('%s: bias_trans must be (states, A) = (%d, %d), got %s'
                           % (name, states, a, tuple(bias_trans.shape)))
    return bias_trans, bias_final, states


def _beam_search(entry, rows, ws_rows, probs, head, beam_width, blank, log_input, lm, space_id, alpha, beta, mid=(),
                 tail=()):
    """The call all four beam search wrappers make: the workspace for ``ws_rows`` rows, the five outputs with ``rows``
    (a tuple) in front of their own shape, and ``entry(probs, *head, T, A, blank, beam_width, log_input, <LM>, *mid,
    <workspace>, <outputs>, *tail)``.  Returns the five outputs."""
    _, t, a = probs.shape
    ws = _bytes_ws(lib.query('ds2_ctc_beam_ws_bytes', ws_rows, t, beam_width), probs)
    labels = torch.empty(rows + (t,), dtype=torch.int32, device=probs.device)
    offsets = torch.empty(rows + (t,), dtype=torch.int32, device=probs.device)
    lens = torch.empty(rows, dtype=torch.int32, device=probs.device)
    score = _empty(rows, probs)
    ctc = _empty(rows, probs)
    tabs, lm_args = _lm_args(lm, probs.device, space_id, alpha, beta)       # tabs: referenced until the call is made
    lib.call(entry, probs, *head, t, a, int(blank), int(beam_width), int(bool(log_input)), *lm_args, *mid, ws,
             ws.numel() * ws.element_size(), labels, offsets, lens, score, ctc, *tail)
    return labels, offsets, lens, score, ctc


def ctc_beam_search(probs, sizes, beam_width, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    """Batched CTC prefix beam search on the current stream (``ds2_ctc_beam_search_batch``).  probs (B,T,A) fp32 on the
    device, sizes (B,) int32 on the device; ``lm`` an ``codes.lm.NGramLM`` or None.  Returns the device tensors
    labels (B,T), offsets (B,T), lens (B,) int32 and score, ctc_logp (B,) fp32."""
    bsz = probs.shape[0]
    return _beam_search('ds2_ctc_beam_search_batch', (bsz,), bsz, probs, (sizes, bsz), beam_width, blank, log_input, lm,
                        space_id, alpha, beta)


def ctc_beam_search_rows(probs, sizes, utt, alpha, beta, beam_width, blank=0, log_input=False, lm=None, space_id=-1):
    """``ctc_beam_search`` with R output rows decoupled from the B utterances (``ds2_ctc_beam_search_rows``): row r decodes
    utterance utt[r] with the LM weights alpha[r], beta[r], all rows in one launch on the current stream.  probs (B,T,A)
    fp32 and sizes (B,) int32 on the device; utt (R,) int32, alpha, beta (R,) fp32 on the device (the weights are ignored
    without an ``lm``).  Returns the device tensors labels (R,T), offsets (R,T), lens (R,) int32 and score, ctc_logp (R,)
    fp32, row r bit-identical to ``ctc_beam_search`` of that utterance with those weights; a utt[r] outside [0, B) gives
    the empty labelling at -inf.  Nothing waits on the stream."""
    _require_device('ctc_beam_search_rows', torch.float32, probs=probs, alpha=alpha, beta=beta)
    _require_device('ctc_beam_search_rows', torch.int32, sizes=sizes, utt=utt)
    bsz = probs.shape[0]
    rows = int(utt.numel())
    if int(sizes.numel()) != bsz or int(alpha.numel()) != rows or int(beta.numel()) != rows:
        raise RuntimeError('ctc_beam_search_rows: sizes must have B entries; alpha and beta one per entry of utt')
    return _beam_search('ds2_ctc_beam_search_rows', (rows,), rows, probs, (sizes, utt, alpha, beta, bsz, rows), beam_width,
                        blank, log_input, lm, space_id, None, None)


def ctc_beam_search_bias(probs, sizes, beam_width, bias_trans, bias_final, bias_weight, blank=0, log_input=False, lm=None,
                         alpha=0.0, beta=0.0, space_id=-1):
    """``ctc_beam_search`` with phrase boosting (``ds2_ctc_beam_search_bias``; include/ds2hip.h "phrase boosting"):
    bias_trans (S,A) and bias_final (S,) int32 on the device are a context graph's tables (``codes.bias.ContextGraph``),
    bias_weight the weight per matched label in nats.  Returns ``ctc_beam_search``'s five device tensors and bias (B,)
    int32: the labels of each returned labelling that the boosted phrases cover.  Nothing waits on the stream."""
    _require_device('ctc_beam_search_bias', torch.float32, probs=probs)
    _require_device('ctc_beam_search_bias', torch.int32, sizes=sizes)
    bsz, _, a = probs.shape
    graph = _bias_args('ctc_beam_search_bias', bias_trans, bias_final, a) + (float(bias_weight),)
    bias = torch.empty((bsz,), dtype=torch.int32, device=probs.device)
    return _beam_search('ds2_ctc_beam_search_bias', (bsz,), bsz, probs, (sizes, bsz), beam_width, blank, log_input, lm,
                        space_id, alpha, beta, mid=graph, tail=(bias,)) + (bias,)


def ctc_beam_search_nbest(probs, sizes, beam_width, nbest, blank=0, log_input=False, lm=None, alpha=0.0, beta=0.0,
                          space_id=-1, bias_trans=None, bias_final=None, bias_weight=0.0):
    """``ctc_beam_search`` -- with ``bias_trans`` / ``bias_final`` / ``bias_weight``, ``ctc_beam_search_bias`` -- returning
    the ``nbest`` best entries of each utterance's final beam (``ds2_ctc_beam_search_nbest``; include/ds2hip.h has the
    ranking).  1 <= nbest <= beam_width.  Returns the device tensors labels (B,N,T), offsets (B,N,T), lens (B,N) int32,
    score, ctc_logp (B,N) fp32, bias (B,N) int32 (None without a graph) and count (B,) int32: rows [0, count[b]) of
    utterance b are its alternatives, best first, row 0 bit-identical to the 1-best search; the rows past the count are
    empty at -inf.  Nothing waits on the stream."""
    _require_device('ctc_beam_search_nbest', torch.float32, probs=probs)
    _require_device('ctc_beam_search_nbest', torch.int32, sizes=sizes)
    bsz, _, a = probs.shape
    n = int(nbest)
    if not 1 <= n <= int(beam_width):
        raise ValueError('ctc_beam_search_nbest: nbest %d is outside 1..beam_width = %d' % (n, int(beam_width)))
    bias, graph = None, (None, None, 0, 0.0)
    if bias_trans is not None:
        if bias_final is None:
            raise RuntimeError('ctc_beam_search_nbest: bias_trans needs bias_final')
        graph = _bias_args('ctc_beam_search_nbest', bias_trans, bias_final, a) + (float(bias_weight),)
        bias = torch.empty((bsz, n), dtype=torch.int32, device=probs.device)
    count = torch.empty((bsz,), dtype=torch.int32, device=probs.device)
    return _beam_search('ds2_ctc_beam_search_nbest', (bsz, n), bsz, probs, (sizes, bsz), beam_width, blank, log_input, lm,
                        space_id, alpha, beta, mid=graph + (n,), tail=(bias, count)) + (bias, count)


EDIT_MAX_ITEMS = lib.EDIT_MAX_ITEMS     # DS2_EDIT_MAX_ITEMS of include/ds2hip.h: labels per side ds2_edit_stats takes
EDIT_THREADS = 256                      # DS2_EDIT_THREADS: threads of its one workgroup per (row, level)
EDIT_CHUNK = 8                          # DS2_EDIT_CHUNK: consecutive labels a thread owns in the item pass
EDIT_FIELDS = ('char_dist', 'char_sub', 'char_del', 'char_ins', 'ref_chars',
               'word_dist', 'word_sub', 'word_del', 'word_ins', 'ref_words')


def edit_stats(hyp, hyp_len, ref, ref_offsets, ref_lens, max_ref_len, space_id=-1, ref_index=None, group=None,
               totals=None, ws=None):
    """Word and character error counts of R label rows against their references in one launch on the current stream
    (``ds2_edit_stats``; include/ds2hip.h has the definition).  hyp (R,stride) and hyp_len (R,) int32 on the device, as the
    beam search and ``greedy_collapse`` return them; flat ref, ref_offsets (N,), ref_lens (N,) int32 on the device;
    ``ref_index`` (R,) int32 picks each row's reference (None: row r uses reference r).  ``group`` (R,) int32 with
    ``totals`` (G,10) int64: the valid rows' ten values are ADDED to totals[group[r]].  Returns stats (R,10) int32 in the
    order of ``EDIT_FIELDS``; an invalid row is all -1.  Nothing waits on the stream."""
    ints = dict(hyp=hyp, hyp_len=hyp_len, ref=ref, ref_offsets=ref_offsets, ref_lens=ref_lens)
    if ref_index is not None:
        ints['ref_index'] = ref_index
    if group is not None:
        ints['group'] = group
    _require_device('edit_stats', torch.int32, **ints)
    if hyp.dim() != 2:
        raise RuntimeError('edit_stats: hyp must be (R, stride)')
    rows, stride = hyp.shape
    n_ref = int(ref_lens.numel())
    if int(hyp_len.numel()) != rows or int(ref_offsets.numel()) != n_ref:
        raise RuntimeError('edit_stats: hyp_len must have R entries; ref_offsets one per entry of ref_lens')
    for x in (ref_index, group):
        if x is not None and int(x.numel()) != rows:
            raise RuntimeError('edit_stats: ref_index and group must have R entries')
    n_groups = 0
    if group is not None:
        if totals is None:
            raise RuntimeError('edit_stats: group needs totals (G,10) int64')
        _require_device('edit_stats', torch.int64, totals=totals)
        if totals.dim() != 2 or totals.shape[1] != 10 or not totals.is_contiguous():
            raise RuntimeError('edit_stats: totals must be a contiguous (G,10) tensor')
        n_groups = int(totals.shape[0])
    if ws is None:
        ws_bytes = lib.query('ds2_edit_stats_ws_bytes', rows, stride, int(max_ref_len))
        ws = torch.empty((max(int(ws_bytes), 16),), dtype=torch.uint8, device=hyp.device)
    stats = torch.empty((rows, 10), dtype=torch.int32, device=hyp.device)
    lib.call('ds2_edit_stats', hyp, hyp_len, rows, stride, ref, ref_offsets, ref_lens, n_ref, int(max_ref_len), ref_index,
             group, n_groups, int(space_id), ws, ws.numel() * ws.element_size(), stats, totals if group is not None else None)
    return stats


def _align_call(entry, ws_arg, probs, head, max_label_len, tail, score_dtype, lo_name=None, with_gap=False):
    """The call all three alignment wrappers make: ``entry(probs, *head, B, T, A, max_label_len, *tail, <workspace>, states,
    starts, ends, [gap,] score)`` with the workspace of ``<entry>_ws_bytes(B, T, ws_arg)``.  ``head``: the device tensors
    behind probs; ``lo_name``: the wrapper's name where head ends in ``lo``, whose shape is checked under it; ``with_gap``:
    the entry has the gap output.  Returns states, starts, ends, gap or None, score."""
    for x in (probs,) + head:
        if not x.is_cuda:
            raise RuntimeError('ds2hip entry points take device tensors; got a CPU tensor')
    bsz, t, a = probs.shape
    if lo_name and (head[-1].dtype != torch.int32 or tuple(head[-1].shape) != (bsz, t)):
        raise RuntimeError('%s: lo must be int32 of shape (B,T) = (%d,%d)' % (lo_name, bsz, t))
    max_label_len = int(max_label_len)
    ws = _bytes_ws(max(lib.query(entry + '_ws_bytes', bsz, t, int(ws_arg)), 16), probs)
    states = torch.empty((bsz, t), dtype=torch.int32, device=probs.device)
    starts = torch.empty((bsz, max(max_label_len, 0)), dtype=torch.int32, device=probs.device)
    ends = torch.empty_like(starts)
    gap = torch.empty((bsz, t), dtype=torch.uint8, device=probs.device) if with_gap else None
    score = torch.empty((bsz,), dtype=score_dtype, device=probs.device)
    lib.call(entry, probs, *head, bsz, t, a, max_label_len, *tail, ws, ws.numel() * ws.element_size(), states, starts, ends,
             *((gap,) if with_gap else ()), score)
    return states, starts, ends, gap, score


def ctc_align(probs, sizes, labels, label_offsets, label_lens, max_label_len, blank=0, log_input=False):
    """CTC forced alignment of a batch in one launch on the current stream (``ds2_ctc_align``).  probs (B,T,A) fp32 on the
    device; sizes (B,), flat labels, label_offsets (B,), label_lens (B,) int32 on the device.  Returns the device tensors
    states (B,T), starts, ends (B,max_label_len) int32 and score (B,) fp32; an utterance without an alignment has
    score -inf and -1 everywhere."""
    states, starts, ends, _, score = _align_call('ds2_ctc_align', max_label_len, probs,
                                                 (sizes, labels, label_offsets, label_lens), max_label_len,
                                                 (int(blank), int(bool(log_input))), torch.float32)
    return states, starts, ends, score


def ctc_align_banded(probs, sizes, labels, label_offsets, label_lens, max_label_len, lo, band, blank=0, log_input=False):
    """``ctc_align`` restricted to a moving band of ``band`` states per frame (``ds2_ctc_align_banded``): work and workspace
    are T x band, so transcripts of any length align.  ``lo`` (B,T) int32 on the device, >= 0 and non-decreasing over an
    utterance's frames: frame t admits the states lo[b,t] <= s < lo[b,t] + band.  ``band`` a power of two in
    lib.ALIGN_BAND_MIN .. lib.ALIGN_BAND_MAX.  Returns states, starts, ends as ``ctc_align`` and score (B,) FLOAT64; an
    utterance without an alignment inside its band (or with a bad band) has score -inf and -1 everywhere."""
    states, starts, ends, _, score = _align_call('ds2_ctc_align_banded', band, probs,
                                                 (sizes, labels, label_offsets, label_lens, lo), max_label_len,
                                                 (int(band), int(blank), int(bool(log_input))), torch.float64,
                                                 lo_name='ctc_align_banded')
    return states, starts, ends, score


def ctc_align_banded_gap(probs, sizes, labels, label_offsets, label_lens, max_label_len, lo, band, space, gap_penalty, blank=0,
                         log_input=False):
    """``ctc_align_banded`` in which the blank states between words (the two end blanks and the blanks beside a ``space``
    label; ``space`` = -1: the end blanks only) may absorb a frame at ``gap_penalty`` (fp32, >= 0, inf allowed) below the
    frame's best symbol (``ds2_ctc_align_banded_gap``; include/ds2hip.h has the definition).  Arguments as
    ``ctc_align_banded``.  Returns the device tensors states, starts, ends, gap (B,T) uint8 -- 1 where the path's frame was
    absorbed -- and score (B,) FLOAT64.  Nothing waits on the stream."""
    return _align_call('ds2_ctc_align_banded_gap', band, probs, (sizes, labels, label_offsets, label_lens, lo), max_label_len,
                       (int(band), int(blank), int(space), float(gap_penalty), int(bool(log_input))), torch.float64,
                       lo_name='ctc_align_banded_gap', with_gap=True)


def keyword_search(logp, sizes, labels, label_offsets, label_lens, min_score, max_hits=4, blank=0, ws=None):
    """Where each of K keywords was said in each utterance, in one call on the current stream (``ds2_ctc_keyword_search``;
    include/ds2hip.h has the definition).  logp (B,T,A) fp32 LOG-probabilities on the device; sizes (B,), flat labels,
    label_offsets (K,), label_lens (K,) int32 and min_score (K,) float64 on the device.  ``ws``: a uint8 device tensor of at
    least ``ds2_ctc_keyword_search_ws_bytes(B, T)`` bytes, or None to allocate one.  Returns the device tensors hits
    (B,K,max_hits,2) int32 (start, end; -1 past the count), hit_score (B,K,max_hits) float64 (-inf past the count) and n_hits
    (B,K) int32, the true count.  Nothing waits on the stream."""
    for x in (logp, sizes, labels, label_offsets, label_lens, min_score):
        if not x.is_cuda:
            raise RuntimeError('ds2hip entry points take device tensors; got a CPU tensor')
    if logp.dtype != torch.float32 or min_score.dtype != torch.float64:
        raise RuntimeError('keyword_search: logp must be float32 and min_score float64')
    for x in (sizes, labels, label_offsets, label_lens):
        if x.dtype != torch.int32:
            raise RuntimeError('keyword_search: sizes, labels, label_offsets and label_lens must be int32')
    bsz, t, a = logp.shape
    k, max_hits = int(label_lens.numel()), int(max_hits)
    if int(sizes.numel()) != bsz or int(label_offsets.numel()) != k or int(min_score.numel()) != k:
        raise RuntimeError('keyword_search: sizes must have B entries; label_offsets, label_lens and min_score K entries')
    if ws is None:
        ws_bytes = lib.query('ds2_ctc_keyword_search_ws_bytes', bsz, t)
        ws = torch.empty((max(int(ws_bytes), 16),), dtype=torch.uint8, device=logp.device)
    shape = (bsz, max(k, 0), max(max_hits, 0))
    hits = torch.empty(shape + (2,), dtype=torch.int32, device=logp.device)
    hit_score = torch.empty(shape, dtype=torch.float64, device=logp.device)
    n_hits = torch.empty(shape[:2], dtype=torch.int32, device=logp.device)
    lib.call('ds2_ctc_keyword_search', logp, sizes, labels, label_offsets, label_lens, min_score, bsz, t, a, k, int(blank),
             max_hits, ws, ws.numel() * ws.element_size(), hits, hit_score, n_hits)
    return hits, hit_score, n_hits


UNIT_MAX_LABELS = lib.UNIT_MAX_LABELS   # DS2_UNIT_MAX_LABELS of include/ds2hip.h: labels of a unit ds2_ctc_unit_posterior scores


def ctc_unit_posterior(probs, sizes, labels, offsets, lens, utt=None, space_id=-1, blank=0, max_units=None, ws=None):
    """The span posterior of every word (``space_id >= 0``) or character (``space_id = -1``) of R decoded label rows, in one
    call on the current stream (``ds2_ctc_unit_posterior``; include/ds2hip.h, "unit posterior", has the definition).  probs
    (B,T,A) fp32 PROBABILITIES and sizes (B,) int32 on the device; labels, offsets (R,stride) and lens (R,) int32 on the device
    as the beam search and ``greedy_collapse`` return them (an N-best result viewed as (B*N, T)); ``utt`` (R,) int32 is each
    row's utterance (None: row r uses utterance r).  ``max_units`` defaults to stride (characters) or (stride + 1) // 2
    (words), which no row can exceed.  ``ws``: a uint8 device tensor of at least ``ds2_ctc_unit_posterior_ws_bytes(R, stride,
    max_units)`` bytes, or None to allocate one.  Returns the device tensors unit_first, unit_len (R,max_units) int32 (-1 past
    the count), unit_logp (R,max_units) float64 (NaN past the count and for a unit of more than ``UNIT_MAX_LABELS`` labels),
    n_units (R,) int32 (the true count; -1 for an invalid row) and dropped (R,) int32.  Nothing waits on the stream."""
    _require_device('ctc_unit_posterior', torch.float32, probs=probs)
    ints = dict(sizes=sizes, labels=labels, offsets=offsets, lens=lens)
    if utt is not None:
        ints['utt'] = utt
    _require_device('ctc_unit_posterior', torch.int32, **ints)
    if probs.dim() != 3 or labels.dim() != 2 or tuple(offsets.shape) != tuple(labels.shape):
        raise RuntimeError('ctc_unit_posterior: probs must be (B,T,A); labels and offsets (R,stride)')
    bsz, t, a = probs.shape
    rows, stride = labels.shape
    if int(sizes.numel()) != bsz or int(lens.numel()) != rows or (utt is not None and int(utt.numel()) != rows):
        raise RuntimeError('ctc_unit_posterior: sizes must have B entries; lens and utt R entries')
    if utt is None and rows > bsz:
        raise RuntimeError('ctc_unit_posterior: %d rows of %d utterances need utt' % (rows, bsz))
    space_id = int(space_id)
    if max_units is None:
        max_units = stride if space_id < 0 else (stride + 1) // 2
    max_units = int(max_units)
    if ws is None:
        ws_bytes = lib.query('ds2_ctc_unit_posterior_ws_bytes', rows, stride, max_units)
        ws = torch.empty((max(int(ws_bytes), 16),), dtype=torch.uint8, device=probs.device)
    shape = (max(rows, 0), max(max_units, 0))
    unit_first = torch.empty(shape, dtype=torch.int32, device=probs.device)
    unit_len = torch.empty(shape, dtype=torch.int32, device=probs.device)
    unit_logp = torch.empty(shape, dtype=torch.float64, device=probs.device)
    n_units = torch.empty(shape[:1], dtype=torch.int32, device=probs.device)
    dropped = torch.empty(shape[:1], dtype=torch.int32, device=probs.device)
    lib.call('ds2_ctc_unit_posterior', probs, sizes, bsz, t, a, labels, offsets, lens, utt, rows, stride, space_id, int(blank),
             max_units, ws, ws.numel() * ws.element_size(), unit_first, unit_len, unit_logp, n_units, dropped)
    return unit_first, unit_len, unit_logp, n_units, dropped


# ----------------------------------------------------------------------------- CTC
def ctc_loss_grad(acts, labels, label_offsets, label_lens, act_lens, max_label_len, grad_scale=1.0,
                  zero_batch_if_inf=False):
    """acts (T,B,A) -> costs (B,), grad (T,B,A); int32 device tensors for the rest.  ``zero_batch_if_inf``: the training
    step's rule -- an infinite batch loss zeroes the whole batch's gradient (codes/engine.py:24-30)."""
    t, bsz, a = acts.shape
    costs = _empty((bsz,), acts)
    grad = torch.empty_like(acts)
    ws = _bytes_ws(lib.query('ds2_ctc_ws_bytes', t, bsz, a, max_label_len), acts)
    lib.call('ds2_ctc_loss_grad', acts, labels, label_offsets, label_lens, act_lens, t, bsz, a, max_label_len,
             float(grad_scale), int(zero_batch_if_inf), costs, grad, ws)
    return costs, grad


MWER_MAX_NBEST = lib.MWER_MAX_NBEST     # DS2_MWER_MAX_NBEST of include/ds2hip.h


def ctc_mwer_ws_bytes(t, bsz, a, nbest, max_label_len):
    """Bytes of workspace ``ctc_mwer_grad`` needs (``ds2_ctc_mwer_ws_bytes``; 0 for sizes the entry refuses)."""
    return int(lib.query('ds2_ctc_mwer_ws_bytes', int(t), int(bsz), int(a), int(nbest), int(max_label_len)))


def ctc_mwer_grad(acts, act_lens, hyp, hyp_len, hyp_count, risk, ref, ref_offsets, ref_lens, max_label_len, ctc_weight=0.0,
                  grad_scale=1.0, zero_batch_if_inf=False, ws=None):
    """Minimum-word-error-rate loss terms and gradient of N-best lists in one call on the current stream
    (``ds2_ctc_mwer_grad``; include/ds2hip.h "MWER" has the definition and the rules).  acts (T,B,A) fp32 un-normalised;
    hyp (B,N,stride), hyp_len (B,N), hyp_count (B,) int32 as ``ctc_beam_search_nbest`` returns them; risk (B,N) fp32; flat
    ref, ref_offsets (B,), ref_lens (B,), act_lens (B,) int32; all on the device.  ``ws``: a uint8 device tensor of at least
    ``ctc_mwer_ws_bytes`` bytes, or None to allocate one.  Returns the device tensors (ref_costs (B,), hyp_costs (B,N),
    posterior (B,N), exp_risk (B,), dropped (B,) int32, grad (T,B,A)).  Nothing waits on the stream."""
    _require_device('ctc_mwer_grad', torch.float32, acts=acts, risk=risk)
    _require_device('ctc_mwer_grad', torch.int32, act_lens=act_lens, hyp=hyp, hyp_len=hyp_len, hyp_count=hyp_count, ref=ref,
                    ref_offsets=ref_offsets, ref_lens=ref_lens)
    if acts.dim() != 3 or hyp.dim() != 3:
        raise RuntimeError('ctc_mwer_grad: acts must be (T,B,A) and hyp (B,N,stride)')
    t, bsz, a = acts.shape
    n, stride = int(hyp.shape[1]), int(hyp.shape[2])
    if int(hyp.shape[0]) != bsz or tuple(hyp_len.shape) != (bsz, n) or tuple(risk.shape) != (bsz, n):
        raise RuntimeError('ctc_mwer_grad: hyp (B,N,stride), hyp_len (B,N) and risk (B,N) must agree with B = %d of acts' % bsz)
    for name, x in (('act_lens', act_lens), ('hyp_count', hyp_count), ('ref_offsets', ref_offsets), ('ref_lens', ref_lens)):
        if int(x.numel()) != bsz:
            raise RuntimeError('ctc_mwer_grad: %s must have B = %d entries' % (name, bsz))
    max_label_len = int(max_label_len)
    if ws is None:
        ws = _bytes_ws(max(ctc_mwer_ws_bytes(t, bsz, a, n, max_label_len), 16), acts)
    elif ws.numel() * ws.element_size() < ctc_mwer_ws_bytes(t, bsz, a, n, max_label_len):
        raise RuntimeError('ctc_mwer_grad: ws holds %d bytes, %d are needed'
                           % (ws.numel() * ws.element_size(), ctc_mwer_ws_bytes(t, bsz, a, n, max_label_len)))
    ref_costs = _empty((bsz,), acts)
    hyp_costs = _empty((bsz, n), acts)
    posterior = _empty((bsz, n), acts)
    exp_risk = _empty((bsz,), acts)
    dropped = _empty((bsz,), acts, torch.int32)
    grad = torch.empty_like(acts)
    lib.call('ds2_ctc_mwer_grad', acts, act_lens, t, bsz, a, hyp, hyp_len, hyp_count, n, stride, risk, ref, ref_offsets, ref_lens,
             max_label_len, float(ctc_weight), float(grad_scale), int(bool(zero_batch_if_inf)), ref_costs, hyp_costs, posterior,
             exp_risk, dropped, grad, ws)
    return ref_costs, hyp_costs, posterior, exp_risk, dropped, grad


# ----------------------------------------------------------------------------- optimiser
def sumsq(x, out=None):
    if out is None:
        out = torch.empty((1,), dtype=torch.float64, device=x.device)
    ws = _bytes_ws(lib.query('ds2_sumsq_ws_bytes', x.numel()), x)
    lib.call('ds2_sumsq', x, x.numel(), out, ws)
    return out


_err_ptr_tables = {}


def step_stats(costs, sumsq_t, out=None):
    """One launch gathering what the host reads after a step: [sum of costs, squared grad norm, any timeout flag,
    number of infinite costs] as float64 (4,)."""
    dev = costs.device
    words = async_error_words()
    key = (_dev_key(dev), tuple(w.data_ptr() for w in words))
    table = _err_ptr_tables.get(key)
    if table is None:
        table = _err_ptr_tables[key] = torch.tensor([w.data_ptr() for w in words] or [0], dtype=torch.int64).to(dev)
    if out is None:
        out = torch.empty((4,), dtype=torch.float64, device=dev)
    # ``out`` may be PAGE-LOCKED HOST memory (its address is valid on the device): the kernel then writes the four values
    # straight to the host, which polls them (wait_step_stats) -- no copy, no event (tools/attic/readback_probe.py: 14.5 against
    # 32-34 us from launch to the host having the values)
    lib.call('ds2_step_stats', costs, costs.numel(), sumsq_t, table, len(words), out if out.is_cuda else out.data_ptr())
    return out


STATS_SENTINEL = 0x7FF8DEADBEEF0001          # a NaN payload no arithmetic produces: "not written yet"


def arm_step_stats(slot):
    """Mark a page-locked float64 (4,) slot as not yet written (before the launch that will write it)."""
    slot.view(torch.int64).fill_(STATS_SENTINEL)


def _stats_timeout():
    """Seconds the host waits for a step's statistics before giving up: ``DS2_STATS_TIMEOUT_S`` if set (``0`` / ``inf`` = no
    limit); otherwise no limit inside a process group -- the statistics are queued behind the gradient all-reduce there, a
    slow peer (rank 0 saving a checkpoint, uneven evaluation shards, a cold loader) is not an error, and the group's own
    watchdog bounds the wait -- and 120 s for a single-GPU run."""
    v = os.environ.get('DS2_STATS_TIMEOUT_S')
    if v is not None:
        t = float(v)
        return None if t <= 0 or t == float('inf') else t
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return None
    return 120.0


def wait_step_stats(slot, timeout_s='default', stream=None):
    """Poll a slot armed by ``arm_step_stats`` until the device has written all four values.

    While waiting, the stream the step was queued on is queried from time to time: a device fault raises as the HIP error it
    is (not as a time-out minutes later), and a stream that has DRAINED without the slot being written -- the statistics
    kernel never ran -- raises at once.  ``timeout_s``: None = wait without limit, 'default' = ``_stats_timeout()``."""
    import time
    words = slot.view(torch.int64).numpy()
    t0, next_query, every = None, 0.0, 0.02
    while (words == STATS_SENTINEL).any():
        time.sleep(0)                             # (hands the GIL to a loader / pin-memory thread that wants it)
        now = time.time()
        if t0 is None:
            t0, next_query = now, now + every
            if timeout_s == 'default':
                timeout_s = _stats_timeout()
            continue
        if now < next_query:
            continue
        every = min(every * 2, 1.0)
        next_query = now + every
        st = stream if stream is not None else torch.cuda.current_stream()
        if st.query():                            # (raises the pending HIP error of a faulted device)
            time.sleep(0.001)
            if (words == STATS_SENTINEL).any():
                raise RuntimeError('the stream has run everything queued on it and the step\'s statistics were never '
                                   'written to host memory')
        if timeout_s is not None and now - t0 > timeout_s:
            raise RuntimeError('the step\'s statistics never arrived in host memory (%.0f s; DS2_STATS_TIMEOUT_S)' % timeout_s)
    return slot.tolist()


def clip_sgd_nesterov(p, g, buf, sumsq_t, grad_scale, max_norm, lr, momentum, first_step):
    lib.call('ds2_clip_sgd_nesterov', p, g, buf, p.numel(), sumsq_t, float(grad_scale), float(max_norm), float(lr),
             float(momentum), int(first_step))
