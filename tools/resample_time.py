#!/usr/bin/env python
"""Time the sample-rate conversion of a one-hour recording (ds2_resample), one JSON line.

    python tools/resample_time.py [--reps 20] [--seconds 3600] [--ref-seconds 60]

Input: seeded uniform int16 noise of ``--seconds``, generated on the device -- 44.1 kHz stereo (the headline), 48 kHz mono and
8 kHz mono -- converted to 16 kHz mono with ``ops.resample_design``'s filters as ONE clip.  Per case: ``ms``: device events
around the bare ``ds2_resample`` call (its read-back of the two offsets and its launch; output and offsets allocated outside),
median of --reps after warm-up; ``bytes_in`` / ``bytes_out``: what the launch must move; ``gbps``: their sum over ``ms``;
``copy_ms``: a device-to-device copy that moves the same number of bytes (half of them read, half written), alternating with
the conversion in the same run; ``copy_share``: ``copy_ms / ms``, the share of the copy's bandwidth the conversion reaches;
``gmacs``: outputs x taps over ``ms``.  ``ref_ms``: tests/resample_ref.py (numpy float64) on the first --ref-seconds of the
same input, once; ``ref_max_abs_diff``: the device's outputs against it over those seconds (0 or 1: the fp32 chain may round
a sample the other way; the last K outputs, which see the rest of the hour on the device, are left out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

CASES = (('44100_stereo', 44100, 2), ('48000_mono', 48000, 1), ('8000_mono', 8000, 1))


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--ref-seconds', type=float, default=60.0)
    args = ap.parse_args()
    import torch
    from ds2hip import lib, ops
    from tests import resample_ref as ref
    assert torch.cuda.is_available(), 'resample_time.py measures on the GPU'
    med = lambda v: float(np.median(v))                                                                 # noqa: E731
    result = {'seconds': args.seconds, 'reps': args.reps, 'ref_seconds': args.ref_seconds}
    for name, rate, channels in CASES:
        L, M, taps = ops.resample_design(rate)
        K = taps.shape[1]
        frames = int(args.seconds * rate)
        n_out = ops.resample_out_len(frames, L, M)
        g = torch.Generator(device='cuda').manual_seed(rate + channels)
        pcm = torch.randint(-32768, 32768, (frames * channels,), dtype=torch.int16, device='cuda', generator=g)
        out = torch.empty(n_out, dtype=torch.int16, device='cuda')
        meta = torch.tensor([0, frames * channels, 0, n_out], dtype=torch.int64, device='cuda')
        taps_d = torch.from_numpy(np.array(taps)).to('cuda')
        half = (pcm.numel() + n_out) // 2                            # a copy that moves the same bytes: half read, half written
        src = torch.empty(half, dtype=torch.int16, device='cuda').copy_(pcm[:half] if half <= pcm.numel() else
                                                                          pcm.repeat(2)[:half])
        dst = torch.empty_like(src)
        conv = lambda: lib.call('ds2_resample', pcm, meta[:2], 1, channels, L, M, taps_d, K, out, meta[2:])   # noqa: E731
        copy = lambda: dst.copy_(src)                                                                   # noqa: E731
        for f in (conv, copy):
            for _ in range(3):
                _timed(f)
        t_conv, t_copy = [], []
        for _ in range(args.reps):                                   # alternating: both see the same machine
            t_conv.append(_timed(conv))
            t_copy.append(_timed(copy))
        ref_frames = min(frames, int(args.ref_seconds * rate))
        head = pcm[:ref_frames * channels].cpu().numpy()
        t0 = time.perf_counter()
        want = ref.resample(head, channels, L, M, taps)
        t_ref = time.perf_counter() - t0
        keep = max(len(want) - K, 0) if ref_frames < frames else len(want)
        got = out[:keep].cpu().numpy().astype(np.int64)
        bytes_in, bytes_out = 2 * pcm.numel(), 2 * n_out
        result[name] = {'rate': rate, 'channels': channels, 'L': L, 'M': M, 'taps': K, 'frames': frames, 'outputs': n_out,
                        'ms': round(med(t_conv), 4), 'ms_min': round(min(t_conv), 4),
                        'bytes_in': bytes_in, 'bytes_out': bytes_out,
                        'gbps': round((bytes_in + bytes_out) / (med(t_conv) * 1e-3) / 1e9, 1),
                        'copy_ms': round(med(t_copy), 4), 'copy_ms_min': round(min(t_copy), 4),
                        'copy_gbps': round(4 * half / (med(t_copy) * 1e-3) / 1e9, 1),
                        'copy_share': round(med(t_copy) / med(t_conv), 3),
                        'gmacs': round(n_out * K / (med(t_conv) * 1e-3) / 1e9, 1),
                        'ref_ms': round(1e3 * t_ref, 1), 'ref_outputs': int(len(want)),
                        'ref_max_abs_diff': int(np.abs(got - want[:keep].astype(np.int64)).max()) if keep else 0}
        del pcm, out, src, dst
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
