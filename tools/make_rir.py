#!/usr/bin/env python
"""Write a seeded set of synthetic room impulse responses as 16-bit mono 16 kHz WAV files, for ``training.reverb``.

    python tools/make_rir.py OUT_DIR [--rt60 0.2 0.4 0.6 0.8] [--count 4] [--seed 0] [--pre-delay-ms 2]

Each file is a direct path (the largest sample) followed by exponentially decaying Gaussian noise that has fallen by 60 dB
after its RT60; ``--count`` files per RT60 value, named ``rt<ms>_<i>.wav``.  The direct-to-reverberant ratio is drawn per
file (uniform in 0..10 dB).  A few milliseconds of silence stand in front of the direct path, as in measured RIRs: the
bank rule of ``codes.transforms.Reverb`` drops them.  This is the simplest statistical room model (Polack's), good enough
to exercise and time the stage; measured or image-method RIR sets in the same format work equally.
"""
import argparse
import os
import sys
import wave

import numpy as np

RATE = 16000


def synth_rir(rt60, rng, pre_delay=32, tail_rt60s=1.5, peak=0.9):
    """One RIR as int16: ``pre_delay`` zeros, the direct path at ``peak`` of full scale, then the decaying noise tail."""
    n = max(int(rt60 * tail_rt60s * RATE), 2)
    t = np.arange(1, n) / float(RATE)
    tail = rng.standard_normal(n - 1) * np.exp(-6.907755278982137 * t / rt60)          # ln(1000): -60 dB at t = rt60
    drr_db = rng.uniform(0.0, 10.0)
    tail *= np.sqrt(10.0 ** (-drr_db / 10.0) / np.sum(tail * tail))                     # energy relative to the direct 1
    tail = np.clip(tail, -0.98, 0.98)                                                   # the direct path stays the peak
    h = np.concatenate([np.zeros(pre_delay), [1.0], tail]) * peak
    return np.round(h * 32767.0).astype(np.int16)


def write_set(out_dir, rt60s=(0.2, 0.4, 0.6, 0.8), count=4, seed=0, pre_delay=32):
    """Write the set; returns the list of paths, in the order written."""
    rng = np.random.RandomState(seed)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for rt60 in rt60s:
        for i in range(count):
            path = os.path.join(out_dir, 'rt%04d_%02d.wav' % (int(round(rt60 * 1000)), i))
            with wave.open(path, 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(RATE)
                w.writeframes(synth_rir(float(rt60), rng, pre_delay).astype('<i2').tobytes())
            paths.append(path)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('out_dir')
    ap.add_argument('--rt60', type=float, nargs='+', default=[0.2, 0.4, 0.6, 0.8], help='RT60 values in seconds')
    ap.add_argument('--count', type=int, default=4, help='files per RT60 value')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--pre-delay-ms', type=float, default=2.0)
    args = ap.parse_args(argv)
    if any(not v > 0 for v in args.rt60) or args.count < 1:
        ap.error('RT60 values must be positive and --count at least 1')
    paths = write_set(args.out_dir, args.rt60, args.count, args.seed, int(args.pre_delay_ms * RATE / 1000.0))
    print('%d files under %s' % (len(paths), args.out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
