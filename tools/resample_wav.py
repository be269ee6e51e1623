#!/usr/bin/env python
"""Convert 16-bit PCM WAV files of any supported rate and 1..8 channels to 16 kHz mono WAV, on the device.

    python tools/resample_wav.py IN.wav [IN2.wav ...] --out-dir DIR [--rate 16000]

train.py and test.py keep requiring 16 kHz mono, so this is how a training corpus (or a noise or RIR set) is converted once.
Every file is read with ``codes.transforms.read_wav16`` and converted with ``codes.transforms.Resample`` (``ds2_resample``,
the filter of ``ops.resample_design``: a decision of this project, not parity with sox), one launch per file, and written
to ``DIR/<the file's own name>``.  A file that cannot be converted -- another sample width, more than eight channels, a rate
without a filter -- and two inputs with one name are refused by name before anything is written.  One line per file on
stdout: ``path rate channels frames -> path frames``."""
import argparse
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))


def main(argv=None):
    ap = argparse.ArgumentParser(description='16-bit PCM WAV of any supported rate -> 16 kHz mono WAV')
    ap.add_argument('inputs', nargs='+', metavar='IN')
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--rate', type=int, default=16000, help='output rate (default: 16000)')
    args = ap.parse_args(argv)
    from codes.transforms import Resample, read_wav16
    from ds2hip import ops
    names = [os.path.basename(p) for p in args.inputs]
    for name in names:
        if names.count(name) > 1:
            raise SystemExit('resample_wav.py: two inputs are named %s; they would be written to one file' % name)
    for p in args.inputs:                                       # a file that will be refused is refused before any work
        try:
            _, rate, _ = read_wav16(p, header_only=True)
            ops.resample_design(rate, args.rate)
        except (ValueError, OSError) as e:
            raise SystemExit('resample_wav.py: %s%s' % ('' if str(e).startswith(p) else p + ': ', e))
    os.makedirs(args.out_dir, exist_ok=True)
    resampler = Resample(args.rate, device='cuda')
    for p, name in zip(args.inputs, names):
        pcm, rate, channels = read_wav16(p)
        out = resampler(pcm, rate, channels).cpu().numpy()
        dst = os.path.join(args.out_dir, name)
        with wave.open(dst, 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(args.rate)
            w.writeframes(out.astype('<i2').tobytes())
        print('%s %d %d %d -> %s %d' % (p, rate, channels, len(pcm) // channels, dst, len(out)))


if __name__ == '__main__':
    main()
