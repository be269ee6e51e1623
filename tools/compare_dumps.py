"""Compare two directories written by bench.py --dump-outputs, array by array: max |a - b| against the array's scale.

    python tools/compare_dumps.py DIR_A DIR_B
"""
import os
import sys

import numpy as np


def main(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    assert names == sorted(f for f in os.listdir(b) if f.endswith('.npy')), 'the two dumps hold different arrays'
    print('%-22s %-10s %12s %12s %14s' % ('array', '', 'max|a-b|', 'max|a|', 'max|a-b|/max|a|'))
    for f in names:
        x = np.load(os.path.join(a, f)).astype(np.float64)
        y = np.load(os.path.join(b, f)).astype(np.float64)
        d = float(np.abs(x - y).max())
        scale = float(np.abs(x).max())
        print('%-22s %-10s %12.3g %12.3g %14.3g' % (f[:-4], 'identical' if np.array_equal(x, y) else 'differs', d, scale,
                                                  d / scale if scale else 0.0))


if __name__ == '__main__':
    main(*sys.argv[1:3])
