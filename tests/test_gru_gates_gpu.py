"""The gate nonlinearities of the GRU recurrence on their own, against float64: fast_sigmoid / fast_tanh of the persistent kernels
(gru_persist_common.h, hardware exp2 / rcp, documented |error| < 3e-7, "saturates correctly") and sigmoidf_ / tanhf of the
launch-per-step kernels, through tests/gate_functions_kernel.hip (built by csrc/build.py into tests/libgate_functions.so)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BOUND = 3e-7                                     # the bound gru_persist_common.h documents
NAMES = ('fast_sigmoid', 'fast_tanh', 'sigmoidf_', 'tanhf')
_lib = {}


def _map(x):
    """x: float32 numpy array -> (4, n) float32: the four functions of NAMES."""
    if 'lib' not in _lib:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libgate_functions.so'))
        lib.gate_functions.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.gate_functions.restype = ctypes.c_int
        _lib['lib'] = lib
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    y = torch.full((4, xd.numel()), float('nan'), dtype=torch.float32, device=DEV)
    assert _lib['lib'].gate_functions(xd.data_ptr(), y.data_ptr(), xd.numel(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _reference(x):
    """float64 sigmoid and tanh of the float32 inputs, in NAMES' order."""
    x64 = x.astype(np.float64)
    with np.errstate(over='ignore'):
        sig = 1.0 / (1.0 + np.exp(-x64))
    th = np.tanh(x64)
    return np.stack([sig, th, sig, th], 0)


DENSE = np.linspace(-30.0, 30.0, 1200001).astype(np.float32)            # 5e-5 apart
_LOG = np.logspace(-8, 0, 8001).astype(np.float32)
LOGSWEEP = np.concatenate([-_LOG[::-1], _LOG])
DENORM_MAX = np.float32(np.finfo(np.float32).tiny) - np.float32(1.4e-45)   # 0x007fffff
SPECIAL = np.array([88, -88, 100, -100, 1e4, -1e4, np.inf, -np.inf, 0.0, -0.0, DENORM_MAX, -DENORM_MAX], dtype=np.float32)


def test_inputs_are_what_they_claim():
    assert DENORM_MAX.view(np.uint32) == 0x007fffff
    assert np.all(np.diff(DENSE) > 0) and DENSE[0] == -30 and DENSE[-1] == 30
    assert np.signbit(SPECIAL[9]) and SPECIAL[9] == 0


@pytest.mark.parametrize('sweep', ['dense', 'log', 'special'])
def test_gate_functions_against_float64(sweep):
    x = {'dense': DENSE, 'log': LOGSWEEP, 'special': SPECIAL}[sweep]
    got, ref = _map(x), _reference(x)
    err = np.abs(got.astype(np.float64) - ref)
    rounded = ref.astype(np.float32)                                     # the true value, correctly rounded to float32
    report = []
    for i, name in enumerate(NAMES):
        worst = int(np.nanargmax(err[i])) if not np.all(np.isnan(err[i])) else 0
        report.append('%s[%s]: max |error| %.3e at x = %r, rms %.3e' % (name, sweep, np.nanmax(err[i]), float(x[worst]),
                                                                       float(np.sqrt(np.nanmean(err[i] ** 2)))))
    print('\n'.join(report))
    for i, name in enumerate(NAMES):
        assert not np.isnan(got[i]).any(), '%s gives NaN for a non-NaN input: x = %r' % (name, x[np.isnan(got[i])][:8])
        assert float(err[i].max()) <= BOUND, report[i]
        # saturation: exactly 0 / 1 (sigmoid), -1 / 0 / +1 (tanh) wherever the true value rounds there
        for v in ((0.0, 1.0) if 'sigmoid' in name else (-1.0, 0.0, 1.0)):
            at = rounded[i] == v
            bad = at & (got[i] != v)
            assert not bad.any(), '%s != %g where the true value rounds there: x = %r -> %r' % (name, v, x[bad][:8], got[i][bad][:8])
        assert (got[i] >= (0.0 if 'sigmoid' in name else -1.0)).all() and (got[i] <= 1.0).all()


def test_gate_functions_are_monotonic_over_the_dense_sweep():
    got = _map(DENSE)
    for i, name in enumerate(NAMES):
        down = np.nonzero(np.diff(got[i]) < 0)[0]
        print('%s: %d decreasing neighbours of %d' % (name, down.size, DENSE.size - 1))
        assert down.size == 0, '%s decreases at x = %r: %r -> %r' % (name, DENSE[down[:4]], got[i][down[:4]], got[i][down[:4] + 1])


def test_gate_functions_propagate_nan():
    got = _map(np.array([np.nan, -np.nan, 1.0], dtype=np.float32))
    for i, name in enumerate(NAMES):
        assert np.isnan(got[i][0]) and np.isnan(got[i][1]) and not np.isnan(got[i][2]), name
