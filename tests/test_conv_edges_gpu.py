"""Every release kernel form of ds2_conv_fwd, ds2_conv2_dgrad and ds2_conv_wgrad at its dispatch edges, against exact and
float64 references.

The cases, the references and the bound are tests/conv_cases.py (checked on the CPU by test_conv_cases_cpu.py).  Every operand
sits in a flat buffer of its own, 0..3 floats off 16-byte alignment, between 64 floats of NaN (inputs, filter, bias) or of a
sentinel bit pattern (outputs, d_weight, d_bias); the workspace is exactly ds2_conv_wt_ws_floats / ds2_conv2_dgrad_ws_floats
long, NaN-filled before every call, with a sentinel guard behind it.  So nothing outside an operand and no workspace float that
no preparation kernel wrote may reach a result, and nothing outside an output may change.  Integer and selection cases are
exact; float64 cases stay under (K + S + 2) 2^-24 (|a| * |b|).  The tests assert results only, never which kernel ran.  Above
HOST_REF_LIMIT elements the float64 tap loop runs on the device (test_device_reference_is_the_numpy_reference holds the two
together).  `-s` prints, per float64 case, error / bound.  Needs an MI355X.

Measured on an MI355X (365 tests, 9 s): every integer and selection case exact in every form; the largest error / bound of
the float64 cases, per entry point and form:
  ds2_conv_fwd     gather, 6 and 9 products, 32 and 64 positions per wave 0.0002; direct conv2 KS 4 / 2 / 1 0.0002 / 0.0003 /
                   0.0005; conv1 NT 1 / 2 0.012 / 0.013
  ds2_conv2_dgrad  gather 0.0007, direct 0.0004
  ds2_conv_wgrad   conv2 direct / lds-f32 / split: d_weight 0.18 / 0.043 / 0.044, d_bias 0.055 / 0.015 / 0.012
                   conv1 direct / lds-f32 / split: d_weight 0.10 / 0.033 / 0.033, d_bias 0.060 / 0.014 / 0.012
The bound is a worst case over K up to 8192 same-signed roundings, so random data stays far inside it (the larger figures
belong to the shortest sums: TOUT = 1 .. 8, one batch element); what it is there to catch is an error that grows with the sum --
a lost partial tile, a piece added twice.  A lost bf16 plane or a wrong tap is what the exact cases catch.  No kernel bug showed;
the one defect found is in the argument contract (conv1 with t_in_frames <= 0, tests/test_conv_cases_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import conv_cases as cc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
HOST_REF_LIMIT = 400000         # elements of the largest operand above which the float64 reference runs on the device
ENV_NAMES = ('DS2_CONV_SPLIT', 'DS2_CONV_SPLIT_DGRAD', 'DS2_CONV_DGRAD_ROWS', 'DS2_CONV_DGRAD_MERGE', 'DS2_CONV_WGRAD_LDS',
             'DS2_CONV_WGRAD_BF16')
F64 = np.float64


@pytest.fixture(scope='module')
def lib():
    from ds2hip import lib as _lib
    return _lib


class Dev:
    """a Flat view on the device"""

    def __init__(self, flat):
        self.flat = flat
        self.host = torch.from_numpy(flat.buf)
        self.t = self.host.to(DEV, copy=True)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * flat.start

    def unchanged(self):
        return torch.equal(self.t.view(torch.int32), self.host.to(DEV).view(torch.int32))

    def result(self, what, shape):
        """the view's floats after a launch: finite, and every float around them what it was"""
        buf = self.t.cpu().numpy()
        assert self.flat.outside_intact(buf), '%s: written outside its view' % what
        out = self.flat.view(buf).copy().reshape(shape)
        assert np.isfinite(out).all(), '%s: %d non-finite values' % (what, (~np.isfinite(out)).sum())
        return out


def _inp(arr, off):
    return Dev(cc.Flat(arr.size, off % 4, 'nan').put(arr))


def _out(n, off):
    return Dev(cc.Flat(n, off % 4, 'sentinel'))


def _workspace(n):
    ws = cc.Flat(n, 0, 'sentinel')
    ws.view().view(np.uint32)[:] = cc.NAN_BITS
    return Dev(ws)


# --------------------------------------------------------------------------------------------- references
def device_convolve(entry, which, data, other, bias=None):
    """cc.convolve in float64 on the device: the same tap loop, term by term"""
    g = cc.GEOM[which]
    a, b, acc = (torch.from_numpy(x).to(DEV) for x in cc.prepare(entry, which, data, other, F64))
    tout = acc.shape[3] if entry == 'fwd' else b.shape[3]
    for kf in range(g.kf):
        for kt in range(g.kt):
            if entry == 'dgrad':
                t = a.shape[3]
                acc[:, :, kf:kf + 41:2, kt:kt + t] += torch.einsum('oc,bodt->bcdt', b[:, :, kf, kt], a)
                continue
            win = a[:, :, kf:kf + g.sf * (g.fout - 1) + 1:g.sf, kt:kt + g.st * (tout - 1) + 1:g.st]
            if entry == 'fwd':
                acc += torch.einsum('oc,bcdt->bodt', b[:, :, kf, kt], win)
            else:
                acc[:, :, kf, kt] = torch.einsum('bodt,bcdt->oc', b, win)
    return cc.finish(entry, acc.cpu().numpy(), bias)


def _convolve(case, data, other, bias=None):
    if max(data.size, other.size, int(np.prod(case.shapes()[2]))) > HOST_REF_LIMIT:
        return device_convolve(case.entry, case.which, data, other, bias)
    return cc.convolve(case.entry, case.which, data, other, F64, bias)


@functools.lru_cache(maxsize=3)
def _made(key):
    """operands and expectations, shared by the cases that differ in the environment only; never written to"""
    case = cc.Case(*key)
    data, other, bias, extra = cc.make_ops(case)
    m = dict(data=data, other=other, bias=bias)
    if case.ref == 'sel':
        m['want'] = cc.sel_reference(case, data, extra)
    else:
        m['want'] = _convolve(case, data, other, bias)
    if case.ref == 'fp64':
        m['scale'] = _convolve(case, np.abs(data), np.abs(other), None if bias is None else np.abs(bias))
    return m


def _check(case, m, got, got_bias=None):
    form = case.form()
    want = m['want']
    if case.ref == 'sel':
        if case.entry == 'wgrad':
            want, want_b = want
            assert np.array_equal(got_bias, want_b), 'd_bias is not +-1'
        bad = got != want
        assert not bad.any(), '%d of %d differ from the selected element, first at %s' % (
            bad.sum(), bad.size, np.argwhere(bad)[0])
        return
    if case.ref == 'int':
        bad = got.astype(F64) != want
        assert not bad.any(), '%d of %d integer results wrong, first at %s' % (bad.sum(), bad.size, np.argwhere(bad)[0])
        if case.entry == 'wgrad':
            assert np.array_equal(got_bias.astype(F64), cc.bias_grad(m['other'], F64))
        return
    ratios = {'result': cc.worst_ratio(np.abs(got.astype(F64) - want), cc.fp64_bound(form, m['scale']))}
    if case.entry == 'wgrad':
        err = np.abs(got_bias.astype(F64) - cc.bias_grad(m['other'], F64))
        ratios['d_bias'] = cc.worst_ratio(err, cc.fp64_bound(form, cc.bias_grad(np.abs(m['other']), F64)))
    for key, r in ratios.items():
        print('RATIO %s %s %s %s %.4f' % (case.entry, form.kernel, case.name, key, r))
        assert r <= 1.0, (case.name, form.kernel, key, r)


def _run(lib, monkeypatch, case):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    m = _made(case.key())
    sd, so, sr = case.shapes()
    data, other = _inp(m['data'], case.off), _inp(m['other'], case.off + 1)
    inputs = [data, other]
    res = _out(int(np.prod(sr)), case.off)
    ws = dbias = None
    if case.entry == 'fwd':
        n = lib.query('ds2_conv_wt_ws_floats', case.which)
        assert n == cc.wt_ws_floats(case.which)
        ws, bias = _workspace(n), _inp(m['bias'], case.off + 2)
        inputs.append(bias)
        lib.call('ds2_conv_fwd', case.which, data.ptr, other.ptr, bias.ptr, case.B, case.T, res.ptr, ws.ptr)
    elif case.entry == 'dgrad':
        n = lib.query('ds2_conv2_dgrad_ws_floats', case.B, case.T)
        assert n == cc.dgrad_ws_floats(case.B, case.T)
        ws = _workspace(n)
        lib.call('ds2_conv2_dgrad', data.ptr, other.ptr, case.B, case.T, res.ptr, ws.ptr, n)
    else:
        dbias = _out(32, case.off + 3)
        lib.call('ds2_conv_wgrad', case.which, data.ptr, other.ptr, case.B, case.T, res.ptr, dbias.ptr)
    torch.cuda.synchronize()
    if ws is not None:
        assert ws.flat.outside_intact(ws.t.cpu().numpy()), 'wrote behind its workspace'
    got = res.result(case.entry, sr)
    got_bias = dbias.result('d_bias', (32,)) if dbias is not None else None
    for d in inputs:
        assert d.unchanged(), 'an input changed'
    _check(case, m, got, got_bias)


@pytest.mark.parametrize('case', cc.fwd_cases(), ids=lambda c: c.name)
def test_conv_fwd_case(lib, monkeypatch, case):
    _run(lib, monkeypatch, case)


@pytest.mark.parametrize('case', cc.dgrad_cases(), ids=lambda c: c.name)
def test_conv2_dgrad_case(lib, monkeypatch, case):
    _run(lib, monkeypatch, case)


@pytest.mark.parametrize('case', cc.wgrad_cases(), ids=lambda c: c.name)
def test_conv_wgrad_case(lib, monkeypatch, case):
    _run(lib, monkeypatch, case)


@pytest.mark.parametrize('entry,which,b,t', [('fwd', 1, 2, 30), ('fwd', 2, 2, 15), ('dgrad', 2, 2, 15), ('wgrad', 1, 2, 30),
                                             ('wgrad', 2, 2, 15)])
def test_device_reference_is_the_numpy_reference(entry, which, b, t):
    case = cc.Case(entry, which, b, t, 'fp64')
    data, other, bias, _ = cc.make_ops(case)
    host = cc.convolve(entry, which, data, other, F64, bias)
    dev = device_convolve(entry, which, data, other, bias)
    scale = cc.convolve(entry, which, np.abs(data), np.abs(other), F64, None if bias is None else np.abs(bias))
    assert host.shape == dev.shape
    assert (np.abs(host - dev) <= 1e-12 * scale).all()         # (float64 sums in another order: 2^-53 per term)
