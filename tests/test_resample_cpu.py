"""Sample-rate conversion, the parts that need no GPU: the float64 reference against the definition, the filter design against
the reference bit for bit, the ratios, tap counts and output lengths of the eight rates, the quality of the designed filters
(conditions on the float64 reference, printed before they are asserted), every refusal by name, the C ABI's declarations, the
CLI flag and the config keys."""
import argparse
import ctypes
import os
import re
import wave

import numpy as np
import pytest

from tests import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(path, rate, channels=1, width=2, frames=160):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(bytes(frames * channels * width))
    return str(path)


# ------------------------------------------------------------------------------------------------ reference and design
@pytest.mark.parametrize('rate', [8000, 24000, 44100, 48000])
def test_polyphase_reference_equals_the_direct_definition(rate):
    """y(m) = sum_j h(m M / L - j) s[j] over the whole clip, against the (L, K) table walked by (i0, p)."""
    rng = np.random.RandomState(rate)
    L, M, taps = ref.design64(rate)
    c = ref.cutoff(L, M)
    for n in (1, 7, 300, 1201):
        s = rng.uniform(-1, 1, size=n)
        a, b = ref.convolve(s, L, M, taps), ref.direct(s, L, M, c)
        assert len(a) == len(b) == ref.out_len(n, L, M)
        # (the two evaluate h at arguments that differ by rounding: m M / L - j against (k - half) - p / L)
        assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(s).sum())


@pytest.mark.parametrize('rate', ref.RATES)
def test_design_is_the_reference_table_bit_for_bit(rate):
    from ds2hip import lib, ops
    L, M, taps = ops.resample_design(rate)
    rL, rM, rtaps = ref.design(rate)
    assert (L, M, taps.shape) == (rL, rM, rtaps.shape) and (L, M, taps.shape[1]) == ref.LMK[rate]
    assert taps.dtype == np.float32 and np.array_equal(taps.view(np.uint32), rtaps.view(np.uint32))
    assert ops.resample_design(rate) is ops.resample_design(rate, 16000)            # cached per argument tuple
    assert abs(float(taps.astype(np.float64).sum()) / L - 1.0) < 1e-3               # unit gain at 0 Hz
    for n in (0, 1, 2, M - 1, M, M + 1, 158760000):
        want = (n * L + M - 1) // M
        assert ref.out_len(n, L, M) == ops.resample_out_len(n, L, M) == lib.query('ds2_resample_out_len', n, L, M) == want


def test_equal_rates_are_the_identity_filter():
    from ds2hip import ops
    L, M, taps = ops.resample_design(16000)
    assert (L, M) == (1, 1) and taps.tolist() == [[1.0]]
    rL, rM, rtaps = ref.design(16000)
    assert (rL, rM) == (1, 1) and np.array_equal(taps, rtaps)
    x = np.array([-32768, 32767, 0, -1, 5], np.int16)
    assert np.array_equal(ref.resample(x, 1, L, M, taps), x)


def _db(v):
    return 20 * np.log10(max(float(v), 1e-300))


@pytest.mark.parametrize('rate', ref.RATES)
def test_filter_quality_on_the_float64_reference(rate):
    """Away from the first and last 400 outputs: a unit sine at 0.5, 0.75 and 0.8 of the lower Nyquist frequency comes out
    within -85 dB of the ideal sine; when downsampling, a unit sine at 1.1, 1.15 and 1.25 x 8000 Hz (where the input can hold
    it) comes out below -85 dB.  The transition band, 0.85 .. 1.05 of the cutoff, is deliberately not held."""
    L, M, taps = ref.design(rate)
    n = 1700 * M // L
    j = np.arange(n, dtype=np.float64)
    m = np.arange(ref.out_len(n, L, M), dtype=np.float64)
    assert len(m) >= 1600
    worst_pass = worst_stop = -np.inf
    for frac in (0.5, 0.75, 0.8):
        f = frac * min(rate, 16000) / 2.0
        y = ref.convolve(np.sin(2 * np.pi * f * j / rate), L, M, taps)
        err = np.abs(y - np.sin(2 * np.pi * f * m / 16000.0))[400:-400].max()
        print('resample %6d Hz: passband %7.1f Hz: error %.1f dB' % (rate, f, _db(err)))
        worst_pass = max(worst_pass, _db(err))
    for mult in (1.1, 1.15, 1.25):
        f = mult * 8000.0
        if rate > 16000 and f < rate / 2.0:
            y = ref.convolve(np.sin(2 * np.pi * f * j / rate), L, M, taps)
            out = np.abs(y)[400:-400].max()
            print('resample %6d Hz: stopband %7.1f Hz: output %.1f dB' % (rate, f, _db(out)))
            worst_stop = max(worst_stop, _db(out))
    print('resample %6d Hz: worst passband %.1f dB, worst stopband %.1f dB' % (rate, worst_pass, worst_stop))
    assert worst_pass < -85.0 and worst_stop < -85.0


# ------------------------------------------------------------------------------------------------ refusals
def test_unsupported_rates_are_refused_with_the_rate_in_the_text():
    from codes.transforms import Resample
    from ds2hip import ops
    for rate in (0, 3999, 192001, 44056, 44101, 16001):
        with pytest.raises(ValueError, match=str(rate)):
            ops.resample_design(rate)
        with pytest.raises(ValueError, match=str(rate)):                             # before anything is uploaded
            Resample(device='cuda')(np.zeros(100, np.int16), rate)
    for rate in (4000, 192000, 176400, 88200, 12000):
        L, M, taps = ops.resample_design(rate)
        assert 1 <= L <= 1024 and 1 <= M <= 4096 and taps.shape[1] % 2 == 1 and taps.shape[1] <= 1023


def test_read_wav16_reads_any_rate_and_refuses_other_widths_by_name(tmp_path):
    from codes.transforms import read_wav16
    x = np.arange(-6, 6, dtype=np.int16)
    with wave.open(str(tmp_path / 'st.wav'), 'wb') as w:
        w.setnchannels(3); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(x.astype('<i2').tobytes())
    pcm, rate, channels = read_wav16(str(tmp_path / 'st.wav'))
    assert pcm.dtype == np.int16 and np.array_equal(pcm, x) and (rate, channels) == (44100, 3)
    assert read_wav16(str(tmp_path / 'st.wav'), header_only=True) == (None, 44100, 3)
    for name, width in (('eight.wav', 1), ('twentyfour.wav', 3), ('thirtytwo.wav', 4)):
        with pytest.raises(ValueError, match=r'%s: %d-bit' % (re.escape(name), 8 * width)):
            read_wav16(_write(tmp_path / name, 48000, width=width))
    with pytest.raises(ValueError, match=r'nine\.wav: 9 channels'):
        read_wav16(_write(tmp_path / 'nine.wav', 48000, channels=9))
    (tmp_path / 'song.mp3.wav').write_bytes(b'ID3' + bytes(64))
    with pytest.raises(ValueError, match=r'song\.mp3\.wav: not a PCM WAV file'):
        read_wav16(str(tmp_path / 'song.mp3.wav'))


# ------------------------------------------------------------------------------------------------ C ABI
def test_resample_entry_points_are_declared_bound_and_exported():
    from ds2hip import lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, res, nargs in (('ds2_resample_out_len', 'size_t', 3), ('ds2_resample', 'int', 11)):
        m = re.search(r'\n\s*%s\s+%s\s*\(([^;]*?)\)\s*;' % (res, name), code)
        assert m, name + ' is not declared in include/ds2hip.h'
        assert len(m.group(1).split(',')) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(handle, name), name + ' is not exported'
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404
    assert int(re.search(r'#define\s+DS2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 404
    assert int(re.search(r'#define\s+DS2_RESAMPLE_TILE\s+(\d+)', hdr).group(1)) == ops.RESAMPLE_TILE
    for doc in ('README.md', 'DESIGN.md'):
        assert 'ds2_resample' in open(os.path.join(ROOT, doc)).read(), doc


def test_refuses_bad_arguments_without_a_launch():
    from ds2hip import lib
    fn = lib.load().ds2_resample
    p = ctypes.c_void_p(1 << 20)                                                    # never dereferenced: refused first
    ok = dict(B=1, channels=1, L=1, M=1, K=1)
    for key, bad in (('B', 0), ('B', 65536), ('channels', 0), ('channels', 9), ('L', 0), ('L', 1025), ('M', 0), ('M', 4097),
                     ('K', 0), ('K', 2), ('K', 1024), ('K', 1025), ('K', -1)):
        a = dict(ok, **{key: bad})
        assert fn(p, p, a['B'], a['channels'], a['L'], a['M'], p, a['K'], p, p, None) == lib.ERR_ARG, (key, bad)
        assert key in lib.load().ds2_last_error().decode()
    assert fn(None, p, 1, 1, 1, 1, p, 1, p, p, None) == lib.ERR_ARG


# ------------------------------------------------------------------------------------------------ CLI flag and config keys
class _Parsed(Exception):
    pass


@pytest.mark.parametrize('script', ['transcribe', 'align_long'])
def test_cli_parses_resample(script, monkeypatch):
    import importlib
    mod = importlib.import_module(script)
    real = argparse.ArgumentParser.parse_args

    def parse_and_stop(self, args=None, namespace=None):
        raise _Parsed(real(self, args, namespace))
    monkeypatch.setattr(argparse.ArgumentParser, 'parse_args', parse_and_stop)
    base = ['--audio', 'a.wav', '--output-path', 'o.jsonl'] + (['--transcript', 'a.txt'] if script == 'align_long' else [])
    with pytest.raises(_Parsed) as got:
        mod.main(base + ['--resample'])
    assert got.value.args[0].resample is True
    with pytest.raises(_Parsed) as got:
        mod.main(base)
    assert got.value.args[0].resample is False


def test_read_source_keeps_the_refusals_without_the_flag(tmp_path):
    import transcribe
    cd = _write(tmp_path / 'cd.wav', 44100, channels=2)
    with pytest.raises(ValueError, match=r'cd\.wav: sample rate 44100 Hz; transcribe.py takes 16000 Hz only'):
        transcribe.read_source(cd, False, header_only=True)
    assert transcribe.read_source(cd, True, header_only=True) == (None, 44100, 2)
    with pytest.raises(ValueError, match=r'odd\.wav: .*44056'):
        transcribe.read_source(_write(tmp_path / 'odd.wav', 44056), True, header_only=True)
    with pytest.raises(ValueError, match=r'wide\.wav: 24-bit'):
        transcribe.read_source(_write(tmp_path / 'wide.wav', 48000, width=3), True, header_only=True)


def test_config_blocks_accept_resample_and_still_refuse_unknown_keys(tmp_path):
    from codes.utils.training_utils import get_noise, get_reverb
    noise_dir, rir_dir = tmp_path / 'noise', tmp_path / 'rir'
    for d in (noise_dir, rir_dir):
        d.mkdir()
        with wave.open(str(d / 'a.wav'), 'wb') as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(np.array([0, 0, 9000, -3000, 1000, 0], '<i2').tobytes())
    for flag in (True, False):
        noise = get_noise(None, {'training': {'noise': {'path': str(noise_dir), 'resample': flag}}})
        rir = get_reverb(None, {'training': {'reverb': {'path': str(rir_dir), 'resample': flag}}})
        assert noise.resample is flag and rir.resample is flag and noise.lengths == [6] and rir.lengths == [3]
    assert get_noise(None, {'training': {'noise': {'path': str(noise_dir)}}}).resample is False
    assert get_reverb(None, {'training': {'reverb': {'path': str(rir_dir)}}}).resample is False
    with pytest.raises(ValueError, match='training.noise'):
        get_noise(None, {'training': {'noise': {'path': str(noise_dir), 'resample': True, 'resampling': True}}})
    with pytest.raises(ValueError, match='resampling'):
        get_reverb(None, {'training': {'reverb': {'path': str(rir_dir), 'resample': True, 'resampling': True}}})


def test_banks_with_resample_size_and_refuse_foreign_files_on_the_host(tmp_path):
    """What resample=True decides before any launch: a foreign noise file's length in the bank follows the output-length rule;
    another sample width and a rate without a filter are refused by name."""
    from codes.transforms import NoiseInjection, Reverb
    d = tmp_path / 'noise'
    d.mkdir()
    _write(d / 'a44.wav', 44100, channels=2, frames=4411)
    _write(d / 'b16.wav', 16000, frames=100)
    assert NoiseInjection(str(d), resample=True).lengths == [ref.out_len(4411, 160, 441), 100]
    with pytest.raises(ValueError, match=r'a44\.wav: 44100 Hz.*nothing is resampled here'):
        NoiseInjection(str(d))
    for name, kw, text in (('c8bit.wav', dict(rate=48000, width=1), r'c8bit\.wav: 48000 Hz, 8 bit'),
                           ('c_odd.wav', dict(rate=44056), r'c_odd\.wav: .*44056')):
        path = _write(d / name, **kw)
        for cls in (NoiseInjection, Reverb):
            with pytest.raises(ValueError, match=text):
                cls(str(d), resample=True)
        os.remove(path)
