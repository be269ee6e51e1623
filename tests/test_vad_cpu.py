"""Host side of the long-recording path: the header's section, the level bin, the Segmenter's conversions and refusals,
hand-worked cases of tests/vad_ref.py (the reference the kernel is held to in tests/test_vad_gpu.py), the JSON assembly of
transcribe.py and its refusal of files that are not 16-bit mono PCM at 16 kHz."""
import os
import re
import wave

import numpy as np
import pytest

from tests import vad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# blocks: min_speech 5, min_silence 6, pad 2; threshold pinned at bin 40 (any block next to a loud one is speech)
RULE = dict(rank=0, margin_bins=0, min_bin=40, max_bin=40, min_speech=5, min_silence=6, pad=2, max_len=100)


def _loud(nb, *spans):
    m = np.zeros(nb, np.int64)
    for s, e in spans:
        m[s:e] = 1
    return m


def _run_lengths(mask, value):
    return [e - s for s, e in ref.runs(mask, value)]


def test_header_declares_both_symbols():
    text = open(os.path.join(ROOT, 'include', 'ds2hip.h')).read()
    assert 'voice-activity segmentation' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'size_t\s+ds2_vad_segment_ws_bytes\s*\(\s*size_t\s+n\s*\)\s*;', code)
    m = re.search(r'int\s+ds2_vad_segment\s*\(([^;]*?)\)\s*;', code)
    assert m and len(m.group(1).split(',')) == 16
    from ds2hip import lib
    assert len(lib.SIGNATURES['ds2_vad_segment'][1]) == 16 and len(lib.SIGNATURES['ds2_vad_segment_ws_bytes'][1]) == 1
    assert re.search(r'#define\s+DS2_ABI_VERSION\s+404\b', text) and lib.ABI_VERSION == 404


def test_level_bin_is_monotone_and_bounded():
    from codes.segment import level_bin
    values = list(range(5001))
    for k in range(2, 41):
        values += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    values = sorted(set(values))
    for f in (ref.level_bin, level_bin):
        bins = [f(v) for v in values]
        assert all(a <= b for a, b in zip(bins, bins[1:]))
        assert [f(v) for v in range(4)] == [0, 1, 2, 3] and f(4) == 8 and f(7) == 11 and f(8) == 12
        assert f(3 * 160 * 2 ** 30) == 155 < ref.BINS
        for k in range(2, 41):
            assert f(2 ** k) == 4 * k and f(2 ** k - 1) == 4 * k - 1 if k > 2 else f(3) == 3
    assert [ref.level_bin(v) for v in values] == [level_bin(v) for v in values]


def test_segmenter_conversions():
    from codes.segment import Segmenter, bin_to_db, db_to_bin, seconds_to_blocks
    assert db_to_bin(-60.0) == 75 and db_to_bin(-30.0) == 115
    s = Segmenter()
    assert (s.max_len, s.min_speech, s.min_silence, s.pad) == (1500, 25, 30, 10)
    assert (s.margin_bins, s.min_bin, s.max_bin) == (16, 75, 115)
    assert seconds_to_blocks(0.254) == 25 and seconds_to_blocks(0.256) == 26 and seconds_to_blocks(2) == 200
    assert s.rank(1180) == 118 and s.rank(9) == 0 and s.rank(0) == 0 and s.rank(1) == 0
    assert Segmenter(percentile=1.0).rank(50) == 49 and Segmenter(percentile=0.0).rank(50) == 0
    # a bin's lower edge is the smallest energy of the bin, in dB relative to a full-scale square over 480 samples
    for k in (8, 75, 91, 115, 155):
        low = 10.0 ** (bin_to_db(k) / 10.0) * 480 * 32768 ** 2
        assert ref.level_bin(int(round(low))) == k and ref.level_bin(int(round(low)) - 1) < k
    assert bin_to_db(0) is None and -61.0 < bin_to_db(75) <= -60.0 and -31.0 < bin_to_db(115) <= -30.0


@pytest.mark.parametrize('kwargs, name', [
    (dict(min_speech=0.01), 'min_speech'), (dict(max_segment=0.03), 'max_segment'), (dict(pad=-0.1), 'pad'),
    (dict(pad=0.15), 'min_silence'), (dict(min_silence=0.2, pad=0.1), 'min_silence'), (dict(percentile=1.5), 'percentile'),
    (dict(percentile=-0.1), 'percentile'), (dict(margin_db=-1.0), 'margin_db'), (dict(margin_db=200.0), 'margin_db'),
    (dict(min_db=-300.0), 'min_db'), (dict(max_db=40.0), 'max_db')])
def test_segmenter_refuses_bad_settings_by_name(kwargs, name):
    from codes.segment import Segmenter
    with pytest.raises(ValueError, match=name):
        Segmenter(**kwargs)


def test_reference_closes_a_gap_one_short_of_min_silence_only():
    # loud blocks [3, 13) mark [2, 14): the three-block sum widens a loud run by one block on each side
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(40, (3, 13), (20, 30))), **RULE)
    assert _run_lengths(r['m3'], 0)[1] == RULE['min_silence'] - 1 and ref.runs(r['m3'], 1) == [(2, 14), (19, 31)]
    assert ref.runs(r['m4'], 1) == [(2, 31)] and r['segs'].tolist() == [[0, 33]]
    assert r['info'] == [1, 0, 40, 29, 40, 0, 0, 0]
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(40, (3, 13), (21, 31))), **RULE)
    assert _run_lengths(r['m3'], 0)[1] == RULE['min_silence'] and r['m4'] == r['m3']
    assert r['segs'].tolist() == [[0, 16], [18, 34]] and r['info'][:5] == [2, 0, 40, 24, 40]


def test_reference_never_bridges_leading_or_trailing_silence():
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(20, (4, 14))), **RULE)
    assert _run_lengths(r['m3'], 0) == [3, 5] and r['m4'] == r['m3'] and r['segs'].tolist() == [[1, 17]]


def test_reference_drops_a_run_one_short_of_min_speech_only():
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(30, (10, 12))), **RULE)
    assert _run_lengths(r['m4'], 1) == [RULE['min_speech'] - 1] and sum(r['m5']) == 0
    assert r['segs'].shape == (0, 2) and r['info'] == [0, 0, 40, 0, 30, 0, 0, 0]
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(30, (10, 13))), **RULE)
    assert _run_lengths(r['m4'], 1) == [RULE['min_speech']] and r['m5'] == r['m4']
    assert r['segs'].tolist() == [[7, 16]] and r['info'][:5] == [1, 0, 40, 5, 30]


def test_reference_does_not_repeat_gap_closing_after_dropping_a_blip():
    # [2, 14) speech, a gap of 6, a blip of 4, a gap of 6, [30, 40) speech: the blip goes, the 16-block gap it leaves stays
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(45, (3, 13), (21, 23), (31, 39))), **RULE)
    assert _run_lengths(r['m4'], 1) == [12, 4, 10] and _run_lengths(r['m4'], 0)[1:3] == [6, 6]
    assert r['segs'].tolist() == [[0, 16], [28, 42]]


def test_reference_pads_clamp_at_both_ends():
    r = ref.vad_ref(ref.pcm_from_blocks(_loud(30, (0, 5), (25, 30)), last=7), **RULE)
    assert ref.runs(r['m5'], 1) == [(0, 6), (24, 30)] and r['segs'].tolist() == [[0, 8], [22, 30]]
    assert r['info'][4] == 30


def test_reference_splits_a_constant_run_at_s_plus_h_every_time():
    rule = dict(RULE, max_len=20)
    r = ref.vad_ref(np.full(100 * 160, 20000, np.int16), **rule)
    assert len(set(r['S'][1:-1])) == 1 and r['S'][0] == r['S'][-1] < r['S'][1] and sum(r['m3']) == 100
    assert r['segs'].tolist() == [[10 * k, 10 * k + 10] for k in range(8)] + [[80, 100]]
    assert r['info'][:5] == [9, ref.level_bin(2 * 160 * 20000 ** 2), 40, 100, 100]
    rule = dict(RULE, max_len=21)                                   # h = 11: pieces of 11 until at most 21 are left
    r = ref.vad_ref(np.full(100 * 160, 20000, np.int16), **rule)
    assert r['segs'].tolist() == [[11 * k, 11 * k + 11] for k in range(8)] + [[88, 100]]


def test_reference_of_an_empty_recording():
    r = ref.vad_ref(np.zeros(0, np.int16), **RULE)
    assert r['segs'].shape == (0, 2) and r['info'] == [0] * 8


def test_reference_on_the_six_clip_recording():
    """The figures of the numpy prototype: six segments, each 1760 .. 1900 samples wider than its clip on either side,
    floor_bin 75 and thr 91 with the Segmenter's defaults."""
    from codes.segment import Segmenter
    x, clips = ref.six_clip_recording()
    s = Segmenter()
    nb = -(-len(x) // 160)
    r = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    assert r['info'][:3] == [6, 75, 91] and r['info'][4] == nb
    for (a, b), (lo, hi) in zip(r['segs'].tolist(), clips):
        assert 1760 <= lo - 160 * a <= 1900 and 1760 <= min(len(x), 160 * b) - hi <= 1900


def test_transcribe_json_assembly_from_hand_made_decoder_output():
    import transcribe
    # characters at output steps 0, 1, (space 2, 3), 7, 9: step t is centred on (2 t + 5) * 10 ms behind the segment's start
    seg = transcribe.segment_record(10, 200, 'AB  CD', [0, 1, 2, 3, 7, 9])
    assert seg == {'start': 0.1, 'end': 2.0, 'text': 'AB  CD',
                   'words': [{'word': 'AB', 'start': 0.15, 'end': 0.17}, {'word': 'CD', 'start': 0.29, 'end': 0.33}]}
    empty = transcribe.segment_record(333, 400, '', [])
    assert empty == {'start': 3.33, 'end': 4.0, 'text': '', 'words': []}
    with pytest.raises(ValueError, match='offsets'):
        transcribe.segment_record(0, 10, 'AB', [1])
    stats = {'noise_floor_db': -60.5056, 'threshold_db': -48.4644, 'speech_seconds': 1.9}
    rec = transcribe.file_record('a.wav', 65000, stats, [seg, empty, dict(seg, text='E')])
    assert rec['path'] == 'a.wav' and rec['duration'] == 4.062 and rec['text'] == 'AB  CD  E'
    assert (rec['noise_floor_db'], rec['threshold_db'], rec['speech_seconds']) == (-60.51, -48.46, 1.9)
    assert rec['segments'][0] is seg
    none = transcribe.file_record('b.wav', 0, {'noise_floor_db': None, 'threshold_db': None, 'speech_seconds': 0.0}, [])
    assert none['text'] == '' and none['segments'] == [] and none['duration'] == 0.0 and none['noise_floor_db'] is None
    # the batching rule: by length descending, ties by start, consecutive groups
    blocks = [(0, 10), (20, 40), (50, 60), (70, 90), (100, 105)]
    assert transcribe.batch_order(blocks, 2) == [[1, 3], [0, 2], [4]]
    assert transcribe.batch_order([], 4) == []


def _wav(path, rate=16000, channels=1, width=2, frames=800):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(bytes(frames * channels * width))


def test_transcribe_refuses_other_formats_by_name(tmp_path):
    import transcribe
    _wav(tmp_path / 'ok.wav')
    assert transcribe.read_pcm16(str(tmp_path / 'ok.wav')).shape == (800,)
    assert transcribe.read_pcm16(str(tmp_path / 'ok.wav'), header_only=True) is None
    for name, kwargs, what in (('fast.wav', dict(rate=22050), '22050 Hz'), ('two.wav', dict(channels=2), '2 channels'),
                               ('byte.wav', dict(width=1), '8-bit')):
        _wav(tmp_path / name, **kwargs)
        for header_only in (False, True):
            with pytest.raises(ValueError) as e:
                transcribe.read_pcm16(str(tmp_path / name), header_only=header_only)
            assert name in str(e.value) and what in str(e.value)
    (tmp_path / 'text.wav').write_text('not audio at all')
    with pytest.raises(ValueError, match='text.wav'):
        transcribe.read_pcm16(str(tmp_path / 'text.wav'))
