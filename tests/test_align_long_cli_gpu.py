"""align_long.py end to end on the six-clip recording of tests/vad_ref.py with an untrained tiny model (seeded weights: the
alignment is whatever fits its outputs best): the segments are the reference segmentation's, every word of the transcript
lands in exactly one segment in order, the JSON is what the stated batching, placement and ``LongAligner`` give in-process,
the written clips are slices of the recording, and what must be refused is refused by name."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import vad_ref as ref
from tests.test_transcribe_cli_gpu import _checkpoint, _write_wav

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRANSCRIPT = 'the  quick brown fox\njumps over  the lazy dog\nand runs   far away today\n'      # ~60 characters, three lines
WORDS = TRANSCRIPT.upper().split()


def _run(args, tmp_path):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'align_long.py')] + args, capture_output=True, text=True,
                          env=dict(os.environ), timeout=600, cwd=str(tmp_path))


def _read_wav(path):
    with wave.open(str(path), 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        return np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')


def test_align_a_long_recording_and_cut_it_into_clips(tmp_path):
    from codes.align import ForcedAligner, LongAligner
    from codes.data import AudioDataset
    from codes.segment import Segmenter
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    from transcribe import batch_order
    ckpt = _checkpoint(tmp_path)
    x, _ = ref.six_clip_recording()
    long_wav, txt, long_txt = str(tmp_path / 'talk.wav'), str(tmp_path / 'talk.txt'), str(tmp_path / 'long.txt')
    _write_wav(long_wav, x)
    (tmp_path / 'talk.txt').write_text(TRANSCRIPT)
    (tmp_path / 'long.txt').write_text('so many words that no frame is left for them ' * 200)
    base = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--batch-size', '4', '--band-states', '64']
    texts = []
    for k, threshold in enumerate(('-1000000.0', '1.0')):            # every clean segment | none (scores are negative)
        out = _run(base + ['--audio', long_wav, '--transcript', txt, '--output-path', str(tmp_path / ('out%d.jsonl' % k)),
                           '--clips-dir', str(tmp_path / ('clips%d' % k)), '--clips-manifest',
                           str(tmp_path / ('clips%d.csv' % k)), '--min-score-per-frame', threshold], tmp_path)
        assert out.returncode == 0, out.stderr[-3000:]
        texts.append((tmp_path / ('out%d.jsonl' % k)).read_text())
    assert texts[0] == texts[1]
    rec, = [json.loads(ln) for ln in texts[0].splitlines()]

    s = Segmenter()
    nb = -(-len(x) // 160)
    want = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad, s.max_len)
    blocks = want['segs'].tolist()
    segs = rec['segments']
    assert len(segs) == len(blocks) == 6
    assert [(g['start'], g['end']) for g in segs] == [(a / 100.0, b / 100.0) for a, b in blocks]
    assert rec['path'] == long_wav and rec['duration'] == round(len(x) / 16000.0, 3)
    assert rec['speech_seconds'] == want['info'][3] / 100.0
    assert rec['frames'] == sum(g['frames'] for g in segs) and all(g['frames'] > 0 for g in segs)
    assert rec['labels'] == len(' '.join(WORDS)) and rec['band_states'] >= 64
    assert rec['score'] is not None and rec['score'] < 0
    assert rec['score_per_frame'] == pytest.approx(rec['score'] / rec['frames'], rel=1e-12)
    # every word of the transcript exactly once, in order
    assert ' '.join(g['text'] for g in segs if g['text']).split() == WORDS
    last = 0.0
    for g in segs:
        assert g['text'] == ' '.join(w['word'] for w in g['words'])
        for w in g['words']:
            assert last <= w['start'] <= w['end'] and g['start'] <= w['start'] <= g['end']
            if g['clean']:
                assert w['end'] <= g['end']
            last = w['start']
    assert rec['score'] == pytest.approx(sum(g['score_per_frame'] * g['frames'] for g in segs), rel=1e-6)

    # in-process: the same segments, longest first (ties by start) in groups of 4, through the frontend and the model; the
    # valid frames laid end to end in time order; one LongAligner over all of them
    torch.set_grad_enabled(False)
    try:
        model, _, val_t, target_t = load_model(ckpt, return_transforms=True, data_dir=str(tmp_path))
        model.eval().to('cuda')
        frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
        parts = {}
        groups = batch_order(blocks, 4)
        assert [i for g in groups for i in g] != list(range(6)) and [len(g) for g in groups] == [4, 2]
        for group in groups:
            wavs = [torch.from_numpy(x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])].astype(np.float32)
                                     * np.float32(frontend.scale)).to('cuda') for i in group]
            inputs, pct = frontend(wavs)
            out = model(inputs)
            sizes = pct.mul_(int(out.shape[1])).int()
            for k, i in enumerate(group):
                parts[i] = out[k, :int(sizes[k])].float()
        probs = torch.cat([parts[i] for i in range(6)])
        labels = target_t[0](' '.join(TRANSCRIPT.split())).reshape(-1)
        res = LongAligner(target_t[0].label_encoder, band_states=64, band_margin=16).align(probs, labels)
        first = np.concatenate([[0], np.cumsum([int(parts[i].shape[0]) for i in range(6)])])
        states = res['states'].cpu().numpy().astype(np.int64)
        sym = np.where(states & 1, labels[np.minimum(states >> 1, len(labels) - 1)], 0)
        terms = probs.cpu().numpy()[np.arange(len(states)), sym]
        terms = np.log(terms.astype(np.float32)).astype(np.float64)
    finally:
        torch.set_grad_enabled(True)
    assert [g['frames'] for g in segs] == np.diff(first).tolist()
    assert rec['score'] == pytest.approx(res['score'], rel=1e-12) and rec['band_states'] == res['band_states']
    assert rec['band_margin'] == res['band_margin']
    owner = lambda t: int(np.searchsorted(first, t, side='right')) - 1          # noqa: E731
    got_texts = [[] for _ in range(6)]
    for word, start, _ in res['words']:
        got_texts[owner(start)].append(word)
    for i, g in enumerate(segs):
        assert g['text'] == ' '.join(got_texts[i])
        assert g['score_per_frame'] == pytest.approx(terms[first[i]:first[i + 1]].sum() / g['frames'], rel=1e-6)
        for w, (word, start, end) in zip(g['words'], [v for v in res['words'] if owner(v[1]) == i]):
            assert w['word'] == word
            assert w['start'] == round(blocks[i][0] / 100.0 + ForcedAligner.frame_to_seconds(start - first[i]), 3)
            assert w['end'] == round(blocks[owner(end)][0] / 100.0 + ForcedAligner.frame_to_seconds(end - first[owner(end)]), 3)
    crossing = {k for c, cs, ce in res['chars'] if c != ' ' and owner(cs) != owner(ce) for k in (owner(cs), owner(ce))}
    assert all(not segs[k]['clean'] for k in crossing)

    # the clips of the first run: every clean segment with a text; of the second: none
    rows = [ln.split(',') for ln in (tmp_path / 'clips0.csv').read_text().splitlines()]
    # (an untrained model lets one symbol soak up the frames, so words run across the borders and few segments, if any,
    # are clean; the run with ONE segment below always writes its clip)
    kept = [i for i, g in enumerate(segs) if g['clean'] and g['text']]
    print('clean segments with a text: %s of %s' % (kept, [bool(g['text']) for g in segs]))
    assert [r[0] for r in rows] == [os.path.join('clips0', 'talk_%05d.wav' % i) for i in kept]
    for r, i in zip(rows, kept):
        clip = x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])]
        assert np.array_equal(_read_wav(tmp_path / r[0]), clip)
        assert (tmp_path / r[1]).read_text().strip() == segs[i]['text'] and r[1] == r[0][:-4] + '.txt'
        assert float(r[2]) == pytest.approx(len(clip) / 16000.0, abs=1e-3)
    assert sorted(os.listdir(str(tmp_path / 'clips0'))) == sorted(os.path.basename(c) for r in rows for c in r[:2])
    assert (tmp_path / 'clips1.csv').read_text() == '' and os.listdir(str(tmp_path / 'clips1')) == []

    # gaps of up to 2 s closed: the recording is ONE segment, so no word can cross a border -- it is clean, carries the whole
    # transcript, and its clip is written whatever the model says
    out = _run(base + ['--audio', long_wav, '--transcript', txt, '--output-path', str(tmp_path / 'one.jsonl'),
                       '--min-silence', '2.0', '--clips-dir', str(tmp_path / 'clips3'), '--clips-manifest',
                       str(tmp_path / 'clips3.csv'), '--min-score-per-frame', '-1000000.0'], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    one = json.loads((tmp_path / 'one.jsonl').read_text())
    s1 = Segmenter(min_silence=2.0)
    want1 = ref.vad_ref(x, s1.rank(nb), s1.margin_bins, s1.min_bin, s1.max_bin, s1.min_speech, s1.min_silence, s1.pad,
                        s1.max_len)['segs'].tolist()
    assert len(want1) == 1 and len(one['segments']) == 1
    g = one['segments'][0]
    assert (g['start'], g['end']) == (want1[0][0] / 100.0, want1[0][1] / 100.0) and g['frames'] == one['frames']
    assert g['clean'] and g['text'].split() == WORDS and one['score'] is not None
    assert g['score_per_frame'] == pytest.approx(one['score_per_frame'], rel=1e-6)
    row, = [ln.split(',') for ln in (tmp_path / 'clips3.csv').read_text().splitlines()]
    assert row[:2] == [os.path.join('clips3', 'talk_00000.wav'), os.path.join('clips3', 'talk_00000.txt')]
    clip = x[160 * want1[0][0]:min(len(x), 160 * want1[0][1])]
    assert np.array_equal(_read_wav(tmp_path / row[0]), clip) and float(row[2]) == pytest.approx(len(clip) / 16000.0, abs=1e-3)
    assert (tmp_path / row[1]).read_text().strip() == g['text']
    assert sorted(os.listdir(str(tmp_path / 'clips3'))) == ['talk_00000.txt', 'talk_00000.wav']
    data = AudioDataset(str(tmp_path), str(tmp_path / 'clips3.csv'), transforms=val_t, target_transforms=target_t[0])
    assert len(data) == 1 and data.durations == [float(row[2])]
    audio, target = data[0]
    assert np.array_equal(torch.as_tensor(audio.pcm).cpu().numpy().reshape(-1), clip)      # the loader's int16 samples
    assert len(target) == len(g['text']) == len(labels)

    # a transcript with more labels than there are frames cannot be aligned: null scores, empty texts, no clip
    out = _run(base + ['--audio', long_wav, '--transcript', long_txt, '--output-path', str(tmp_path / 'none.jsonl'),
                       '--clips-dir', str(tmp_path / 'clips2'), '--clips-manifest', str(tmp_path / 'clips2.csv'),
                       '--min-score-per-frame', '-1000000.0'], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    none = json.loads((tmp_path / 'none.jsonl').read_text())
    assert none['score'] is None and none['score_per_frame'] is None and none['labels'] > none['frames'] == rec['frames']
    assert [g['text'] for g in none['segments']] == [''] * 6 and all(g['words'] == [] for g in none['segments'])
    assert all(g['score_per_frame'] is None for g in none['segments'])
    assert (tmp_path / 'clips2.csv').read_text() == '' and os.listdir(str(tmp_path / 'clips2')) == []


def test_align_long_refuses_by_name(tmp_path):
    from codes.utils.io_utils import AttrDict
    ckpt = _checkpoint(tmp_path)
    ok, cd, txt = str(tmp_path / 'ok.wav'), str(tmp_path / 'cd44k.wav'), str(tmp_path / 't.txt')
    _write_wav(ok, np.zeros(1600, np.int16))
    _write_wav(cd, np.zeros(4410, np.int16), rate=44100)
    (tmp_path / 't.txt').write_text('hello\n')
    common = ['--data-dir', str(tmp_path), '--output-path', str(tmp_path / 'out.jsonl')]
    out = _run(['--model-path', ckpt, '--audio', ok, cd, '--transcript', txt, txt] + common, tmp_path)
    assert out.returncode != 0 and 'cd44k.wav' in out.stderr and '44100' in out.stderr
    assert not os.path.exists(str(tmp_path / 'out.jsonl'))           # refused before any work
    mt = str(tmp_path / 'mt.pth')
    cfg = {'model': {'name': 'mt', 'langs': ['en', 'pt_BR'], 'params': {}}, 'training': {}}
    torch.save({'args': {'config': AttrDict(cfg)}, 'state_dict': {}}, mt)
    out = _run(['--model-path', mt, '--audio', ok, '--transcript', txt] + common, tmp_path)
    assert out.returncode != 0 and 'multi-task checkpoint' in out.stderr and 'mt.pth' in out.stderr
    # the counts of --audio and --transcript must match, and the clip options go together
    out = _run(['--model-path', ckpt, '--audio', ok, ok, '--transcript', txt] + common, tmp_path)
    assert out.returncode != 0 and '--transcript' in out.stderr
    out = _run(['--model-path', ckpt, '--audio', ok, '--transcript', txt, '--clips-dir', str(tmp_path / 'c')] + common,
               tmp_path)
    assert out.returncode != 0 and 'go together' in out.stderr
