"""align_long.py --gap-penalty end to end, in the manner of tests/test_align_long_cli_gpu.py: the six-clip recording of
tests/vad_ref.py through an untrained tiny model (seeded weights: what is absorbed is whatever its outputs make cheapest).
With the flag the record and the clips are what the stated rules give from ``ops.ctc_align_banded_gap``'s outputs; without it
the record has none of the new keys and is the one ``LongAligner`` without a penalty yields; the refusals are by name; and
one case on synthetic posteriors drives the re-centring of the band."""
import json
import os

import numpy as np
import pytest
import torch

from tests import align_gap_ref as gref
from tests import align_banded_ref as bref
from tests import vad_ref as ref
from tests.test_align_gap_gpu import SPACE, _recording, _words
from tests.test_align_long_cli_gpu import TRANSCRIPT, WORDS, _read_wav, _run
from tests.test_transcribe_cli_gpu import _checkpoint, _write_wav

pytestmark = pytest.mark.gpu

G = 0.1                              # (the untrained model's best symbol is 0.14 nats above its blank at the median)
NEW_KEYS = ('gap_penalty', 'gap_seconds', 'band_recentred', 'gaps')


def _six_segment_probs(ckpt, tmp_path, x, blocks):
    """The recording's probabilities as align_long.py lays them out (tests/test_align_long_cli_gpu.py checks that layout):
    -> (probs (T,A) on the device, first frame of every segment and the total, labels, target transform)."""
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import load_model
    from transcribe import batch_order
    model, _, val_t, target_t = load_model(ckpt, return_transforms=True, data_dir=str(tmp_path))
    model.eval().to('cuda')
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
    parts = {}
    for group in batch_order(blocks, 4):
        wavs = [torch.from_numpy(x[160 * blocks[i][0]:min(len(x), 160 * blocks[i][1])].astype(np.float32)
                                 * np.float32(frontend.scale)).to('cuda') for i in group]
        inputs, pct = frontend(wavs)
        out = model(inputs)
        sizes = pct.mul_(int(out.shape[1])).int()
        for k, i in enumerate(group):
            parts[i] = out[k, :int(sizes[k])].float()
    probs = torch.cat([parts[i] for i in range(len(blocks))]).contiguous()
    first = np.concatenate([[0], np.cumsum([int(parts[i].shape[0]) for i in range(len(blocks))])])
    labels = target_t[0](' '.join(TRANSCRIPT.split())).reshape(-1)
    return probs, first, labels, target_t[0]


def _runs(mask):
    """Maximal runs of True -> [(first, last)]."""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(a), int(b) - 1) for a, b in zip(edges[::2], edges[1::2])]


def test_gap_penalty_record_and_clips(tmp_path):
    from codes.align import ForcedAligner, LongAligner, diagonal_band
    from codes.segment import Segmenter
    from ds2hip import ops
    ckpt = _checkpoint(tmp_path)
    x, _ = ref.six_clip_recording()
    wav, txt = str(tmp_path / 'talk.wav'), str(tmp_path / 'talk.txt')
    _write_wav(wav, x)
    (tmp_path / 'talk.txt').write_text(TRANSCRIPT)
    base = ['--model-path', ckpt, '--data-dir', str(tmp_path), '--batch-size', '4', '--band-states', '64', '--audio', wav,
            '--transcript', txt]

    def clips(k):
        return ['--clips-dir', str(tmp_path / ('clips%d' % k)), '--clips-manifest', str(tmp_path / ('clips%d.csv' % k)),
                '--min-score-per-frame', '-1000000.0']
    out = _run(base + ['--output-path', str(tmp_path / 'gap.jsonl'), '--gap-penalty', str(G), '--max-gap-seconds', '0.3']
               + clips(0), tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    out = _run(base + ['--output-path', str(tmp_path / 'plain.jsonl')], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads((tmp_path / 'gap.jsonl').read_text())
    plain = json.loads((tmp_path / 'plain.jsonl').read_text())

    s = Segmenter()
    nb = -(-len(x) // 160)
    blocks = ref.vad_ref(x, s.rank(nb), s.margin_bins, s.min_bin, s.max_bin, s.min_speech, s.min_silence, s.pad,
                         s.max_len)['segs'].tolist()
    torch.set_grad_enabled(False)
    try:
        probs, first, labels, target_t = _six_segment_probs(ckpt, tmp_path, x, blocks)
        res = LongAligner(target_t.label_encoder, band_states=64, band_margin=16, gap_penalty=G).align(probs, labels)
        res_plain = LongAligner(target_t.label_encoder, band_states=64, band_margin=16).align(probs, labels)
        space = int(target_t.label_encoder.transform([' ']))
        t_n, n = int(probs.shape[0]), len(labels)
        i32 = lambda v: torch.tensor(np.asarray(v, dtype=np.int32).reshape(-1), device='cuda')     # noqa: E731
        if res['band_recentred'] == 0:                                  # the result IS the entry point's on the diagonal band
            lo = diagonal_band(t_n, 2 * n + 1, res['band_states']).to('cuda', torch.int32)[None]
            direct = ops.ctc_align_banded_gap(probs[None], i32(t_n), i32(labels), i32(0), i32(n), n, lo, res['band_states'],
                                              space, G)
            assert torch.equal(direct[0][0], res['states']) and torch.equal(direct[3][0], res['gap'])
            assert float(direct[4][0]) == res['score']
        probs_h = probs.cpu().numpy()
    finally:
        torch.set_grad_enabled(True)

    # without the flag: none of the new keys, and LongAligner's plain result
    assert not any(k in plain for k in NEW_KEYS) and not any('gap_frames' in g for g in plain['segments'])
    assert 'gap' not in res_plain and 'gap_frames' not in res_plain and 'band_recentred' not in res_plain
    assert sorted(res_plain) == ['band_margin', 'band_states', 'chars', 'score', 'score_per_frame', 'states', 'words']
    assert plain['score'] == pytest.approx(res_plain['score'], rel=1e-12) and plain['band_states'] == res_plain['band_states']
    assert plain['band_margin'] == res_plain['band_margin']
    assert ' '.join(g['text'] for g in plain['segments'] if g['text']).split() == WORDS

    # with it: the record by the stated rules
    states, gap = res['states'].cpu().numpy().astype(np.int64), res['gap'].cpu().numpy().astype(bool)
    assert 0 < res['gap_frames'] == int(gap.sum()) < t_n and space >= 1
    assert gref.eligible(labels, space)[states][gap].all()
    assert rec['gap_penalty'] == G and rec['band_recentred'] == res['band_recentred']
    assert rec['gap_seconds'] == round(int(gap.sum()) * 0.02, 3)
    assert rec['score'] == pytest.approx(res['score'], rel=1e-12)
    assert rec['score_per_frame'] == pytest.approx(res['score'] / t_n, rel=1e-12)          # the kernel's total, all frames
    assert set(rec) - set(plain) == set(NEW_KEYS) and set(plain) <= set(rec)
    owner = lambda t: int(np.searchsorted(first, t, side='right')) - 1                  # noqa: E731
    sec = lambda t: round(blocks[owner(t)][0] / 100.0 + ForcedAligner.frame_to_seconds(t - first[owner(t)]), 3)   # noqa: E731
    want_gaps = []
    for k in range(len(blocks)):
        want_gaps += [{'start': sec(first[k] + a), 'end': sec(first[k] + b), 'segment': k}
                      for a, b in _runs(gap[first[k]:first[k + 1]])]
    assert rec['gaps'] == want_gaps
    sym = np.where(states & 1, labels[np.minimum(states >> 1, n - 1)], 0)
    terms = np.log(probs_h[np.arange(t_n), sym].astype(np.float32)).astype(np.float64)
    segs = rec['segments']
    assert ' '.join(g['text'] for g in segs if g['text']).split() == WORDS
    for k, g in enumerate(segs):
        g_k = gap[first[k]:first[k + 1]]
        assert g['gap_frames'] == int(g_k.sum()) and g['frames'] == len(g_k)
        if (~g_k).any():
            assert g['score_per_frame'] == pytest.approx(terms[first[k]:first[k + 1]][~g_k].sum() / (~g_k).sum(), rel=1e-6)
        else:
            assert g['score_per_frame'] is None
    print('gap frames per segment: %s of %s' % ([g['gap_frames'] for g in segs], [g['frames'] for g in segs]))

    # clips: clean, with a text, and at most 0.3 s (15 frames) absorbed
    kept = [i for i, g in enumerate(segs) if g['clean'] and g['text'] and g['score_per_frame'] is not None
            and g['gap_frames'] * 0.02 <= 0.3]
    rows = [ln.split(',') for ln in (tmp_path / 'clips0.csv').read_text().splitlines()]
    assert [r[0] for r in rows] == [os.path.join('clips0', 'talk_%05d.wav' % i) for i in kept]

    # one segment (gaps of up to 2 s closed) is always clean: its clip is written at a generous limit, and with the default
    # limit of 0 only if nothing was absorbed
    for k, extra in ((1, ['--max-gap-seconds', '100000']), (2, [])):
        out = _run(base + ['--output-path', str(tmp_path / ('one%d.jsonl' % k)), '--min-silence', '2.0', '--gap-penalty',
                           str(G)] + extra + clips(k), tmp_path)
        assert out.returncode == 0, out.stderr[-3000:]
        one = json.loads((tmp_path / ('one%d.jsonl' % k)).read_text())
        g, = one['segments']
        assert g['clean'] and g['text'].split() == WORDS and g['gap_frames'] == round(one['gap_seconds'] / 0.02)
        assert all(v['segment'] == 0 for v in one['gaps'])
        written = sorted(os.listdir(str(tmp_path / ('clips%d' % k))))
        assert written == (['talk_00000.txt', 'talk_00000.wav'] if k == 1 or g['gap_frames'] == 0 else [])
        if written:
            block = [int(round(g['start'] * 100)), int(round(g['end'] * 100))]
            assert np.array_equal(_read_wav(tmp_path / ('clips%d' % k) / 'talk_00000.wav'),
                                  x[160 * block[0]:min(len(x), 160 * block[1])])


def test_gap_flags_refused_by_name(tmp_path):
    ok, txt = str(tmp_path / 'ok.wav'), str(tmp_path / 't.txt')
    _write_wav(ok, np.zeros(1600, np.int16))
    (tmp_path / 't.txt').write_text('hello\n')
    common = ['--model-path', str(tmp_path / 'none.pth'), '--audio', ok, '--transcript', txt, '--output-path',
              str(tmp_path / 'out.jsonl')]
    out = _run(common + ['--max-gap-seconds', '1.0'], tmp_path)
    assert out.returncode != 0 and '--max-gap-seconds' in out.stderr and '--gap-penalty' in out.stderr
    out = _run(common + ['--gap-penalty', '-1'], tmp_path)
    assert out.returncode != 0 and '--gap-penalty' in out.stderr
    out = _run(common + ['--gap-penalty', '1', '--max-gap-seconds', '-2'], tmp_path)
    assert out.returncode != 0 and '--max-gap-seconds' in out.stderr
    assert not os.path.exists(str(tmp_path / 'out.jsonl'))


def test_a_long_uncovered_opening_recentres_the_band(monkeypatch):
    """100 labels in 400 frames of which the first 120 are not in the transcript: the true path waits in state 0 while the
    diagonal band's lower edge has risen to 28, so the diagonal band clips it at any width the aligner may use -- here the
    widest is forced down to 64, which ``band_states`` = 64 then both starts and ends with.  Log inputs in multiples of 1/4
    (tests/test_align_gap_gpu.py's recording), so the optimum is exact and unique: the final path is the full-width
    reference's."""
    from codes.align import LongAligner
    from ds2hip import lib
    rng = np.random.default_rng(7)
    a, n, t, opening = 12, 100, 400, 120
    labels = _words(rng, n, a)
    body, ins_body = _recording(rng, labels, t - opening + 5, a)     # (its own 5 opening frames, and 115 more)
    head = (rng.integers(-40, -11, size=(opening - 5, a)) / 4.0).astype(np.float32)
    head[:, a - 1] = 0.0
    x = np.concatenate([head, body])
    ins = np.concatenate([np.ones(opening - 5, dtype=bool), ins_body])
    s_n = 2 * n + 1
    want_score, want_states, want_gap = gref.align_gap(x, labels, np.zeros(t, dtype=np.int64), 256, 0, SPACE, 1.0,
                                                       impl=bref.masked_full)
    assert np.array_equal(want_gap.astype(bool), ins) and (want_states[:opening] == 0).all()
    assert not bref.in_band(want_states, bref.diagonal(t, s_n, 64), 64)                 # the diagonal band clips it
    monkeypatch.setattr(lib, 'ALIGN_BAND_MAX', 64)
    enc = [chr(ord('a') + k) for k in range(a)]
    enc[SPACE] = ' '
    probs = torch.from_numpy(x).cuda()
    res = LongAligner(enc, band_states=64, band_margin=16, log_input=True, gap_penalty=1.0).align(probs, labels)
    assert res['band_states'] == 64 and 1 <= res['band_recentred'] <= 2
    assert np.array_equal(res['states'].cpu().numpy(), want_states)
    assert np.array_equal(res['gap'].cpu().numpy(), want_gap) and res['score'] == want_score
    assert res['gap_frames'] == int(ins.sum()) and res['band_margin'] >= 16
    stuck = LongAligner(enc, band_states=64, band_margin=16, log_input=True, gap_penalty=1.0, recentre=0).align(probs, labels)
    assert stuck['band_recentred'] == 0 and stuck['score'] < want_score and stuck['band_margin'] < 16
    off = LongAligner(enc, band_states=64, band_margin=16, log_input=True).align(probs, labels)
    assert 'band_recentred' not in off and off['score'] < stuck['score']
