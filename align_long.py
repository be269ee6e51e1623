#!/usr/bin/env python
"""Corpus cutting CLI: align a LONG recording to its whole transcript and cut both into training clips (not in the
reference, whose data scripts only consume corpora that somebody already cut).

    python align_long.py --model-path CKPT (--audio A.wav [B.wav ...] --transcript A.txt [B.txt ...] |
                         --manifest M.csv [--data-dir DIR]) --output-path OUT.jsonl [--batch-size 32]
                         [--band-states 4096 --band-margin 16] [--resample] [--gap-penalty G [--max-gap-seconds X]]
                         [--clips-dir DIR --clips-manifest FILE --min-score-per-frame X]
                         [--max-segment S --min-speech S --min-silence S --pad S --percentile Q --margin-db D
                          --min-db D --max-db D]

Per recording: the samples are uploaded once and cut into speech segments on the device (``codes.segment.Segmenter``,
transcribe.py's flags and defaults); the segments go through the frontend and the model in transcribe.py's batches; their
probabilities are laid end to end in time order (segment k owns frames [F_k, F_k + n_k)) and aligned in ONE banded launch
(``codes.align.LongAligner``, ``ds2_ctc_align_banded``) to the labels of the whole transcript file -- newlines as spaces,
runs of white space collapsed, normalised by the checkpoint's ``ToLabel``.  The alignment is then cut at the segment borders:
a word belongs to the segment that holds the start frame of its first character; a word whose characters lie in two segments
marks both as not ``clean``; a segment's ``score_per_frame`` is the float64 sum of the fp32 logs of the probabilities the path
takes at its frames, over their number.

One JSON line per recording, in input order: ``path``, ``duration``, ``frames``, ``labels``, ``score``, ``score_per_frame``
(null when the transcript cannot be aligned; the segments then carry empty texts), ``band_states``, ``band_margin``,
``noise_floor_db``, ``threshold_db``, ``speech_seconds`` and ``segments``, a list of ``{start, end, frames, text,
score_per_frame, clean, words: [{word, start, end}]}`` with times in seconds rounded to 3 decimals (frame F_k + j is at the
segment's start plus the centre of model output step j).

``--clips-dir DIR --clips-manifest FILE --min-score-per-frame X`` (together or not at all) write every segment that is
clean, has a text and scores at or above X as ``DIR/<audio stem>_<k:05d>.wav`` (its int16 samples, bit for bit) and ``.txt``
(its text), and a manifest row ``wav,txt,duration`` per clip, with paths relative to ``--data-dir`` where that is given: the
format ``codes.data.AudioDataset`` reads.  There is NO default threshold: nobody has measured what value separates good clips
from bad on a trained model.

``--gap-penalty G`` (default: off) lets the alignment skip audio the transcript does not cover -- announcements, questions
from the floor, music with voice: the blanks between words (and before the first and after the last) may absorb a frame
whatever the model says about it, at G nats per absorbed frame below the frame's best symbol
(``ds2_ctc_align_banded_gap``).  G is a placeholder: nobody has measured which value separates uncovered audio from badly
recognised covered audio on a trained model.  Without the flag such audio is force-aligned all the same and shows up only as
low segment scores.  With it:
  record    gains ``gap_penalty``, ``gap_seconds`` (0.02 s per absorbed frame), ``band_recentred`` (the launches on a band
            re-centred on the previous path, which a long uncovered opening needs) and ``gaps``, a list of ``{start, end,
            segment}``: the maximal runs of absorbed frames, cut at segment borders, from the first frame's time to the
            last's by the same frame-to-seconds rule as words.  Its ``score_per_frame`` stays the kernel's total over ALL
            frames, the absorbed frames' terms included.
  segment   gains ``gap_frames``; its ``score_per_frame`` is taken over its NON-gap frames only -- the float64 sum of the
            path's fp32 logs at those frames over their number, null if it has none -- because a clip threshold judges how
            the transcript fits the audio it covers.
  clips     a clip is written only if, beyond the conditions above, ``gap_frames * 0.02 <= --max-gap-seconds`` (default 0:
            no absorbed frame inside a clip).  A wholly uncovered segment has no text and is never written.
``--max-gap-seconds`` without ``--gap-penalty`` is refused by name.  Without ``--gap-penalty`` the records and the clips are
byte for byte what they were before the flag existed.  Skipping TEXT the audio does not contain (headers, footnotes), a
penalty per position, gaps inside words, resampling beyond ``--resample`` and other sample formats are out of scope.
Input is 16-bit mono PCM WAV at 16 kHz; anything else is refused by name before any work is done -- unless ``--resample``
is given, as in transcribe.py: a 16-bit PCM WAV of any supported rate and 1..8 channels is converted to 16 kHz mono on the
device before it is segmented, the record gains ``source_rate`` and ``source_channels``, every time refers to the 16 kHz
samples, and ``--clips-dir`` writes the CONVERTED samples (16 kHz mono, what train.py reads)."""
import argparse
import json
import math
import os
import sys
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

from codes.align import ForcedAligner, LongAligner  # noqa: E402
from transcribe import SAMPLE_RATE, batch_order, read_pcm16, read_source, source_samples  # noqa: E402,F401


FRAME_SECONDS = 0.02                # one model output step (codes.align.ForcedAligner.frame_to_seconds)


def normalised_transcript(path):
    """The whole transcript file as one line: newlines as spaces, runs of white space collapsed."""
    with open(path, 'r', encoding='utf8') as f:
        return ' '.join(f.read().split())


def recording_probs(pcm, n, model, frontend, segmenter, batch_size, alphabet_size):
    """Segment the uploaded samples and run the segments through the frontend and the model in transcribe.py's batches ->
    (blocks (n_seg, 2), stats, probs (T_total, A) on the device with the segments' valid frames in time order, frames per
    segment)."""
    from ds2hip import ops
    bounds, stats = segmenter.segment(pcm)
    blocks = stats['blocks']
    parts = [None] * len(blocks)
    if len(blocks):
        wav, _ = ops.decode_augment(pcm, [0, n], scale=frontend.scale)
        for group in batch_order(blocks, batch_size):
            inputs, input_percentages = frontend([wav[int(bounds[i][0]):int(bounds[i][1])] for i in group])
            out = model(inputs)                                                     # (B,T,A) probabilities
            sizes = input_percentages.mul_(int(out.shape[1])).int()                 # as test.py
            for k, i in enumerate(group):
                parts[i] = out[k, :int(sizes[k])].float()
    frames = [int(p.shape[0]) for p in parts]
    probs = torch.cat(parts) if parts else torch.zeros((0, alphabet_size), device=pcm.device)
    return blocks, stats, probs.contiguous(), frames


def path_terms(probs, states, labels, blank):
    """The fp32 log of the probability the path takes at each frame, as float64 (T,) on the device."""
    states = states.to(torch.int64)
    lab = torch.as_tensor(np.asarray(labels, dtype=np.int64).reshape(-1), device=probs.device)
    sym = torch.full_like(states, int(blank))
    odd = (states & 1) == 1
    sym[odd] = lab[states[odd] >> 1]
    return probs.gather(1, sym[:, None])[:, 0].log().double()


def cut_at_segments(res, blocks, frames, terms, gap=None):
    """The ``segments`` entries: ``res`` LongAligner's result over the concatenated frames, ``terms`` the path's per-frame
    terms on the host (None without an alignment).  ``gap`` (--gap-penalty: the absorbed frames, (T,) bool on the host): every
    entry gains ``gap_frames`` and its score is taken over the other frames; the ``gaps`` list is returned beside the
    entries."""
    sec = ForcedAligner.frame_to_seconds
    first = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)               # F_k, and the total at the end
    owner = lambda t: int(np.searchsorted(first, t, side='right')) - 1              # noqa: E731
    time_of = lambda t: int(blocks[owner(t)][0]) / 100.0 + sec(t - first[owner(t)])  # noqa: E731
    words = [[] for _ in frames]
    clean = [True] * len(frames)
    chars = res['chars']
    pos = 0
    for word, s, e in res['words']:
        while chars[pos][0] == ' ':
            pos += 1
        spanned = {owner(f) for _, cs, ce in chars[pos:pos + len(word)] for f in (cs, ce)}
        pos += len(word)
        if len(spanned) > 1:
            for k in spanned:
                clean[k] = False
        words[owner(s)].append({'word': word, 'start': round(time_of(s), 3), 'end': round(time_of(e), 3)})
    out = []
    gaps = []
    for k, n_k in enumerate(frames):
        spf = None if terms is None or n_k == 0 else float(terms[first[k]:first[k + 1]].sum()) / n_k
        seg = {'start': round(int(blocks[k][0]) / 100.0, 3), 'end': round(int(blocks[k][1]) / 100.0, 3), 'frames': n_k,
               'text': ' '.join(w['word'] for w in words[k]), 'score_per_frame': spf, 'clean': clean[k], 'words': words[k]}
        if gap is not None:
            g_k = gap[first[k]:first[k + 1]]
            kept = n_k - int(g_k.sum())
            seg['gap_frames'] = n_k - kept
            seg['score_per_frame'] = (None if terms is None or kept == 0
                                      else float(terms[first[k]:first[k + 1]][~g_k].sum()) / kept)
            edges = np.flatnonzero(np.diff(np.concatenate([[0], g_k.astype(np.int8), [0]])))     # run starts and ends
            gaps += [{'start': round(time_of(first[k] + a), 3), 'end': round(time_of(first[k] + b - 1), 3), 'segment': k}
                     for a, b in zip(edges[::2], edges[1::2])]
        out.append(seg)
    return out if gap is None else (out, gaps)


def align_samples(path, samples, labels, model, frontend, segmenter, aligner, batch_size, device='cuda'):
    """``samples``: 1-D int16 numpy array or tensor of one recording, ``labels`` its transcript's label ids -> (its JSON
    record, the segments' blocks)."""
    pcm = torch.as_tensor(samples)
    n = int(pcm.numel())
    pcm = pcm.to(device)
    alphabet_size = len(aligner.label_encoder.classes_)
    blocks, stats, probs, frames = recording_probs(pcm, n, model, frontend, segmenter, batch_size, alphabet_size)
    res = aligner.align(probs, labels)
    ok = math.isfinite(res['score'])
    terms = path_terms(probs, res['states'], labels, aligner.blank_index).cpu().numpy() if ok and len(frames) else None
    rec = {'path': path, 'duration': round(n / float(SAMPLE_RATE), 3), 'frames': int(sum(frames)), 'labels': int(len(labels)),
           'score': res['score'] if ok else None, 'score_per_frame': res['score_per_frame'] if ok else None,
           'band_states': res['band_states'], 'band_margin': res['band_margin'],
           'noise_floor_db': None if stats['noise_floor_db'] is None else round(stats['noise_floor_db'], 2),
           'threshold_db': None if stats['threshold_db'] is None else round(stats['threshold_db'], 2),
           'speech_seconds': round(stats['speech_seconds'], 3)}
    cut = res if ok else {'chars': [], 'words': []}
    if 'gap' not in res:
        rec['segments'] = cut_at_segments(cut, blocks, frames, terms)
        return rec, blocks
    gap = res['gap'].cpu().numpy().astype(bool)
    rec['segments'], gaps = cut_at_segments(cut, blocks, frames, terms, gap)
    rec.update(gap_penalty=aligner.gap_penalty, gap_seconds=round(int(gap.sum()) * FRAME_SECONDS, 3),
               band_recentred=res['band_recentred'], gaps=gaps)
    return rec, blocks


def write_clips(rec, blocks, samples, audio_path, clips_dir, data_dir, threshold, max_gap_seconds=None):
    """The clips of one recording -> manifest rows.  ``max_gap_seconds`` (--gap-penalty): a segment with more absorbed audio
    than this is not written."""
    stem = os.path.splitext(os.path.basename(audio_path))[0]
    name = (lambda p: os.path.relpath(os.path.abspath(p), os.path.abspath(data_dir)) if data_dir else os.path.abspath(p))
    rows = []
    for k, seg in enumerate(rec['segments']):
        if not (seg['clean'] and seg['text'] and seg['score_per_frame'] is not None and seg['score_per_frame'] >= threshold):
            continue
        if max_gap_seconds is not None and seg['gap_frames'] * FRAME_SECONDS > max_gap_seconds:
            continue
        clip = np.asarray(samples[160 * int(blocks[k][0]):min(len(samples), 160 * int(blocks[k][1]))], dtype='<i2')
        wav_path = os.path.join(clips_dir, '%s_%05d.wav' % (stem, k))
        txt_path = os.path.join(clips_dir, '%s_%05d.txt' % (stem, k))
        with wave.open(wav_path, 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(SAMPLE_RATE)
            w.writeframes(clip.tobytes())
        with open(txt_path, 'w', encoding='utf8') as f:
            f.write(seg['text'] + '\n')
        rows.append('%s,%s,%.3f' % (name(wav_path), name(txt_path), len(clip) / float(SAMPLE_RATE)))
    return rows


def main(argv=None):
    p = argparse.ArgumentParser(description='DeepSpeech alignment of long recordings to their transcripts')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--audio', nargs='+', metavar='WAV', help='16-bit mono PCM WAV files at 16 kHz, of any length')
    src.add_argument('--manifest', metavar='CSV', help='rows of audio_path,transcript_path[,...]')
    p.add_argument('--resample', action='store_true',
                   help='take 16-bit PCM WAV of any supported rate and 1..8 channels: converted to 16 kHz mono on the device')
    p.add_argument('--transcript', nargs='+', metavar='TXT', help='one transcript file per --audio file, in its order')
    p.add_argument('--data-dir', help='directory that relative --manifest paths (and the label files) are found in')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--output-path', required=True, type=str, help='JSON lines, one per recording')
    p.add_argument('--batch-size', default=32, type=int, help='segments per forward pass (default: 32)')
    p.add_argument('--band-states', default=4096, type=int, help='states per frame the alignment starts with (default: 4096)')
    p.add_argument('--band-margin', default=16, type=int,
                   help='the band is doubled while the path comes closer than this to its edge (default: 16)')
    p.add_argument('--gap-penalty', default=None, type=float, metavar='G',
                   help='let the blanks between words absorb audio the transcript does not cover, at G nats per absorbed frame '
                        'below the frame\'s best symbol (default: off; a placeholder, nobody has measured a good value)')
    p.add_argument('--max-gap-seconds', default=None, type=float, metavar='X',
                   help='with --gap-penalty: a clip is written only if it holds at most X seconds of absorbed audio (default: 0)')
    p.add_argument('--clips-dir', default=None, type=str, help='write the clean segments at or above the threshold here')
    p.add_argument('--clips-manifest', default=None, type=str, help='the manifest (wav,txt,duration) of the written clips')
    p.add_argument('--min-score-per-frame', default=None, type=float,
                   help='threshold on a segment\'s log-score per frame for --clips-dir (no default: nobody has measured one)')
    p.add_argument('--max-segment', default=15.0, type=float, help='longest segment in seconds (default: 15)')
    p.add_argument('--min-speech', default=0.25, type=float, help='shorter speech is dropped, seconds (default: 0.25)')
    p.add_argument('--min-silence', default=0.3, type=float, help='shorter gaps are closed, seconds (default: 0.3)')
    p.add_argument('--pad', default=0.1, type=float, help='kept on either side of a segment, seconds (default: 0.1)')
    p.add_argument('--percentile', default=0.1, type=float,
                   help='share of the 10 ms blocks taken as the noise floor (default: 0.1)')
    p.add_argument('--margin-db', default=12.0, type=float, help='speech exceeds the noise floor by this (default: 12)')
    p.add_argument('--min-db', default=-60.0, type=float, help='lowest threshold in dBFS (default: -60)')
    p.add_argument('--max-db', default=-30.0, type=float, help='highest threshold in dBFS (default: -30)')
    args = p.parse_args(argv)
    clip_args = (args.clips_dir, args.clips_manifest, args.min_score_per_frame)
    if any(v is None for v in clip_args) and not all(v is None for v in clip_args):
        p.error('--clips-dir, --clips-manifest and --min-score-per-frame go together')
    if args.batch_size < 1:
        p.error('--batch-size must be at least 1')
    if args.max_gap_seconds is not None and args.gap_penalty is None:
        p.error('--max-gap-seconds needs --gap-penalty')
    if args.gap_penalty is not None and not args.gap_penalty >= 0:
        p.error('--gap-penalty must not be negative')
    if args.max_gap_seconds is not None and not args.max_gap_seconds >= 0:
        p.error('--max-gap-seconds must not be negative')
    max_gap = None if args.gap_penalty is None else (args.max_gap_seconds or 0.0)
    if args.band_states < 1 or args.band_margin < 0:
        p.error('--band-states must be positive and --band-margin not negative')
    if args.audio:
        if not args.transcript or len(args.transcript) != len(args.audio):
            p.error('--audio needs --transcript with one transcript file per audio file')
        files = [(a, a, t) for a, t in zip(args.audio, args.transcript)]
    else:
        if args.transcript:
            p.error('--transcript goes with --audio; a --manifest names its transcripts itself')
        find = lambda name: name if os.path.isabs(name) or not args.data_dir else os.path.join(args.data_dir, name)  # noqa: E731
        with open(args.manifest) as f:
            rows = [[c.strip() for c in line.split(',')] for line in f if line.strip()]
        if any(len(r) < 2 for r in rows):
            p.error('--manifest rows are audio_path,transcript_path[,...]')
        files = [(r[0], find(r[0]), find(r[1])) for r in rows]

    from codes.segment import Segmenter
    from codes.transforms import BatchSpectrogram, Resample, waveform_scale
    from codes.utils.model_utils import checkpoint_langs, load_model
    try:
        segmenter = Segmenter(max_segment=args.max_segment, min_speech=args.min_speech, min_silence=args.min_silence,
                              pad=args.pad, percentile=args.percentile, margin_db=args.margin_db, min_db=args.min_db,
                              max_db=args.max_db)
    except ValueError as e:
        p.error(str(e))
    for _, path, txt in files:                              # a file that will be refused is refused before any work
        try:
            read_source(path, args.resample, header_only=True)
        except (ValueError, OSError) as e:
            raise SystemExit('align_long.py: ' + str(e))
        if not os.path.isfile(txt):
            raise SystemExit('align_long.py: %s: no such transcript file' % txt)

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)      # read once, for the check and the model
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('align_long.py: %s is a multi-task checkpoint (languages %s); align_long.py aligns with '
                         'single-task models only, as test.py evaluates them' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    model.eval().to('cuda')
    target_t = target_t[0]
    aligner = LongAligner(target_t.label_encoder, band_states=args.band_states, band_margin=args.band_margin,
                          gap_penalty=args.gap_penalty)
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
    resampler = Resample(SAMPLE_RATE, device='cuda') if args.resample else None
    if args.clips_dir is not None:
        os.makedirs(args.clips_dir, exist_ok=True)

    n_seg, clip_rows = 0, []
    with open(args.output_path, 'w') as out_f:
        for name, path, txt in files:
            try:
                samples, source = source_samples(path, args.resample, resampler)
            except ValueError as e:
                raise SystemExit('align_long.py: ' + str(e))
            # (ToLabel given a PATH reads its first line only; the whole file goes in as a string)
            labels = target_t(normalised_transcript(txt)).reshape(-1)
            rec, blocks = align_samples(name, samples, labels, model, frontend, segmenter, aligner, args.batch_size)
            rec.update(source)
            n_seg += len(rec['segments'])
            out_f.write(json.dumps(rec) + '\n')
            out_f.flush()
            if args.clips_dir is not None and rec['score'] is not None:
                if torch.is_tensor(samples):                # (--resample: the converted samples come back for the clips)
                    samples = samples.cpu().numpy()
                clip_rows += write_clips(rec, blocks, samples, path, args.clips_dir, args.data_dir, args.min_score_per_frame,
                                        max_gap)
    if args.clips_manifest is not None:
        with open(args.clips_manifest, 'w') as f:
            f.write(''.join(r + '\n' for r in clip_rows))
    print('Aligned %d recordings (%d segments) -> %s%s' % (len(files), n_seg, args.output_path, '' if args.clips_dir is None
                                                           else '; wrote %d clips to %s' % (len(clip_rows), args.clips_dir)))


if __name__ == '__main__':
    main()
