#!/usr/bin/env python
"""Transcription CLI for recordings of any length, with no transcript and nobody to cut them (not in the reference).

    python transcribe.py --model-path CKPT (--audio A.wav [B.wav ...] | --manifest M.csv [--data-dir DIR])
                         --output-path OUT.jsonl [--batch-size 32] [--decoder greedy|beam] [--beam-width W]
                         [--lm-path F --lm-unit U --alpha A --beta B] [--beam-device] [--resample]
                         [--hotword PHRASE ...] [--hotwords FILE] [--hotword-weight W] [--nbest N] [--confidence]
                         [--max-segment S --min-speech S --min-silence S --pad S --percentile Q --margin-db D
                          --min-db D --max-db D]

Every file's samples are read once and uploaded once; ``codes.segment.Segmenter`` (``ds2_vad_segment``) cuts them on the
device into speech segments of at most ``--max-segment`` seconds; the segments, longest first, go through the frontend, the
model and the decoder in groups of ``--batch-size``, as slices of the one device buffer.  One JSON line per input file, in
input order: ``path``, ``duration``, ``noise_floor_db``, ``threshold_db``, ``speech_seconds``, ``text`` (the segment texts
joined by one space) and ``segments``, a list of ``{start, end, text, words: [{word, start, end}]}`` with times in seconds
rounded to 3 decimals.  A word spans its first to its last character; a character's time is the segment's start plus the
centre of the model output step the decoder reports for it.  Model loading, amplitude scale, frontend and decoders are
test.py's.  Input is 16-bit mono PCM WAV at 16 kHz; anything else is refused by name (there is no resampling) -- unless
``--resample`` is given: a 16-bit PCM WAV of any supported rate and 1..8 channels is then uploaded as it is and converted to
16 kHz mono on the device (``codes.transforms.Resample``, ``ds2_resample``) before it is segmented; the record gains
``source_rate`` and ``source_channels``, and ``duration`` and all times refer to the 16 kHz samples.  ``--hotword`` /
``--hotwords`` boost phrases in ``--decoder beam`` (``codes.bias.PhraseBooster``, the device search); the record gains
``hotwords``, the phrases as normalised.  ``--nbest N`` (``--decoder beam``, the device search; 1..``--beam-width``): the
record gains ``nbest`` and every segment ``alternatives``, a list of ``{text, score, posterior}``, best first, element 0
being the segment's ``text``; ``words`` and all times stay those of the 1-best, and ``posterior`` is the weight of an
alternative among the ones returned under the fused score (``codes.decoder.DeviceBeamCTCDecoder``), not a calibrated
probability.  ``--confidence`` (with ``--decoder beam``: the device search): every entry of ``words`` gains ``confidence``,
the word's span posterior (``codes.confidence``; include/ds2hip.h "unit posterior") rounded to 4 decimals, or null for a
word of more than 64 characters; with ``--nbest`` every alternative gains ``word_confidences``, a list in word order.  The
value is acoustic only, conditional on the frames the decoder gave the word, and nobody has measured its calibration."""
import argparse
import json
import os
import sys
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))

from codes.align import ForcedAligner, group_words  # noqa: E402
from codes.bias import add_hotword_arguments, booster_from_arguments, check_hotword_arguments  # noqa: E402
from codes.decoder import add_nbest_arguments, check_nbest_arguments  # noqa: E402

SAMPLE_RATE = 16000


def read_pcm16(path, header_only=False):
    """The samples of a 16-bit mono PCM WAV file at 16 kHz as a 1-D int16 numpy array; anything else raises ValueError with
    the file's name.  ``header_only``: check the format and return None."""
    try:
        with wave.open(path, 'rb') as w:
            channels, width, rate, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getcomptype()
            raw = b'' if header_only else w.readframes(w.getnframes())
    except (wave.Error, EOFError) as e:
        raise ValueError('%s: not a PCM WAV file (%s)' % (path, e))
    if rate != SAMPLE_RATE:
        raise ValueError('%s: sample rate %d Hz; transcribe.py takes 16000 Hz only (there is no resampling)' % (path, rate))
    if channels != 1:
        raise ValueError('%s: %d channels; transcribe.py takes mono only' % (path, channels))
    if width != 2 or comp != 'NONE':
        raise ValueError('%s: %d-bit samples; transcribe.py takes 16-bit PCM only' % (path, 8 * width))
    return None if header_only else np.frombuffer(raw, dtype='<i2').astype(np.int16)


def read_source(path, resample, header_only=False):
    """What ``--resample`` changes about reading a file: without it ``read_pcm16`` and its refusals; with it any 16-bit PCM
    WAV of 1..8 channels whose rate has a filter (``ops.resample_design``), an unsupported rate being refused by name.
    Returns ``(samples as stored in the file or None, rate, channels)``."""
    if not resample:
        return read_pcm16(path, header_only), SAMPLE_RATE, 1
    from codes.transforms import read_wav16
    from ds2hip import ops
    samples, rate, channels = read_wav16(path, header_only)
    try:
        ops.resample_design(rate, SAMPLE_RATE)
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))
    return samples, rate, channels


def source_samples(path, resample, resampler=None):
    """The recording as 16 kHz mono int16 -- the file's own samples, or with ``--resample`` the device tensor the conversion
    leaves -- and the fields the record gains."""
    samples, rate, channels = read_source(path, resample)
    if not resample:
        return samples, {}
    return resampler(samples, rate, channels), {'source_rate': rate, 'source_channels': channels}


def batch_order(blocks, batch_size):
    """The batching rule: segments by length descending, ties by start, in consecutive groups of ``batch_size``.
    blocks: [(start, end)] -> [[index, ...], ...]."""
    order = sorted(range(len(blocks)), key=lambda i: (-(int(blocks[i][1]) - int(blocks[i][0])), int(blocks[i][0])))
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def rounded_confidences(values):
    """The values as the record prints them: 4 decimals, None staying None."""
    return [None if c is None else round(float(c), 4) for c in values]


def segment_record(start_block, end_block, text, offsets, confidences=None):
    """One entry of ``segments``: times from the segment's blocks (block / 100) and the decoder's per-character offsets.
    ``confidences``: one value per word of ``text`` (``--confidence``); every word then gains ``confidence``."""
    t0 = int(start_block) / 100.0
    offs = [int(o) for o in offsets]
    if len(offs) != len(text):
        raise ValueError('the decoder returned %d offsets for %d characters' % (len(offs), len(text)))
    sec = ForcedAligner.frame_to_seconds
    words = [{'word': w, 'start': round(t0 + sec(s), 3), 'end': round(t0 + sec(e), 3)}
             for w, s, e in group_words([(c, o, o) for c, o in zip(text, offs)])]
    if confidences is not None:
        if len(confidences) != len(words):
            raise ValueError('%d confidences for %d words' % (len(confidences), len(words)))
        for word, c in zip(words, rounded_confidences(confidences)):
            word['confidence'] = c
    return {'start': round(t0, 3), 'end': round(int(end_block) / 100.0, 3), 'text': text, 'words': words}


def file_record(path, n_samples, stats, segments):
    """The JSON line of one file from its segment entries (in time order)."""
    return {'path': path, 'duration': round(n_samples / float(SAMPLE_RATE), 3),
            'noise_floor_db': None if stats['noise_floor_db'] is None else round(stats['noise_floor_db'], 2),
            'threshold_db': None if stats['threshold_db'] is None else round(stats['threshold_db'], 2),
            'speech_seconds': round(stats['speech_seconds'], 3), 'text': ' '.join(s['text'] for s in segments),
            'segments': segments}


def segment_alternatives(decoder, k, texts, nbest):
    """``alternatives`` of utterance k of the decoder's last batch: ``[{text, score, posterior}]``, best first."""
    if nbest > 1:
        scores, post = decoder.last_nbest_scores[k], decoder.last_nbest_posteriors[k]
    else:                                                   # the 1-best entry: the whole weight, unless nothing is possible
        scores = [decoder.last_scores[k]]
        post = [1.0 if scores[0] > float('-inf') else 0.0]
    return [{'text': t, 'score': s, 'posterior': p} for t, s, p in zip(texts, scores, post)]


def transcribe_samples(path, samples, model, frontend, decoder, segmenter, batch_size, device='cuda', nbest=None,
                       confidence=False):
    """``samples``: 1-D int16 numpy array or tensor of one recording -> its JSON record.  One upload, one segmentation and
    one int16 -> float conversion of the whole buffer; every segment is a slice of that buffer.  ``nbest``: the N of
    ``--nbest`` (a ``DeviceBeamCTCDecoder(nbest=N)``); every segment then gains ``alternatives``.  ``confidence``: the
    decoder was built with a ``UnitConfidence``; words (and alternatives) gain their confidences."""
    from ds2hip import ops
    pcm = torch.as_tensor(samples)
    n = int(pcm.numel())
    pcm = pcm.to(device)
    bounds, stats = segmenter.segment(pcm)
    blocks = stats['blocks']
    entries = [None] * len(blocks)
    if len(blocks):
        wav, _ = ops.decode_augment(pcm, [0, n], scale=frontend.scale)
        for group in batch_order(blocks, batch_size):
            inputs, input_percentages = frontend([wav[int(bounds[i][0]):int(bounds[i][1])] for i in group])
            out = model(inputs)                                                     # (B,T,A) probabilities
            sizes = input_percentages.mul_(int(out.shape[1])).int()                 # as test.py
            decoded, offsets = decoder.decode(out, sizes)
            conf = decoder.last_confidences if confidence else None
            for k, i in enumerate(group):
                entries[i] = segment_record(blocks[i][0], blocks[i][1], decoded[k][0], offsets[k][0].tolist(),
                                            None if conf is None else conf[k][0])
                if nbest is not None:
                    entries[i]['alternatives'] = segment_alternatives(decoder, k, decoded[k], nbest)
                    if conf is not None:
                        for alt, values in zip(entries[i]['alternatives'], conf[k]):
                            alt['word_confidences'] = rounded_confidences(values)
    return file_record(path, n, stats, entries)


def main(argv=None):
    p = argparse.ArgumentParser(description='DeepSpeech transcription of long recordings')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--audio', nargs='+', metavar='WAV', help='16-bit mono PCM WAV files at 16 kHz, of any length')
    src.add_argument('--manifest', metavar='CSV', help='a manifest whose first column names the files')
    p.add_argument('--resample', action='store_true',
                   help='take 16-bit PCM WAV of any supported rate and 1..8 channels: converted to 16 kHz mono on the device')
    p.add_argument('--data-dir', help='directory that relative --manifest paths (and the label files) are found in')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--output-path', required=True, type=str, help='JSON lines, one per input file')
    p.add_argument('--batch-size', default=32, type=int, help='segments per forward pass (default: 32)')
    p.add_argument('--decoder', default='greedy', choices=['greedy', 'beam'], type=str)
    p.add_argument('--beam-width', default=16, type=int)
    p.add_argument('--lm-path', default=None, type=str,
                   help='ARPA n-gram LM fused into --decoder beam (runs the device search); default: none')
    p.add_argument('--lm-unit', default='word', choices=['word', 'char'])
    p.add_argument('--alpha', default=0.8, type=float, help='LM weight (default: 0.8; ignored without --lm-path)')
    p.add_argument('--beta', default=1.0, type=float, help='bonus per LM token (default: 1.0; ignored without --lm-path)')
    p.add_argument('--beam-device', action='store_true',
                   help='run --decoder beam as one batched device launch (implied by --lm-path)')
    add_hotword_arguments(p)
    add_nbest_arguments(p)
    p.add_argument('--confidence', action='store_true',
                   help='add every word\'s span posterior to the record (with --decoder beam: runs the device search)')
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
    if args.lm_path and args.decoder != 'beam':
        p.error('--lm-path needs --decoder beam: only the beam search can fuse a language model')
    hotwords = check_hotword_arguments(p, args)
    nbest = check_nbest_arguments(p, args)
    if args.batch_size < 1:
        p.error('--batch-size must be at least 1')

    from codes.decoder import BeamCTCDecoder, DeviceBeamCTCDecoder, GreedyDecoder
    from codes.segment import Segmenter
    from codes.transforms import BatchSpectrogram, Resample, waveform_scale
    from codes.utils.model_utils import checkpoint_langs, load_model
    try:
        segmenter = Segmenter(max_segment=args.max_segment, min_speech=args.min_speech, min_silence=args.min_silence,
                              pad=args.pad, percentile=args.percentile, margin_db=args.margin_db, min_db=args.min_db,
                              max_db=args.max_db)
    except ValueError as e:
        p.error(str(e))
    if args.audio:
        files = [(f, f) for f in args.audio]
    else:
        with open(args.manifest) as f:
            names = [line.split(',')[0].strip() for line in f if line.strip()]
        files = [(name, name if os.path.isabs(name) or not args.data_dir else os.path.join(args.data_dir, name))
                 for name in names]
    for _, path in files:                                   # a file that will be refused is refused before any work
        try:
            read_source(path, args.resample, header_only=True)
        except (ValueError, OSError) as e:
            raise SystemExit('transcribe.py: ' + str(e))

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)      # read once, for the check and the model
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('transcribe.py: %s is a multi-task checkpoint (languages %s); transcribe.py runs single-task '
                         'models only, as test.py evaluates them' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    model.eval().to('cuda')
    target_t = target_t[0]
    confidence = None
    if args.confidence:
        from codes.confidence import UnitConfidence
        try:
            confidence = UnitConfidence(target_t.label_encoder)
        except ValueError as e:
            raise SystemExit('transcribe.py: --confidence: ' + str(e))
    if args.decoder == 'greedy':
        decoder = GreedyDecoder(target_t.label_encoder, confidence=confidence)
    elif args.lm_path or args.beam_device or hotwords or args.nbest is not None or args.confidence:
        lm = None
        if args.lm_path:
            from codes.lm import NGramLM
            lm = NGramLM.from_arpa(args.lm_path, target_t.label_encoder.classes_.tolist(), unit=args.lm_unit)
        booster = booster_from_arguments('transcribe.py', args, target_t) if hotwords else None
        decoder = DeviceBeamCTCDecoder(target_t.label_encoder, beam_width=args.beam_width, lm=lm, alpha=args.alpha,
                                       beta=args.beta, booster=booster, nbest=nbest, confidence=confidence)
    else:
        decoder = BeamCTCDecoder(target_t.label_encoder, beam_width=args.beam_width)
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
    resampler = Resample(SAMPLE_RATE, device='cuda') if args.resample else None

    n_seg = 0
    with open(args.output_path, 'w') as out_f:
        for name, path in files:
            try:
                samples, source = source_samples(path, args.resample, resampler)
            except ValueError as e:
                raise SystemExit('transcribe.py: ' + str(e))
            rec = transcribe_samples(name, samples, model, frontend, decoder, segmenter, args.batch_size,
                                     nbest=args.nbest, confidence=args.confidence)
            rec.update(source)
            if args.nbest is not None:
                rec['nbest'] = nbest
            if hotwords:
                rec['hotwords'] = list(decoder.booster.keywords)
            n_seg += len(rec['segments'])
            out_f.write(json.dumps(rec) + '\n')
            out_f.flush()
    print('Transcribed %d recordings (%d segments) -> %s' % (len(files), n_seg, args.output_path))


if __name__ == '__main__':
    main()
