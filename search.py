#!/usr/bin/env python
"""Keyword-search CLI: where in recordings of any length were the given phrases said (not in the reference).

    python search.py --model-path CKPT (--audio A.wav [B.wav ...] | --manifest M.csv [--data-dir DIR])
                     (--keyword PHRASE [--keyword PHRASE ...] | --keywords FILE) --output-path OUT.jsonl
                     [--min-score-per-char X] [--max-hits N] [--batch-size 32] [--resample]
                     [--max-segment S --min-speech S --min-silence S --pad S --percentile Q --margin-db D
                      --min-db D --max-db D]

Input, segmentation and batching are transcribe.py's (its functions are used, not copied): every file is uploaded once,
cut on the device into speech segments, and the segments, longest first, go through the frontend and the model in groups
of ``--batch-size``.  No decoder runs: each group's probabilities go to ONE ``ds2_ctc_keyword_search`` call for all
keywords (``codes.search.KeywordSearcher``).  One JSON line per input file, in input order: ``path``, ``duration``,
``noise_floor_db``, ``threshold_db``, ``speech_seconds``, ``keywords`` (the phrases as normalised for the model),
``truncated`` (the number of (segment, keyword) pairs that had more than ``--max-hits`` hits; only the first ``--max-hits``
of such a pair are listed) and ``hits``, sorted by start and then by keyword order: ``{keyword, start, end, score,
score_per_char, segment}`` with times in seconds rounded to 3 decimals -- the segment's start plus the centre of the model
output step -- and ``segment`` the index of the speech segment in time order.  A score is how far, in log-probability, the
model must leave its own best path to have said the keyword there (0 = it is the best path); a hit needs
``score >= --min-score-per-char * labels``.  THE DEFAULT of -1.0 per character IS A PLACEHOLDER: nobody has measured which
value separates hits from false alarms on a trained model.  Occurrences that cross a segment border are not found
(``--min-silence`` and ``--max-segment`` decide where borders fall); for whole words put spaces into the phrase."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))
sys.path.insert(0, ROOT)

import transcribe as tr  # noqa: E402
from codes.align import ForcedAligner  # noqa: E402


def hit_entries(segment, start_block, found):
    """``found``: KeywordSearcher's records of one segment -> the entries of ``hits``: times are the segment's start
    (block / 100) plus the centre of the model output step."""
    t0 = int(start_block) / 100.0
    sec = ForcedAligner.frame_to_seconds
    return [{'keyword': h['keyword'], 'start': round(t0 + sec(h['start_frame']), 3),
             'end': round(t0 + sec(h['end_frame']), 3), 'score': h['score'], 'score_per_char': h['score_per_char'],
             'segment': int(segment)} for h in found]


def file_record(path, n_samples, stats, keywords, entries, truncated):
    """The JSON line of one file from its hit entries: sorted by (start, keyword order), otherwise in the order given."""
    rec = tr.file_record(path, n_samples, stats, [])
    del rec['text'], rec['segments']
    order = {k: i for i, k in enumerate(keywords)}
    rec.update({'keywords': list(keywords), 'truncated': int(truncated),
                'hits': sorted(entries, key=lambda h: (h['start'], order[h['keyword']]))})
    return rec


def search_samples(path, samples, model, frontend, searcher, segmenter, batch_size, device='cuda'):
    """``samples``: 1-D int16 numpy array or tensor of one recording -> its JSON record.  One upload, one segmentation and
    one int16 -> float conversion of the whole buffer, as ``transcribe.transcribe_samples``; one keyword launch per group."""
    from ds2hip import ops
    pcm = torch.as_tensor(samples)
    n = int(pcm.numel())
    pcm = pcm.to(device)
    bounds, stats = segmenter.segment(pcm)
    blocks = stats['blocks']
    per_segment, truncated = [[] for _ in blocks], 0
    if len(blocks):
        wav, _ = ops.decode_augment(pcm, [0, n], scale=frontend.scale)
        for group in tr.batch_order(blocks, batch_size):
            inputs, input_percentages = frontend([wav[int(bounds[i][0]):int(bounds[i][1])] for i in group])
            out = model(inputs)                                                     # (B,T,A) probabilities
            sizes = input_percentages.mul_(int(out.shape[1])).int()                 # as test.py
            found, n_hits = searcher.search(out, sizes)
            truncated += int((n_hits > searcher.max_hits).sum())
            for k, i in enumerate(group):
                per_segment[i] = hit_entries(i, blocks[i][0], found[k])
    return file_record(path, n, stats, searcher.keywords, [h for seg in per_segment for h in seg], truncated)


def read_phrases(keyword_args, keywords_file):
    """``--keyword`` phrases, then the non-empty lines of ``--keywords FILE``, in that order."""
    phrases = list(keyword_args or [])
    if keywords_file:
        with open(keywords_file, encoding='utf8') as f:
            phrases += [line.rstrip('\r\n') for line in f if line.strip()]
    return phrases


def main(argv=None):
    p = argparse.ArgumentParser(description='DeepSpeech keyword search in long recordings')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--audio', nargs='+', metavar='WAV', help='16-bit mono PCM WAV files at 16 kHz, of any length')
    src.add_argument('--manifest', metavar='CSV', help='a manifest whose first column names the files')
    p.add_argument('--resample', action='store_true',
                   help='take 16-bit PCM WAV of any supported rate and 1..8 channels: converted to 16 kHz mono on the device')
    p.add_argument('--data-dir', help='directory that relative --manifest paths (and the label files) are found in')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--output-path', required=True, type=str, help='JSON lines, one per input file')
    p.add_argument('--batch-size', default=32, type=int, help='segments per forward pass (default: 32)')
    p.add_argument('--keyword', action='append', metavar='PHRASE', help='a phrase to search for (repeatable)')
    p.add_argument('--keywords', metavar='FILE', help='a file with one phrase per line')
    p.add_argument('--min-score-per-char', default=-1.0, type=float,
                   help='a hit scores at least this times its number of labels (default: -1.0, an unmeasured placeholder)')
    p.add_argument('--max-hits', default=4, type=int, help='hits listed per segment and keyword, 1..64 (default: 4)')
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
    if args.batch_size < 1:
        p.error('--batch-size must be at least 1')
    phrases = read_phrases(args.keyword, args.keywords)
    if not phrases:
        p.error('give at least one phrase with --keyword or --keywords')

    from codes.search import KeywordSearcher
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
            tr.read_source(path, args.resample, header_only=True)
        except (ValueError, OSError) as e:
            raise SystemExit('search.py: ' + str(e))

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)      # read once, for the check and the model
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('search.py: %s is a multi-task checkpoint (languages %s); search.py runs single-task models '
                         'only, as test.py evaluates them' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    try:
        searcher = KeywordSearcher(target_t[0], phrases, min_score_per_char=args.min_score_per_char,
                                   max_hits=args.max_hits)
    except ValueError as e:
        raise SystemExit('search.py: ' + str(e))
    model.eval().to('cuda')
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
    resampler = Resample(tr.SAMPLE_RATE, device='cuda') if args.resample else None

    n_hits = 0
    with open(args.output_path, 'w') as out_f:
        for name, path in files:
            try:
                samples, source = tr.source_samples(path, args.resample, resampler)
            except ValueError as e:
                raise SystemExit('search.py: ' + str(e))
            rec = search_samples(name, samples, model, frontend, searcher, segmenter, args.batch_size)
            rec.update(source)
            n_hits += len(rec['hits'])
            out_f.write(json.dumps(rec) + '\n')
            out_f.flush()
    print('Searched %d recordings for %d phrases (%d hits) -> %s' % (len(files), len(searcher.keywords), n_hits,
                                                                     args.output_path))


if __name__ == '__main__':
    main()
