#!/usr/bin/env python
"""Forced-alignment CLI: time every character and word of a manifest's transcripts against its audio with a trained
checkpoint, and score how well each transcript fits (not in the reference).

    python align.py --model-path CKPT --manifest M.csv --data-dir DIR --output-path OUT.jsonl
                    [--min-score-per-frame X --pruned-manifest FILE]

One JSON line per manifest row, in manifest order: ``path``, ``transcript`` (as normalised for the model), ``frames``,
``score`` and ``score_per_frame`` (null where the transcript cannot be aligned), ``words`` and ``chars`` with inclusive
``start_frame`` / ``end_frame`` of the model's output steps and ``start`` / ``end`` in seconds (the centres of those steps).
``--pruned-manifest`` writes the manifest rows whose score per frame is at or above ``--min-score-per-frame``: the way to
drop mis-transcribed clips before fine-tuning.  Same loader, frontend and model loading as test.py; one eval forward and
one ``ds2_ctc_align`` launch per minibatch."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))

from codes.align import ForcedAligner  # noqa: E402
from codes.data import AudioDataLoader, AudioDataset  # noqa: E402
from codes.transforms import BatchSpectrogram, waveform_scale  # noqa: E402
from codes.utils.model_utils import checkpoint_langs, load_model  # noqa: E402


def _spans(items, key):
    sec = ForcedAligner.frame_to_seconds
    return [{key: text, 'start_frame': s, 'end_frame': e, 'start': round(sec(s), 3), 'end': round(sec(e), 3)}
            for text, s, e in items]


def main(argv=None):
    p = argparse.ArgumentParser(description='DeepSpeech forced alignment')
    p.add_argument('--data-dir')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--manifest', metavar='DIR', default='data/test_manifest.csv')
    p.add_argument('--batch-size', default=32, type=int)
    p.add_argument('--num-workers', default=4, type=int)
    p.add_argument('--output-path', required=True, type=str, help='JSON lines, one per manifest row')
    p.add_argument('--min-score-per-frame', default=None, type=float,
                   help='threshold on the alignment log-score per frame for --pruned-manifest')
    p.add_argument('--pruned-manifest', default=None, type=str,
                   help='write the manifest rows at or above --min-score-per-frame here')
    args = p.parse_args(argv)
    if (args.min_score_per_frame is None) != (args.pruned_manifest is None):
        p.error('--min-score-per-frame and --pruned-manifest go together')

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)      # read once, for the check and the model
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('align.py: %s is a multi-task checkpoint (languages %s); align.py aligns with single-task models '
                         'only, as test.py evaluates them' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    model.eval().to('cuda')
    target_t = target_t[0]
    aligner = ForcedAligner(target_t.label_encoder)
    dataset = AudioDataset(args.data_dir, args.manifest, transforms=val_t, target_transforms=target_t)
    loader = AudioDataLoader(dataset, batch_size=args.batch_size, num_workers=args.num_workers, raw_audio=True)
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))
    with open(args.manifest) as f:
        rows = [line.strip() for line in f if line.strip()]                      # the rows AudioDataset kept, in its order

    kept, row = [], 0
    with open(args.output_path, 'w') as out_f:
        for wavs, targets, _, target_sizes in loader:
            inputs, input_percentages = frontend(wavs)
            out = model(inputs)                                                     # (B,T,A) probabilities
            sizes = input_percentages.mul_(int(out.shape[1])).int()                 # as test.py
            results = aligner.align(out, sizes, targets, target_sizes)
            off = 0
            for i, res in enumerate(results):
                ok = math.isfinite(res['score'])
                n = int(target_sizes[i])
                ids = targets[off:off + n].tolist()
                off += n
                text = ''.join(str(c) for c in target_t.label_encoder.inverse_transform(ids)) if n else ''
                out_f.write(json.dumps({
                    'path': rows[row].split(',')[0], 'transcript': text, 'frames': int(sizes[i]),
                    'score': res['score'] if ok else None,
                    'score_per_frame': res['score_per_frame'] if ok else None,
                    'words': _spans(res['words'], 'word'), 'chars': _spans(res['chars'], 'char')}) + '\n')
                if args.pruned_manifest is not None and ok and res['score_per_frame'] >= args.min_score_per_frame:
                    kept.append(rows[row])
                row += 1
    if args.pruned_manifest is not None:
        with open(args.pruned_manifest, 'w') as f:
            f.write(''.join(r + '\n' for r in kept))
    print('Aligned %d utterances -> %s%s' % (row, args.output_path, '' if args.pruned_manifest is None else
                                              '; kept %d of them in %s' % (len(kept), args.pruned_manifest)))


if __name__ == '__main__':
    main()
