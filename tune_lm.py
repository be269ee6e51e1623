#!/usr/bin/env python
"""Tune the LM fusion weights of ``test.py --decoder beam --lm-path`` on a validation manifest.

    python tune_lm.py --model-path CKPT --data-dir DATA --manifest DATA/val.csv --lm-path word3.arpa \\
        --alphas 0:2:0.25 --betas 0,0.5,1,2 --beam-width 16 --output-path tune.json

One forward pass over the manifest (``test.py``'s loader, frontend and model loading); every batch's probabilities, sizes
and targets stay on the device, then the full (alpha, beta) grid is decoded and scored there (``codes.tune.LMTuner``) and
one table comes back.  WER / CER are ``test.py``'s, so a grid entry equals the ``Test Summary`` of a ``test.py`` run with
that ``--alpha`` / ``--beta`` at the same batch size and beam width.  Not in the reference.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))

from codes.tune import LMTuner, best_point, parse_grid  # noqa: E402,F401


def main(argv=None):
    p = argparse.ArgumentParser(description='Grid search of the LM weights (alpha, beta) of the device beam search')
    p.add_argument('--data-dir')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--manifest', metavar='DIR', default='data/val_manifest.csv')
    p.add_argument('--batch-size', default=32, type=int)
    p.add_argument('--num-workers', default=4, type=int)
    p.add_argument('--beam-width', default=16, type=int)
    p.add_argument('--lm-path', default=None, type=str, help='ARPA n-gram LM (build one with tools/make_lm.py); required')
    p.add_argument('--lm-unit', default='word', choices=['word', 'char'],
                   help='the tokens of the --lm-path LM: words or characters (default: word)')
    p.add_argument('--alphas', default='0:2:0.25', help="LM weights to try: a comma list or lo:hi:step (default: 0:2:0.25)")
    p.add_argument('--betas', default='0,0.5,1,2', help='token bonuses to try: a comma list or lo:hi:step (default: 0,0.5,1,2)')
    p.add_argument('--rows-per-launch', default=2048, type=int,
                   help='(grid point, utterance) rows decoded per device launch (default: 2048, the measured best; at least one grid point)')
    p.add_argument('--cache-gb', default=8.0, type=float,
                   help="device memory for the manifest's probabilities (default: 8); a manifest that needs more is refused")
    p.add_argument('--output-path', default=None, type=str, help='write the JSON table here (default: only the Best line)')
    args = p.parse_args(argv)
    if not args.lm_path:
        p.error('--lm-path is required: tune_lm.py tunes the weights of a language model')
    try:
        alphas, betas = parse_grid(args.alphas, '--alphas'), parse_grid(args.betas, '--betas')
        if len(alphas) * len(betas) > 4096:
            raise ValueError('--alphas x --betas: %d grid points, more than 4096' % (len(alphas) * len(betas)))
    except ValueError as e:
        p.error(str(e))
    if args.rows_per_launch < 1:
        p.error('--rows-per-launch must be >= 1')

    from codes.data import AudioDataLoader, AudioDataset
    from codes.decoder import DeviceBeamCTCDecoder, GreedyDecoder
    from codes.lm import NGramLM
    from codes.metrics import DeviceErrorRate
    from codes.transforms import BatchSpectrogram, waveform_scale
    from codes.utils.model_utils import checkpoint_langs, load_model

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('tune_lm.py: %s is a multi-task checkpoint (languages %s); tune_lm.py tunes single-task models '
                         'only, as test.py evaluates them' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    model.eval().to('cuda')
    target_t = target_t[0]
    lm = NGramLM.from_arpa(args.lm_path, target_t.label_encoder.classes_.tolist(), unit=args.lm_unit)
    tuner = LMTuner(target_t.label_encoder, lm, args.beam_width, alphas, betas, rows_per_launch=args.rows_per_launch)
    greedy = GreedyDecoder(target_t.label_encoder)
    plain = DeviceBeamCTCDecoder(target_t.label_encoder, beam_width=args.beam_width)
    dataset = AudioDataset(args.data_dir, args.manifest, transforms=val_t, target_transforms=target_t)
    loader = AudioDataLoader(dataset, batch_size=args.batch_size, num_workers=args.num_workers, raw_audio=True)
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))

    # one forward pass; the outputs stay on the device
    cache, cached_bytes, budget = [], 0, int(args.cache_gb * 2 ** 30)
    for wavs, targets, _, target_sizes in loader:
        inputs, input_percentages = frontend(wavs)
        out = model(inputs).detach().contiguous().float()                       # (B,T,A) probabilities
        sizes = input_percentages.mul_(int(out.shape[1])).int()                 # test.py:79
        cached_bytes += out.numel() * out.element_size()
        if cached_bytes > budget:                   # over the budget: keep nothing, go on counting to name the needed size
            cache = []
            continue
        cache.append((out, sizes.to('cuda'), targets.to('cuda', dtype=torch.int32), target_sizes.to(dtype=torch.int32)))
    if cached_bytes > budget:
        raise SystemExit('tune_lm.py: the probabilities of %s take %.3f GB on the device, more than --cache-gb %g; '
                         'pass --cache-gb %.3f or more, or tune on a smaller manifest'
                         % (args.manifest, cached_bytes / 2 ** 30, args.cache_gb, cached_bytes / 2 ** 30 + 0.001))

    meters = {'greedy': DeviceErrorRate(tuner.space_id), 'beam_no_lm': DeviceErrorRate(tuner.space_id)}
    for out, sizes, targets, target_sizes in cache:
        meters['greedy'].update(*greedy.decode_labels(out, sizes), targets, target_sizes)
        meters['beam_no_lm'].update(*plain.decode_labels(out, sizes), targets, target_sizes)
        tuner.add_batch(out, sizes, targets, target_sizes)
    res = tuner.result()
    report = {'manifest': args.manifest, 'utterances': res['utterances'], 'ref_words': res['ref_words'],
              'ref_chars': res['ref_chars'], 'ref_len': res['ref_len'], 'beam_width': args.beam_width,
              'lm_path': args.lm_path, 'lm_unit': args.lm_unit, 'rows_per_launch': args.rows_per_launch,
              'greedy': meters['greedy'].compute(), 'beam_no_lm': meters['beam_no_lm'].compute(),
              'grid': res['grid'], 'best': res['best']}
    if args.output_path:
        with open(args.output_path, 'w') as f:
            json.dump(report, f, indent=1)
    best = res['best']
    print('Best alpha {a:g} beta {b:g} WER {wer:.3f} CER {cer:.3f}'.format(a=best['alpha'], b=best['beta'],
                                                                           wer=best['wer'], cer=best['cer']))
    return report


if __name__ == '__main__':
    main()
