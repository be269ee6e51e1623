#!/usr/bin/env python
"""Evaluation CLI with the reference's flags (reference ``test.py:12-26``): greedy-decode a manifest with a trained
checkpoint and report corpus-level WER / CER (``test.py:81-104``: total edits / total reference words, chars).
Additions: ``--decoder beam`` with ``--lm-path``, ``--hotword`` and ``--nbest N`` (the device search; with ``--nbest`` an
``Oracle Summary`` line follows the ``Test Summary``: the best of each utterance's N alternatives, WER and CER
independently; ``--nbest-path`` writes the alternatives as JSON lines); ``--confidence-path FILE`` (greedy or beam, the
device search): one JSON line per utterance with every hypothesis word's span posterior (``codes.confidence``) and whether
a minimal word alignment to the reference keeps it (``codes.metrics.word_matches``), and a ``Confidence Summary`` line
after the ``Test Summary``: the data to measure calibration with, which nobody has done for this value."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))

from codes.bias import add_hotword_arguments, booster_from_arguments, check_hotword_arguments  # noqa: E402
from codes.data import AudioDataLoader, AudioDataset  # noqa: E402
from codes.decoder import (BeamCTCDecoder, DeviceBeamCTCDecoder, GreedyDecoder, add_nbest_arguments,  # noqa: E402
                           check_nbest_arguments)
from codes.transforms import BatchSpectrogram, waveform_scale  # noqa: E402
from codes.utils.model_utils import checkpoint_langs, load_model  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description='DeepSpeech transcription')
    p.add_argument('--data-dir')
    p.add_argument('--model-path', default='models/deepspeech_final.pth')
    p.add_argument('--cuda', action='store_true', help='kept for compatibility: the model always runs on the GPU')
    p.add_argument('--manifest', metavar='DIR', default='data/test_manifest.csv')
    p.add_argument('--batch-size', default=32, type=int)
    p.add_argument('--num-workers', default=4, type=int)
    p.add_argument('--decoder', default='greedy', choices=['greedy', 'beam', 'none'], type=str,
                   help="'beam' (CTC prefix beam search, no LM) is an addition to the reference's greedy / none")
    p.add_argument('--beam-width', default=16, type=int)
    p.add_argument('--lm-path', default=None, type=str,
                   help='ARPA n-gram LM fused into --decoder beam (runs the device search; build one with '
                        'tools/make_lm.py); default: none')
    p.add_argument('--lm-unit', default='word', choices=['word', 'char'],
                   help='the tokens of the --lm-path LM: words or characters (default: word)')
    p.add_argument('--alpha', default=0.8, type=float, help='LM weight (default: 0.8; ignored without --lm-path)')
    p.add_argument('--beta', default=1.0, type=float,
                   help='bonus per LM token, a word or a character (default: 1.0; ignored without --lm-path)')
    p.add_argument('--beam-device', action='store_true',
                   help='run --decoder beam as one batched device launch (implied by --lm-path); default: the host '
                        'search, one utterance at a time')
    add_hotword_arguments(p)
    add_nbest_arguments(p)
    p.add_argument('--nbest-path', default=None, type=str, metavar='FILE',
                   help='with --decoder beam: write one JSON line per utterance, {"reference", "alternatives": [{"text", '
                        '"score", "ctc_logp", "posterior"}]}, for an external rescorer (runs the device search)')
    p.add_argument('--confidence-path', default=None, type=str, metavar='FILE',
                   help='with --decoder greedy or beam (runs the device search): write one JSON line per utterance, '
                        '{"reference", "text", "words": [{"word", "confidence", "correct"}]}')
    p.add_argument('--verbose', action='store_true')
    p.add_argument('--output-path', default=None, type=str)
    args = p.parse_args(argv)
    if args.lm_path and args.decoder != 'beam':
        p.error('--lm-path needs --decoder beam: only the beam search can fuse a language model')
    hotwords = check_hotword_arguments(p, args)
    nbest = check_nbest_arguments(p, args)
    if args.nbest_path and args.decoder != 'beam':
        p.error('--nbest-path needs --decoder beam: only the beam search has alternatives')
    if args.confidence_path and args.decoder == 'none':
        p.error('--confidence-path needs --decoder greedy or beam: without a decoder there are no words to score')

    ckpt = torch.load(args.model_path, map_location='cpu', weights_only=False)      # read once, for the check and the model
    ckpt_langs = checkpoint_langs(ckpt)
    if len(ckpt_langs) > 1:
        raise SystemExit('test.py: %s is a multi-task checkpoint (languages %s); test.py evaluates single-task models '
                         'only, as the reference\'s does' % (args.model_path, ckpt_langs))
    torch.set_grad_enabled(False)
    model, _, val_t, target_t = load_model(args.model_path, return_transforms=True, data_dir=args.data_dir, ckpt=ckpt)
    model.eval().to('cuda')
    target_t = target_t[0]
    confidence = None
    if args.confidence_path:
        from codes.confidence import UnitConfidence
        from codes.metrics import word_matches
        try:
            confidence = UnitConfidence(target_t.label_encoder)
        except ValueError as e:
            raise SystemExit('test.py: --confidence-path: ' + str(e))
    decoder = {'greedy': lambda: GreedyDecoder(target_t.label_encoder, confidence=confidence),
               'beam': lambda: BeamCTCDecoder(target_t.label_encoder, beam_width=args.beam_width),
               'none': lambda: None}[args.decoder]
    want_nbest = args.nbest is not None or bool(args.nbest_path)       # either flag runs the device search
    if args.decoder == 'beam' and (args.lm_path or args.beam_device or hotwords or want_nbest or args.confidence_path):
        def decoder():
            lm = None
            if args.lm_path:
                from codes.lm import NGramLM
                lm = NGramLM.from_arpa(args.lm_path, target_t.label_encoder.classes_.tolist(), unit=args.lm_unit)
            booster = booster_from_arguments('test.py', args, target_t) if hotwords else None
            return DeviceBeamCTCDecoder(target_t.label_encoder, beam_width=args.beam_width, lm=lm, alpha=args.alpha,
                                        beta=args.beta, booster=booster, nbest=nbest, confidence=confidence)
    decoder = decoder()
    target_decoder = GreedyDecoder(target_t.label_encoder)
    dataset = AudioDataset(args.data_dir, args.manifest, transforms=val_t, target_transforms=target_t)
    loader = AudioDataLoader(dataset, batch_size=args.batch_size, num_workers=args.num_workers, raw_audio=True)
    frontend = BatchSpectrogram(device='cuda', scale=waveform_scale(val_t))

    total_cer = total_wer = num_tokens = num_chars = 0
    oracle_wer = oracle_cer = 0                     # --nbest: the best alternative per utterance, WER and CER independently
    nbest_lines = []
    conf_lines, conf_sums = [], {True: [0, 0.0], False: [0, 0.0]}      # correct / wrong: words with a value, their sum
    output_data = []
    for wavs, targets, _, target_sizes in loader:
        inputs, input_percentages = frontend(wavs)
        out = model(inputs)                                                     # (B,T,A) probabilities
        sizes = input_percentages.mul_(int(out.shape[1])).int()                 # test.py:70-71
        if decoder is None:
            output_data.append((out.cpu().numpy(), sizes.numpy()))
            continue
        decoded, _ = decoder.decode(out, sizes)
        off = 0
        for i, n in enumerate(target_sizes.tolist()):
            reference = target_decoder.convert_to_strings([targets[off:off + n]])[0][0]
            off += n
            transcript = decoded[i][0]
            w, c = decoder.wer(transcript, reference), decoder.cer(transcript, reference)
            total_wer += w
            total_cer += c
            num_tokens += len(reference.split())
            num_chars += len(reference)
            if want_nbest:
                oracle_wer += min(decoder.wer(alt, reference) for alt in decoded[i])
                oracle_cer += min(decoder.cer(alt, reference) for alt in decoded[i])
            if args.nbest_path:
                if nbest > 1:
                    fields = zip(decoded[i], decoder.last_nbest_scores[i], decoder.last_nbest_ctc_log_probs[i],
                                 decoder.last_nbest_posteriors[i])
                else:                               # the 1-best entries: one alternative, the whole weight unless impossible
                    s = decoder.last_scores[i]
                    fields = [(transcript, s, decoder.last_ctc_log_probs[i], 1.0 if s > float('-inf') else 0.0)]
                nbest_lines.append(json.dumps({'reference': reference, 'alternatives': [
                    {'text': t_, 'score': s_, 'ctc_logp': c_, 'posterior': p_} for t_, s_, c_, p_ in fields]}))
            if confidence is not None:
                words = transcript.split()
                values = decoder.last_confidences[i][0]
                marks = word_matches(words, reference.split())
                for v, ok in zip(values, marks):
                    if v is not None:
                        conf_sums[ok][0] += 1
                        conf_sums[ok][1] += v
                conf_lines.append(json.dumps({'reference': reference, 'text': transcript, 'words': [
                    {'word': w_, 'confidence': v_, 'correct': ok_} for w_, v_, ok_ in zip(words, values, marks)]}))
            if args.verbose:
                print('Ref: {}\nHyp: {}\nWER: {}\t CER: {}\n'.format(reference.lower(), transcript.lower(),
                                                                      w / max(1, len(reference.split())),
                                                                      c / max(1, len(reference))))
    if decoder is not None:
        print('Test Summary \tAverage WER {wer:.3f}\tAverage CER {cer:.3f}\t'.format(
            wer=100.0 * total_wer / max(1, num_tokens), cer=100.0 * total_cer / max(1, num_chars)))
        if args.nbest is not None:
            print('Oracle Summary \tN-best {n}\tOracle WER {wer:.3f}\tOracle CER {cer:.3f}\t'.format(
                n=nbest, wer=100.0 * oracle_wer / max(1, num_tokens), cer=100.0 * oracle_cer / max(1, num_chars)))
        if args.nbest_path:
            with open(args.nbest_path, 'w') as f:
                f.write(''.join(line + '\n' for line in nbest_lines))
        if confidence is not None:
            (n_ok, sum_ok), (n_bad, sum_bad) = conf_sums[True], conf_sums[False]
            print('Confidence Summary \twords {n}\tcorrect {c}\tmean confidence correct {x:.3f}\twrong {y:.3f}\t'.format(
                n=n_ok + n_bad, c=n_ok, x=sum_ok / max(1, n_ok), y=sum_bad / max(1, n_bad)))
            with open(args.confidence_path, 'w') as f:
                f.write(''.join(line + '\n' for line in conf_lines))
    else:
        np.save(args.output_path, np.asarray(output_data, dtype=object), allow_pickle=True)


if __name__ == '__main__':
    main()
