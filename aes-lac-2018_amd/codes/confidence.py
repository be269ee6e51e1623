"""Word and character confidences of a decoded transcript (not in the reference).

The value of a unit -- a word, or a single character -- is its SPAN POSTERIOR: the probability, under the model's own frame
posteriors, that the frames between the unit's first and last decoder offset spell exactly that unit, summed over every CTC
alignment of those frames (include/ds2hip.h, "unit posterior"; ``ds2_ctc_unit_posterior`` in ``csrc/ctc_unit.hip``).  It is
acoustic only -- no LM, no boost -- and it is conditional on the span: an error that moves a word's borders is seen only
through the frames inside them.  Nobody has measured how well this value is calibrated on a trained model.

The decoders take a ``UnitConfidence`` as ``confidence=``; they then score the label rows they already hold on the device
against the probabilities they decoded and set ``last_confidences``.
"""
import math

import torch

from ds2hip import ops

from .preprocessing import OrderedLabelEncoder


class UnitConfidence(object):
    """``unit='word'``: one value per word (``codes.align.group_words``' rule: the runs between spaces); ``unit='char'``: one
    per label.  ``score`` returns the device tensors of ``ops.ctc_unit_posterior`` without a wait; ``to_lists`` makes the
    one readback."""

    def __init__(self, label_encoder, blank_index=0, unit='word'):
        if isinstance(label_encoder, str):
            label_encoder = list(label_encoder)
        if isinstance(label_encoder, (set, list)):
            label_encoder = OrderedLabelEncoder().fit(label_encoder)
        if unit not in ('word', 'char'):
            raise ValueError("UnitConfidence: unit must be 'word' or 'char', got %r" % (unit,))
        self.label_encoder, self.blank_index, self.unit = label_encoder, int(blank_index), unit
        classes = [str(c) for c in label_encoder.classes_.tolist()]
        self.space_id = -1
        if unit == 'word':
            if ' ' not in classes:
                raise ValueError("UnitConfidence: unit='word' needs a space in the alphabet, which %r has not; use "
                                 "unit='char'" % (classes,))
            self.space_id = classes.index(' ')

    def score(self, probs, sizes, labels, offsets, lens, utt=None):
        """probs (B,T,A) PROBABILITIES and sizes (B,) on the device; labels, offsets (R,stride) and lens (R,) int32 on the
        device as a decoder's search returned them; ``utt`` (R,) int32 each row's utterance (None: row r is utterance r).
        Returns (unit_first, unit_len, unit_logp, n_units, dropped) on the device; nothing waits on the stream."""
        probs = probs.detach().contiguous().float()
        return ops.ctc_unit_posterior(probs, sizes, labels, offsets, lens, utt, self.space_id, self.blank_index)

    @staticmethod
    def lists_from(scored):
        """The readback of ``score``'s tensors: per row ``[confidence]`` in unit order, ``exp(logp)`` or None for a dropped
        unit; an invalid row has none."""
        _, _, logp, n_units, _ = scored
        logp, n_units = logp.cpu().numpy(), n_units.cpu().numpy()
        out = []
        for r in range(len(n_units)):
            n = min(max(int(n_units[r]), 0), logp.shape[1])
            out.append([None if math.isnan(v) else math.exp(v) for v in logp[r, :n].tolist()])
        return out

    def to_lists(self, probs, sizes, labels, offsets, lens, utt=None):
        return self.lists_from(self.score(probs, sizes, labels, offsets, lens, utt))


def check_decoder_confidence(decoder, confidence):
    """A decoder's ``confidence=`` argument: None, or a ``UnitConfidence`` made for the decoder's alphabet and blank."""
    if confidence is None:
        return None
    if not isinstance(confidence, UnitConfidence):
        raise TypeError('confidence must be a codes.confidence.UnitConfidence or None, got %r' % (confidence,))
    have = [str(c) for c in confidence.label_encoder.classes_.tolist()]
    want = [str(c) for c in decoder.label_encoder.classes_.tolist()]
    if have != want or confidence.blank_index != decoder.blank_index:
        raise ValueError('the UnitConfidence was made for the alphabet %r with blank %d, the decoder has %r with blank %d'
                         % (have, confidence.blank_index, want, decoder.blank_index))
    if getattr(decoder, 'log_input', False):
        raise ValueError('confidences are computed from probabilities: a decoder with log_input=True takes none')
    return confidence


def nbest_rows(labels, offsets, lens):
    """An N-best result (B,N,T), (B,N) viewed as the rows ``UnitConfidence.score`` takes, and their utterances."""
    bsz, n, t = labels.shape
    utt = torch.div(torch.arange(bsz * n, dtype=torch.int32, device=labels.device), n, rounding_mode='floor').int()
    return labels.view(bsz * n, t), offsets.view(bsz * n, t), lens.view(bsz * n), utt
