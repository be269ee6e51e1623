"""Greedy CTC decoding and edit-distance metrics (reference ``codes/decoder.py``).

``GreedyDecoder.decode(probs (B,T,A), sizes) -> (strings, offsets)`` keeps the reference's return shape
(``[[str]]`` and ``[[IntTensor]]``, ``codes/decoder.py:99-160``).  The argmax over the alphabet and the
collapse (drop blank; drop a symbol equal to the previous FRAME's symbol) run on the GPU
(``ds2_argmax_rows`` + ``ds2_greedy_collapse``); only the compacted ids cross to the host to become strings.
Edit distance replaces python-Levenshtein (absent here) with ``ds2_edit_distance`` (host C++ in libds2hip.so).
``BeamCTCDecoder`` (CTC prefix beam search, ``ds2_ctc_beam_search``) is an addition: the reference's ``test.py:21``
offers greedy / none only.  ``DeviceBeamCTCDecoder`` runs the same search for a whole batch in one
launch on the device (``ds2_ctc_beam_search_batch``), optionally fused with an n-gram LM (``codes.lm.NGramLM``); with
``nbest=N`` it returns the N best entries of each final beam (``ds2_ctc_beam_search_nbest``).
"""
import numpy as np
import torch

from ds2hip import lib, ops

from .confidence import UnitConfidence, check_decoder_confidence, nbest_rows
from .preprocessing import OrderedLabelEncoder


def _levenshtein(a, b):
    """Edit distance of two sequences of hashable items (``ds2_edit_distance``, host C++)."""
    ids = {}
    ia = np.asarray([ids.setdefault(x, len(ids)) for x in a], dtype=np.int32)
    ib = np.asarray([ids.setdefault(x, len(ids)) for x in b], dtype=np.int32)
    return lib.host_call('ds2_edit_distance', ia, len(ia), ib, len(ib))


def add_nbest_arguments(parser):
    """The ``--nbest`` flag test.py and transcribe.py share."""
    parser.add_argument('--nbest', default=None, type=int, metavar='N',
                        help='alternatives per utterance from --decoder beam, best first, 1..--beam-width (runs the device '
                             'search); default: 1')


def check_nbest_arguments(parser, args):
    """Refuse ``--nbest`` with any decoder that has no alternatives and outside 1..--beam-width; the N to use (1 if the
    flag was not given: ``args.nbest`` stays None then)."""
    if args.nbest is None:
        return 1
    if args.decoder != 'beam':
        parser.error('--nbest needs --decoder beam: only the beam search has alternatives')
    if not 1 <= args.nbest <= args.beam_width:
        parser.error('--nbest %d is outside 1..--beam-width = 1..%d: the alternatives are entries of the final beam'
                     % (args.nbest, args.beam_width))
    return args.nbest


def _device_sizes(probs, sizes):
    """``sizes``, or without them the full length T for each of the B utterances of ``probs`` (B,T,A), as a contiguous
    (B,) int32 tensor on the device of ``probs``."""
    bsz, t, _ = probs.shape
    if sizes is None:
        return torch.full((bsz,), t, dtype=torch.int32, device=probs.device)
    return torch.as_tensor(sizes).to(device=probs.device, dtype=torch.int32).contiguous()


class Decoder(object):
    def __init__(self, label_encoder, blank_index=0):
        if isinstance(label_encoder, str):
            label_encoder = list(label_encoder)
        if isinstance(label_encoder, (set, list)):
            label_encoder = OrderedLabelEncoder().fit(label_encoder)
        self.label_encoder = label_encoder
        self.blank_index = blank_index

    def wer(self, s1, s2):
        """Word-level edit distance (codes/decoder.py:49-67)."""
        return _levenshtein(s1.split(), s2.split())

    def cer(self, s1, s2):
        """Character edit distance with spaces removed (codes/decoder.py:69-78)."""
        return _levenshtein(s1.replace(' ', ''), s2.replace(' ', ''))

    def decode(self, probs, sizes=None):
        raise NotImplementedError


class GreedyDecoder(Decoder):
    """``confidence``: a ``codes.confidence.UnitConfidence`` made for the same alphabet and blank; ``decode`` then scores
    the label rows it holds on the device against the probabilities it was given and sets ``last_confidences[b][n]``, the
    list of values (one per word, or per character) of ``strings[b][n]``.  Without one nothing changes."""

    def __init__(self, label_encoder, blank_index=0, confidence=None):
        super().__init__(label_encoder, blank_index)
        self.confidence = check_decoder_confidence(self, confidence)
        self.last_confidences = None

    def _to_string(self, ids):
        if len(ids) == 0:
            return ''
        return ''.join(self.label_encoder.inverse_transform(ids))

    def convert_to_strings(self, sequences, sizes=None, remove_repetitions=False, return_offsets=False):
        """Host path for already-integer sequences (targets), codes/decoder.py:99-140."""
        strings, offsets = [], []
        for i in range(len(sequences)):
            seq = np.asarray(torch.as_tensor(sequences[i]).cpu()).reshape(-1)
            n = int(sizes[i]) if sizes is not None else len(seq)
            keep, offs = [], []
            for t in range(n):
                c = int(seq[t])
                if c == self.blank_index:
                    continue
                if remove_repetitions and t != 0 and c == int(seq[t - 1]):
                    continue
                keep.append(c)
                offs.append(t)
            strings.append([self._to_string(keep)])
            offsets.append([torch.IntTensor(offs)])
        return (strings, offsets) if return_offsets else strings

    def decode(self, probs, sizes=None):
        """probs (B,T,A) on the GPU -> ([[str]], [[IntTensor offsets]]); device argmax + collapse."""
        if not probs.is_cuda:
            raise RuntimeError('GreedyDecoder.decode runs on device tensors only')
        bsz, t, a = probs.shape
        flat = probs.contiguous().float().view(bsz * t, a)
        best = ops.argmax_rows(flat, bsz * t, a).view(bsz, t)
        sizes_d = _device_sizes(probs, sizes)
        ids, offs, lens = ops.greedy_collapse(best, sizes_d, self.blank_index)
        if self.confidence is not None:
            scored = self.confidence.score(probs, sizes_d, ids, offs, lens)
            self.last_confidences = [[c] for c in UnitConfidence.lists_from(scored)]
        ids, offs, lens = ids.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
        strings = [[self._to_string(ids[b, :lens[b]])] for b in range(bsz)]
        offsets = [[torch.IntTensor(offs[b, :lens[b]].copy())] for b in range(bsz)]
        return strings, offsets

    def decode_labels(self, probs, sizes=None):
        """``decode`` without the trip to the host: (labels (B,T) int32, lens (B,) int32) on the device, row b holding the
        label ids of ``decode``'s string b -- the layout ``ops.edit_stats`` scores.  Nothing waits on the stream."""
        if not probs.is_cuda:
            raise RuntimeError('GreedyDecoder.decode_labels runs on device tensors only')
        bsz, t, a = probs.shape
        best = ops.argmax_rows(probs.contiguous().float().view(bsz * t, a), bsz * t, a).view(bsz, t)
        sizes_d = _device_sizes(probs, sizes)
        ids, _, lens = ops.greedy_collapse(best, sizes_d, self.blank_index)
        return ids, lens


class BeamCTCDecoder(GreedyDecoder):
    """CTC prefix beam search without a language model (not in the reference).

    ``decode(probs (B,T,A), sizes)`` returns the same ``([[str]], [[IntTensor offsets]])`` shape as the greedy
    decoder; the probabilities cross to the host once and the search runs in ``ds2_ctc_beam_search``.
    ``log_input=True`` if ``probs`` are log-probabilities."""

    def __init__(self, label_encoder, blank_index=0, beam_width=16, log_input=False):
        super().__init__(label_encoder, blank_index)
        if beam_width < 1:
            raise ValueError('beam_width must be >= 1')
        self.beam_width, self.log_input = int(beam_width), bool(log_input)
        self.last_log_probs = None

    def decode(self, probs, sizes=None):
        import ctypes
        host = np.ascontiguousarray(torch.as_tensor(probs).detach().float().cpu().numpy())
        bsz, t, a = host.shape
        strings, offsets, scores = [], [], []
        for b in range(bsz):
            n = int(sizes[b]) if sizes is not None else t
            ids, offs = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
            length, logp = ctypes.c_int(0), ctypes.c_float(0.0)
            lib.host_call('ds2_ctc_beam_search', host[b, :n], n, a, self.blank_index, self.beam_width,
                          int(self.log_input), ids, offs, len(ids), length, logp)
            strings.append([self._to_string(ids[:length.value])])
            offsets.append([torch.IntTensor(offs[:length.value].copy())])
            scores.append(logp.value)
        self.last_log_probs = scores
        return strings, offsets


class DeviceBeamCTCDecoder(GreedyDecoder):
    """CTC prefix beam search of a whole batch in one device launch, with optional n-gram LM shallow fusion (not in the
    reference).  Ranks prefixes by ``log(p_b + p_nb) + alpha * LM + beta * N`` (``csrc/ctc_beam.hip``); ``lm=None``
    ignores alpha and beta and gives the labels of ``BeamCTCDecoder``.  The offsets are the frames at which the labels
    were appended on the best hypothesis's surviving lineage (``BeamCTCDecoder`` reports the frame a prefix was first
    proposed, even by a proposal that was later pruned; the two agree unless a prefix of the best path left the beam and
    came back).  ``decode(probs, sizes)`` takes device tensors; ``last_scores`` / ``last_ctc_log_probs`` hold the fused
    score (with the end-of-utterance LM terms) and the CTC log-probability of each best labelling.

    ``booster``: a ``codes.bias.PhraseBooster`` made for the same alphabet and blank; the search then runs
    ``ds2_ctc_beam_search_bias``, which adds ``weight * V(prefix)`` to the rank (include/ds2hip.h "phrase boosting"), and
    ``last_bias_counts`` holds, per utterance, the labels of the returned labelling that the phrases cover.  Without one
    nothing changes: the unbiased entry is called with the same arguments as ever.

    ``nbest`` (1..beam_width, default 1): with ``nbest > 1`` the search is ``ds2_ctc_beam_search_nbest`` and ``decode``
    returns, per utterance, up to ``nbest`` alternatives, best first: the valid entries of the final beam ranked by the
    fused score (include/ds2hip.h), so ``strings[b]`` and ``offsets[b]`` have ``max(1, count[b])`` entries and entry 0 is
    what ``nbest == 1`` returns (an impossible input keeps its one empty string).  ``last_scores``,
    ``last_ctc_log_probs`` and ``last_bias_counts`` stay the per-utterance values of entry 0; ``last_nbest_scores[b]``,
    ``last_nbest_ctc_log_probs[b]``, ``last_nbest_bias_counts[b]`` (with a booster) and ``last_nbest_posteriors[b]`` are
    lists as long as ``strings[b]``.  The posterior of alternative n is ``exp(s_n - logsumexp(s_0 .. s_{count-1}))`` over
    the returned float32 fused scores, in float64 (``nbest_posteriors``): a weight AMONG THE RETURNED ALTERNATIVES UNDER
    THE FUSED SCORE, not a calibrated probability -- the score holds alpha, beta and the boost, the list ends at
    ``nbest``, and nobody has measured its calibration on a trained model.  With ``nbest == 1`` nothing changes: the
    1-best entries are called with the arguments they get today and the ``last_nbest_*`` fields stay None.

    ``confidence``: as for ``GreedyDecoder``; ``last_confidences[b][n]`` covers every returned alternative (the rows of an
    N-best result are scored in one call, each against its own utterance).  The values are acoustic: no LM, no boost."""

    def __init__(self, label_encoder, blank_index=0, beam_width=16, lm=None, alpha=0.0, beta=0.0, log_input=False,
                 booster=None, nbest=1, confidence=None):
        self.log_input = bool(log_input)                       # (before the check of ``confidence``, which refuses it)
        super().__init__(label_encoder, blank_index, confidence)
        if not 1 <= beam_width <= 128:
            raise ValueError('beam_width must be in 1..128 for the device search, got %d' % beam_width)
        if not 1 <= nbest <= beam_width:
            raise ValueError('nbest must be in 1..beam_width = 1..%d, got %d' % (beam_width, nbest))
        self.nbest = int(nbest)
        self.last_nbest_scores = self.last_nbest_ctc_log_probs = None
        self.last_nbest_bias_counts = self.last_nbest_posteriors = None
        self.beam_width, self.log_input = int(beam_width), bool(log_input)
        self.lm, self.alpha, self.beta = lm, float(alpha), float(beta)
        classes = [str(c) for c in self.label_encoder.classes_.tolist()]
        if lm is not None and classes != lm.labels:
            raise ValueError('the LM was built for the alphabet %r, the decoder has %r' % (lm.labels, classes))
        self.space_id = classes.index(' ') if ' ' in classes else -1
        self.last_scores = None
        self.last_ctc_log_probs = None
        self.booster, self.last_bias_counts = booster, None
        if booster is not None:
            have = [str(c) for c in booster.label_encoder.classes_.tolist()]
            if have != classes or booster.blank_index != blank_index:
                raise ValueError('the phrase booster was built for the alphabet %r with blank %d, the decoder has %r with '
                                 'blank %d' % (have, booster.blank_index, classes, blank_index))

    def _search(self, probs, sizes_d):
        """The launch: the five device tensors of ``ops.ctc_beam_search`` and, with a booster, the bias counts (else None)."""
        probs = probs.detach().contiguous().float()
        if self.booster is None:
            return ops.ctc_beam_search(probs, sizes_d, self.beam_width, self.blank_index, self.log_input, self.lm,
                                       self.alpha, self.beta, self.space_id) + (None,)
        trans, final = self.booster.tables(probs.device)
        return ops.ctc_beam_search_bias(probs, sizes_d, self.beam_width, trans, final, self.booster.weight,
                                        self.blank_index, self.log_input, self.lm, self.alpha, self.beta, self.space_id)

    def _search_nbest(self, probs, sizes_d):
        """The N-best launch: the seven device tensors of ``ops.ctc_beam_search_nbest``."""
        probs = probs.detach().contiguous().float()
        trans, final, weight = None, None, 0.0
        if self.booster is not None:
            trans, final = self.booster.tables(probs.device)
            weight = self.booster.weight
        return ops.ctc_beam_search_nbest(probs, sizes_d, self.beam_width, self.nbest, self.blank_index, self.log_input,
                                         self.lm, self.alpha, self.beta, self.space_id, trans, final, weight)

    @staticmethod
    def nbest_posteriors(scores):
        """``exp(s_n - logsumexp(s))`` in float64 from the returned float32 fused scores; ``[0.0]`` for no alternatives.
        A weight among these alternatives under the fused score, not a calibrated probability."""
        s = np.asarray(scores, dtype=np.float32).astype(np.float64)
        if s.size == 0:
            return [0.0]
        m = s.max()
        if not np.isfinite(m):                                 # every score beyond float32: the formula has no value
            return [1.0 / s.size] * s.size
        e = np.exp(s - m)                                      # the same number with the maximum taken out first
        return (e / e.sum()).tolist()

    def _decode_nbest(self, probs, sizes_d):
        bsz = probs.shape[0]
        labels, offs, lens, score, ctc, bias, count = self._search_nbest(probs, sizes_d)
        conf = None
        if self.confidence is not None:
            conf = UnitConfidence.lists_from(self.confidence.score(probs, sizes_d, *nbest_rows(labels, offs, lens)))
        labels, offs, lens, count = labels.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy(), count.cpu().numpy()
        score, ctc = score.cpu().numpy(), ctc.cpu().numpy()
        keep = [max(1, int(c)) for c in count]
        self.last_scores = score[:, 0].tolist()
        self.last_ctc_log_probs = ctc[:, 0].tolist()
        self.last_nbest_scores = [score[b, :keep[b]].tolist() for b in range(bsz)]
        self.last_nbest_ctc_log_probs = [ctc[b, :keep[b]].tolist() for b in range(bsz)]
        self.last_nbest_posteriors = [self.nbest_posteriors(score[b, :int(count[b])]) for b in range(bsz)]
        if bias is not None:
            bias = bias.cpu().numpy()
            self.last_bias_counts = bias[:, 0].tolist()
            self.last_nbest_bias_counts = [bias[b, :keep[b]].tolist() for b in range(bsz)]
        if conf is not None:
            self.last_confidences = [[conf[b * self.nbest + n] for n in range(keep[b])] for b in range(bsz)]
        strings = [[self._to_string(labels[b, n, :lens[b, n]]) for n in range(keep[b])] for b in range(bsz)]
        offsets = [[torch.IntTensor(offs[b, n, :lens[b, n]].copy()) for n in range(keep[b])] for b in range(bsz)]
        return strings, offsets

    def decode(self, probs, sizes=None):
        if not probs.is_cuda:
            raise RuntimeError('DeviceBeamCTCDecoder.decode runs on device tensors only')
        sizes_d = _device_sizes(probs, sizes)
        if self.nbest > 1:
            return self._decode_nbest(probs, sizes_d)
        bsz = probs.shape[0]
        labels, offs, lens, score, ctc, bias = self._search(probs, sizes_d)
        if self.confidence is not None:
            scored = self.confidence.score(probs, sizes_d, labels, offs, lens)
            self.last_confidences = [[c] for c in UnitConfidence.lists_from(scored)]
        labels, offs, lens = labels.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
        if bias is not None:
            self.last_bias_counts = bias.cpu().tolist()
        self.last_scores = score.cpu().tolist()
        self.last_ctc_log_probs = ctc.cpu().tolist()
        strings = [[self._to_string(labels[b, :lens[b]])] for b in range(bsz)]
        offsets = [[torch.IntTensor(offs[b, :lens[b]].copy())] for b in range(bsz)]
        return strings, offsets

    def decode_labels(self, probs, sizes=None):
        """``decode`` without the trip to the host: (labels (B,T) int32, lens (B,) int32) on the device, row b holding the
        label ids of ``decode``'s string b -- the layout ``ops.edit_stats`` scores.  Nothing waits on the stream, and
        ``last_scores`` / ``last_ctc_log_probs`` are left as they were; with a booster ``last_bias_counts`` is set to the
        (B,) int32 DEVICE tensor of the counts."""
        if not probs.is_cuda:
            raise RuntimeError('DeviceBeamCTCDecoder.decode_labels runs on device tensors only')
        labels, _, lens, _, _, bias = self._search(probs, _device_sizes(probs, sizes))
        if bias is not None:
            self.last_bias_counts = bias
        return labels, lens

    def decode_labels_nbest(self, probs, sizes=None):
        """The alternatives without the trip to the host: (labels (B,N,T) int32, lens (B,N) int32, count (B,) int32) on
        the device, N = ``nbest``, rows [0, count[b]) of utterance b best first and the rest empty.  Viewed as (B*N, T) and
        (B*N,) that is the layout ``ops.edit_stats`` scores with ``ref_index = arange(B*N) // N``.  Nothing waits on the
        stream and no ``last_*`` field is touched."""
        if not probs.is_cuda:
            raise RuntimeError('DeviceBeamCTCDecoder.decode_labels_nbest runs on device tensors only')
        labels, _, lens, _, _, _, count = self._search_nbest(probs, _device_sizes(probs, sizes))
        return labels, lens, count
