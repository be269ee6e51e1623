"""Keyword search: where in a batch of utterances was each of a list of phrases said (not in the reference).  The decoders
write what the model would have written, so a search of their text misses every occurrence whose top-1 is off by a
character (greedy) or that the language model talks the beam out of; ``ds2_ctc_keyword_search`` (``csrc/ctc_keyword.hip``)
reads the frame posteriors instead: for every utterance and keyword, the spans whose best CTC reading of the keyword stays
within ``min_score`` of the model's own best path.  The host part below normalises the phrases and names the hits.

Out of scope: whole-word matching (put the space label into the phrase: ' CAT '), wildcard or fuzzy phrases, keywords of
more than 64 labels, occurrences that cross the border between two utterances, anything that changes the decoders."""
import numpy as np
import torch

from ds2hip import lib, ops

from .preprocessing import OrderedLabelEncoder


class KeywordSearcher(object):
    """``KeywordSearcher(label_encoder, phrases)``: ``label_encoder`` is the checkpoint's ``ToLabel`` (its normalisation
    -- upper-casing, accent folding, dropping characters outside the alphabet -- is applied to the phrases as it is to
    transcripts), or a label encoder / list / string of the alphabet, for which a default ``ToLabel`` is made.  A phrase that
    normalises to nothing, to more than 64 labels, to something that holds the blank symbol, or to the same labels as an
    earlier phrase is refused by name (ValueError).  ``min_score[k] = min_score_per_char * L_k`` in float64 on the host.

    ``search(probs (B,T,A) on the device, sizes)`` takes the model's PROBABILITIES, takes their log on the device once and
    makes one ``ds2_ctc_keyword_search`` call for all keywords.  It returns ``(found, n_hits)``: ``found[b]`` is the list of
    ``{keyword, utterance, start_frame, end_frame, score, score_per_char}`` of utterance b, by keyword and then by end
    frame (frames inclusive, model output steps); ``n_hits`` the (B,K) numpy array of TRUE counts, which exceed
    ``max_hits`` where hits were left out."""

    def __init__(self, label_encoder, phrases, min_score_per_char=-1.0, max_hits=4, blank_index=0):
        from .transforms import ToLabel
        if callable(label_encoder) and hasattr(label_encoder, 'label_encoder'):
            to_label = label_encoder
        else:
            if isinstance(label_encoder, str):
                label_encoder = list(label_encoder)
            if isinstance(label_encoder, (set, list)):
                label_encoder = OrderedLabelEncoder().fit(label_encoder)
            to_label = ToLabel(labels=label_encoder.classes_.tolist())
        self.label_encoder = to_label.label_encoder
        self.blank_index, self.max_hits = int(blank_index), int(max_hits)
        self.min_score_per_char = float(min_score_per_char)
        if not 1 <= self.max_hits <= 64:
            raise ValueError('KeywordSearcher: max_hits = %r is outside 1..64' % (max_hits,))
        phrases = list(phrases)
        if not phrases:
            raise ValueError('KeywordSearcher: no phrases')
        self.keywords, self.labels, seen = [], [], {}
        for phrase in phrases:
            ids = [int(v) for v in np.asarray(to_label(phrase)).reshape(-1)]
            text = ''.join(str(c) for c in self.label_encoder.inverse_transform(ids)) if ids else ''
            if not ids:
                raise ValueError('KeywordSearcher: the phrase %r normalises to nothing in this alphabet' % (phrase,))
            if len(ids) > lib.KWS_MAX_LEN:
                raise ValueError('KeywordSearcher: the phrase %r normalises to %d labels; the longest keyword has %d'
                                 % (phrase, len(ids), lib.KWS_MAX_LEN))
            if self.blank_index in ids:
                raise ValueError('KeywordSearcher: the phrase %r holds the blank symbol' % (phrase,))
            if tuple(ids) in seen:
                raise ValueError('KeywordSearcher: the phrase %r normalises to %r, as the phrase %r does'
                                 % (phrase, text, seen[tuple(ids)]))
            seen[tuple(ids)] = phrase
            self.keywords.append(text)
            self.labels.append(ids)
        lens = np.asarray([len(v) for v in self.labels], np.int32)
        self._lens = torch.from_numpy(lens)
        self._offsets = torch.from_numpy((np.cumsum(lens) - lens).astype(np.int32))
        self._flat = torch.from_numpy(np.concatenate(self.labels).astype(np.int32))
        self.min_score = np.float64(self.min_score_per_char) * lens.astype(np.float64)
        self._dev = {}

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(x.to(device) for x in (self._flat, self._offsets, self._lens,
                                                          torch.from_numpy(self.min_score)))
        return self._dev[key]

    def search_device(self, probs, sizes):
        """The launch alone: (hits, hit_score, n_hits) as device tensors (``ops.keyword_search``); nothing waits."""
        if not probs.is_cuda:
            raise RuntimeError('KeywordSearcher.search runs on device tensors only')
        flat, offsets, lens, min_score = self._tables(probs.device)
        logp = torch.log(probs.detach().contiguous().float())
        sizes = torch.as_tensor(sizes).to(probs.device, torch.int32).reshape(-1)
        return ops.keyword_search(logp, sizes, flat, offsets, lens, min_score, self.max_hits, self.blank_index)

    def records(self, hits, hit_score, n_hits):
        """The three outputs as numpy arrays -> found[b] (see the class)."""
        found = []
        for b in range(hits.shape[0]):
            rows = []
            for k, text in enumerate(self.keywords):
                for i in range(min(int(n_hits[b, k]), self.max_hits)):
                    score = float(hit_score[b, k, i])
                    rows.append({'keyword': text, 'utterance': b, 'start_frame': int(hits[b, k, i, 0]),
                                 'end_frame': int(hits[b, k, i, 1]), 'score': score,
                                 'score_per_char': score / len(self.labels[k])})
            found.append(rows)
        return found

    def search(self, probs, sizes):
        hits, hit_score, n_hits = (x.cpu().numpy() for x in self.search_device(probs, sizes))
        return self.records(hits, hit_score, n_hits), n_hits
