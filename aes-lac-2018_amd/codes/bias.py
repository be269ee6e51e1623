"""Phrase boosting for the device CTC beam search (not in the reference): the other half of keyword search.  A list of
phrases -- names, products, jargon -- becomes a context graph, and ``ds2_ctc_beam_search_bias`` (``csrc/ctc_beam.hip``) adds
``w * V(prefix)`` to the rank of every prefix, ``V`` being the labels the phrases cover under the rule written out in
``include/ds2hip.h`` ("phrase boosting"): leftmost-longest, non-overlapping, a phrase begun but not finished keeping its
credit only while it can still be finished.

``ContextGraph`` builds the two tables of that rule's automaton on the host; ``PhraseBooster`` normalises the phrases as
``codes.search.KeywordSearcher`` does and keeps the tables on the device.  Whole-word matching is by putting spaces into
the phrase (' CAT ').  Out of scope: per-phrase weights, a biased ``ds2_ctc_beam_search_rows``, the host search."""
import numpy as np
import torch

from ds2hip import lib

from .preprocessing import OrderedLabelEncoder


def add_hotword_arguments(parser):
    """The three flags test.py and transcribe.py share."""
    parser.add_argument('--hotword', action='append', default=None, metavar='PHRASE',
                        help='a phrase to boost in --decoder beam (repeatable; runs the device search; put spaces into '
                             'the phrase for whole-word matching); default: none')
    parser.add_argument('--hotwords', default=None, metavar='FILE', help='a file of phrases to boost, one per line')
    parser.add_argument('--hotword-weight', default=2.0, type=float,
                        help='boost per matched character in nats (default: 2.0, a placeholder: nobody has measured which '
                             'weight helps on a trained model)')


def read_phrases(hotword_args, hotwords_file):
    """``--hotword`` phrases, then the non-empty lines of ``--hotwords FILE``, in that order."""
    phrases = list(hotword_args or [])
    if hotwords_file:
        with open(hotwords_file, encoding='utf8') as f:
            phrases += [line.rstrip('\r\n') for line in f if line.strip()]
    return phrases


def check_hotword_arguments(parser, args):
    """Refuse the flags with any decoder that cannot boost; True if a booster is wanted."""
    wanted = args.hotword is not None or args.hotwords is not None
    if wanted and args.decoder != 'beam':
        parser.error('--hotword / --hotwords need --decoder beam: only the beam search can boost phrases')
    return wanted


def booster_from_arguments(prog, args, to_label):
    """The ``PhraseBooster`` of the flags for the checkpoint's ``ToLabel``; a refused phrase ends the program by name."""
    try:
        return PhraseBooster(to_label, read_phrases(args.hotword, args.hotwords), weight=args.hotword_weight)
    except (ValueError, OSError) as e:
        raise SystemExit('%s: %s' % (prog, e))


class ContextGraph(object):
    """``ContextGraph(phrases, n_labels, blank)``: ``phrases`` a list of label lists (1..64 labels each, no blank, no
    duplicates, at most 1024; their trie has at most 32768 nodes, root included; ValueError otherwise).

    The nodes of the trie of all prefixes are numbered in BFS order, children in ascending label order, root = 0:
    ``paths[s]`` is node s's label tuple, ``depth[s]`` its length.  ``next[s][c]`` and ``gain[s][c]`` are the automaton of
    the scan (``gain = V(path(s) + c) - depth(s)``, in -63..+1), ``final[s] = F(path(s)) - depth(s) <= 0``; ``trans`` packs
    ``next | gain << 16`` as the kernel reads it, (S, n_labels) int32.  The blank column is never read and holds zeros."""

    def __init__(self, phrases, n_labels, blank=0):
        n_labels, blank = int(n_labels), int(blank)
        if not 0 <= blank < n_labels:
            raise ValueError('ContextGraph: the blank %d is outside the alphabet of %d labels' % (blank, n_labels))
        phrases = [tuple(int(c) for c in p) for p in phrases]
        if len(phrases) > lib.BIAS_MAX_PHRASES:
            raise ValueError('ContextGraph: %d phrases; the most is %d' % (len(phrases), lib.BIAS_MAX_PHRASES))
        for k, p in enumerate(phrases):
            if not 1 <= len(p) <= lib.BIAS_MAX_LEN:
                raise ValueError('ContextGraph: phrase %d has %d labels; a phrase has 1..%d' % (k, len(p), lib.BIAS_MAX_LEN))
            if any(c == blank or not 0 <= c < n_labels for c in p):
                raise ValueError('ContextGraph: phrase %d holds the blank or a label outside [0, %d)' % (k, n_labels))
        if len(set(phrases)) != len(phrases):
            raise ValueError('ContextGraph: the phrases hold a duplicate')
        prefixes = {()}
        for p in phrases:
            prefixes.update(p[:k] for k in range(1, len(p) + 1))
        if len(prefixes) > lib.BIAS_MAX_STATES:
            raise ValueError('ContextGraph: the phrases make %d states; the most is %d' % (len(prefixes), lib.BIAS_MAX_STATES))
        # BFS order with children in ascending label order = by (depth, the parent's number, label); level by level
        levels = {}
        for p in prefixes:
            levels.setdefault(len(p), []).append(p)
        ident, paths = {(): 0}, [()]
        for d in range(1, len(levels)):
            for p in sorted(levels[d], key=lambda p: (ident[p[:-1]], p[-1])):
                ident[p] = len(paths)
                paths.append(p)
        n = len(paths)
        self.n_labels, self.blank, self.phrases, self.paths = n_labels, blank, phrases, paths
        self.depth = np.asarray([len(p) for p in paths], np.int32)
        terminal = np.zeros(n, bool)
        terminal[[ident[p] for p in phrases]] = True
        nxt = np.zeros((n, n_labels), np.int32)
        gain = np.zeros((n, n_labels), np.int32)
        children = [[] for _ in range(n)]
        for s in range(1, n):
            children[ident[paths[s][:-1]]].append(s)
        # leaving node s by a label it has no child for: the scan of path(s) + c takes the steps it would take on path(s)
        # with its first stop overruled -- m_s labels in complete phrases, then pending at node t_s, a shorter one -- and
        # goes on from t_s with c; at the end of the utterance F(path(s)) = m_s + F(path(t_s)) in the same way
        m_of, t_of, f_of = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for s in range(n):
            d = int(self.depth[s])
            if s:
                q, a = ident[paths[s][:-1]], paths[s][-1]
                if terminal[s]:
                    m_of[s], t_of[s] = d, 0
                elif q == 0:
                    m_of[s], t_of[s] = 0, 0
                else:
                    tq = int(t_of[q])
                    t_of[s] = nxt[tq, a]
                    m_of[s] = m_of[q] + self.depth[tq] + gain[tq, a] - self.depth[t_of[s]]
                t = int(t_of[s])
                f_of[s] = m_of[s] + f_of[t]
                nxt[s] = nxt[t]
                gain[s] = m_of[s] + self.depth[t] + gain[t] - d
            for ch in children[s]:
                nxt[s, paths[ch][-1]] = ch
                gain[s, paths[ch][-1]] = 1
        nxt[:, blank] = 0
        gain[:, blank] = 0
        self.next, self.gain = nxt, gain
        self.final = (f_of - self.depth).astype(np.int32)
        self.trans = (nxt | (gain << 16)).astype(np.int32)
        self.n_states = n

    def walk(self, labels):
        """(V, F) of a label sequence by the tables: the sum of the gains, and that plus ``final`` of the state reached."""
        s = v = 0
        for c in labels:
            v += int(self.gain[s, c])
            s = int(self.next[s, c])
        return v, v + int(self.final[s])


class PhraseBooster(object):
    """``PhraseBooster(label_encoder, phrases, weight=2.0)``: ``label_encoder`` as for ``KeywordSearcher`` (the
    checkpoint's ``ToLabel``, whose normalisation is applied to the phrases, or a label encoder / list / string of the
    alphabet).  A phrase that normalises to nothing, to more than 64 labels, to something that holds the blank symbol, or
    to the same labels as an earlier phrase is refused by name (ValueError), and so are more than 1024 phrases or a trie of
    more than 32768 states.  ``weight``: nats per matched label; 2.0 is a placeholder that no trained model has tuned.
    ``keywords`` are the phrases as normalised, ``labels`` their label lists, ``graph`` the ``ContextGraph``;
    ``tables(device)`` the (trans, final) int32 tensors on that device, uploaded once."""

    def __init__(self, label_encoder, phrases, weight=2.0, blank_index=0):
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
        self.blank_index, self.weight = int(blank_index), float(weight)
        if not np.isfinite(np.float32(self.weight)):
            raise ValueError('PhraseBooster: the weight %r is not a finite float32' % (weight,))
        phrases = list(phrases)
        if not phrases:
            raise ValueError('PhraseBooster: no phrases')
        if len(phrases) > lib.BIAS_MAX_PHRASES:
            raise ValueError('PhraseBooster: %d phrases; the most is %d' % (len(phrases), lib.BIAS_MAX_PHRASES))
        self.keywords, self.labels, seen = [], [], {}
        for phrase in phrases:
            ids = [int(v) for v in np.asarray(to_label(phrase)).reshape(-1)]
            text = ''.join(str(c) for c in self.label_encoder.inverse_transform(ids)) if ids else ''
            if not ids:
                raise ValueError('PhraseBooster: the phrase %r normalises to nothing in this alphabet' % (phrase,))
            if len(ids) > lib.BIAS_MAX_LEN:
                raise ValueError('PhraseBooster: the phrase %r normalises to %d labels; the longest phrase has %d'
                                 % (phrase, len(ids), lib.BIAS_MAX_LEN))
            if self.blank_index in ids:
                raise ValueError('PhraseBooster: the phrase %r holds the blank symbol' % (phrase,))
            if tuple(ids) in seen:
                raise ValueError('PhraseBooster: the phrase %r normalises to %r, as the phrase %r does'
                                 % (phrase, text, seen[tuple(ids)]))
            seen[tuple(ids)] = phrase
            self.keywords.append(text)
            self.labels.append(ids)
        n_states = len({tuple(ids[:k]) for ids in self.labels for k in range(len(ids) + 1)})
        if n_states > lib.BIAS_MAX_STATES:
            raise ValueError('PhraseBooster: the phrases make %d states; the most is %d' % (n_states, lib.BIAS_MAX_STATES))
        self.graph = ContextGraph(self.labels, len(self.label_encoder.classes_), self.blank_index)
        self._dev = {}

    def tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.graph.trans).to(device), torch.from_numpy(self.graph.final).to(device))
        return self._dev[key]
