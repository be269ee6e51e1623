"""N-gram language model for the device CTC beam search (``DeviceBeamCTCDecoder``, ``csrc/ctc_beam.hip``).

``NGramLM.from_arpa(path, labels, unit='word'|'char')`` reads a standard ARPA file (log10 values; what ``lmplz`` or
``tools/make_lm.py`` writes), keeps the n-grams the alphabet can spell, and builds the two open-addressing tables the
kernel probes:

* the n-gram table: key = ``seq_hash(token ids)``, value = ``(ln p, ln backoff)`` as float32;
* in word mode, the word table: key = ``seq_hash(alphabet indices of the word's characters)``, value = word id.

Both tables are arrays of 16-byte entries ``{uint64 key; 4 bytes; 4 bytes}`` with a power-of-two capacity of at least
twice the entry count, probed linearly from ``key & (cap - 1)``; key 0 marks an empty slot.  ``seq_hash`` below and
``csrc/ds2_hash.h`` (what the kernel uses) are the same function (tests/test_lm_cpu.py pins both to fixed vectors).
A table entry is identified by its 64-bit hash alone: two distinct kept n-grams with one hash are refused when the table
is built; a queried n-gram that is absent but shares a present one's hash (probability ~ n / 2**64) reads that value.

Token ids: in char mode a label's id is its alphabet index and ``<s>``, ``</s>``, ``<unk>`` get ``A``, ``A+1``,
``A+2``; the ARPA token ``space_token`` (default ``<space>``) is the space label.  In word mode ids are assigned in
order of the unigram section.  An out-of-vocabulary token scores ``<unk>``'s unigram if the LM has one, else
``oov_logp``, without backoff weights, and enters the history as ``<unk>`` (or as an id no n-gram contains).
"""
import logging
import math
import re

import numpy as np

LN10 = math.log(10.0)
MAX_ORDER = 8
M64 = (1 << 64) - 1
HASH_SEED = 0x243F6A8885A308D3
HASH_STEP = 0x9E3779B97F4A7C15

log = logging.getLogger(__name__)


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hash_step(h, x):
    """One step of the rolling hash: ``mix64(h + HASH_STEP + (uint32)x)`` (``ds2_hash_step`` on the device)."""
    return _mix64((h + HASH_STEP + (int(x) & 0xFFFFFFFF)) & M64)


def seq_hash(ids):
    """64-bit hash of a sequence of int ids; never 0 (0 marks an empty table slot)."""
    h = HASH_SEED
    for x in ids:
        h = hash_step(h, x)
    return h or 1


def build_table(keys, lo, hi):
    """Open-addressing table of 16-byte entries (uint64 key, 4-byte lo, 4-byte hi) -> (cap, 2) uint64 array.
    ``lo``/``hi`` are float32 or int32 numpy arrays; raises on a duplicate key (a 64-bit collision)."""
    n = len(keys)
    cap = 2
    while cap < 2 * n:
        cap *= 2
    table = np.zeros((cap, 2), dtype=np.uint64)
    lo_bits = np.ascontiguousarray(lo).view(np.uint32).astype(np.uint64)
    hi_bits = np.ascontiguousarray(hi).view(np.uint32).astype(np.uint64)
    mask = cap - 1
    for k, key in enumerate(keys):
        i = key & mask
        while table[i, 0] != 0:
            if int(table[i, 0]) == key:
                raise ValueError('NGramLM: two table entries share the 64-bit hash %#x' % key)
            i = (i + 1) & mask
        table[i, 0] = key
        table[i, 1] = lo_bits[k] | (hi_bits[k] << np.uint64(32))
    return table


def table_lookup(table, key):
    """Index of ``key`` in a table from build_table, or -1."""
    mask = len(table) - 1
    i = key & mask
    for _ in range(len(table)):
        have = int(table[i, 0])
        if have == key:
            return i
        if have == 0:
            return -1
        i = (i + 1) & mask
    return -1


def parse_arpa(path):
    """-> {n: [(tokens tuple, log10 p, log10 backoff or None)]}; raises ValueError on a malformed file."""
    counts, grams, section = {}, {}, None
    with open(path, 'r', encoding='utf8') as f:
        lines = f.read().splitlines()
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if not line:
            continue
        if line == '\\data\\':
            section = 'data'
            continue
        if line == '\\end\\':
            section = 'end'
            break
        m = re.match(r'^\\(\d+)-grams:$', line)
        if m:
            section = int(m.group(1))
            if section not in counts:
                raise ValueError('%s:%d: section \\%d-grams: is not announced in \\data\\' % (path, no, section))
            grams[section] = []
            continue
        if section == 'data':
            m = re.match(r'^ngram\s+(\d+)\s*=\s*(\d+)$', line)
            if not m:
                raise ValueError('%s:%d: malformed \\data\\ line: %r' % (path, no, line))
            counts[int(m.group(1))] = int(m.group(2))
        elif isinstance(section, int):
            parts = line.split()
            n = section
            if len(parts) not in (n + 1, n + 2):
                raise ValueError('%s:%d: a %d-gram line needs %d or %d fields: %r' % (path, no, n, n + 1, n + 2, line))
            try:
                p = float(parts[0])
                bo = float(parts[n + 1]) if len(parts) == n + 2 else None
            except ValueError:
                raise ValueError('%s:%d: malformed number in %r' % (path, no, line))
            grams[n].append((tuple(parts[1:n + 1]), p, bo))
        elif section is None:
            continue                                    # text before \data\ is allowed (lmplz writes none, SRILM a blank)
        else:
            raise ValueError('%s:%d: unexpected line %r' % (path, no, line))
    if not counts:
        raise ValueError('%s: no \\data\\ section' % path)
    if section != 'end':
        raise ValueError('%s: missing \\end\\' % path)
    for n, c in counts.items():
        if len(grams.get(n, ())) != c:
            raise ValueError('%s: \\data\\ announces %d %d-grams, the file has %d' % (path, c, n, len(grams.get(n, ()))))
    if sorted(counts) != list(range(1, len(counts) + 1)):
        raise ValueError('%s: n-gram orders %s are not 1..N' % (path, sorted(counts)))
    return grams


class NGramLM(object):
    """A back-off n-gram LM over the alphabet's tokens.  ``log_prob`` is the pure-Python scorer with the same rule the
    kernel applies; ``ngram_table`` / ``word_table`` are the numpy tables, ``to(device)`` uploads them once."""

    def __init__(self, labels, unit, order, ngrams, vocab, oov_logp, space_token='<space>'):
        self.labels = list(labels)
        self.unit = unit
        self.order = order
        self.ngrams = ngrams                      # {tuple(ids): (ln p, ln bo)}, float32-rounded values
        self.vocab = vocab                        # token string -> id
        self.space_token = space_token
        self.bos_id = vocab.get('<s>', -1)
        self.eos_id = vocab.get('</s>', -1)
        self.unk_id = vocab.get('<unk>', -1)
        self.hist_unk_id = self.unk_id if self.unk_id >= 0 else len(vocab) + len(self.labels) + 3
        unk = ngrams.get((self.unk_id,)) if self.unk_id >= 0 else None
        self.oov_logp = float(np.float32(unk[0] if unk is not None else oov_logp))
        self._device_tables = {}
        keys = list(ngrams)
        self.ngram_table = build_table([seq_hash(k) for k in keys],
                                       np.asarray([ngrams[k][0] for k in keys], dtype=np.float32),
                                       np.asarray([ngrams[k][1] for k in keys], dtype=np.float32))
        self.word_table = None
        if unit == 'word':
            idx = {c: i for i, c in enumerate(self.labels)}
            words = [w for w in vocab if w not in ('<s>', '</s>', '<unk>')]
            self.word_table = build_table([seq_hash([idx[c] for c in w]) for w in words],
                                          np.asarray([vocab[w] for w in words], dtype=np.int32),
                                          np.zeros(len(words), dtype=np.int32))
        if self.bos_id < 0 or self.eos_id < 0:
            raise ValueError('NGramLM: the LM has no <s> or no </s> unigram')

    @classmethod
    def from_arpa(cls, path, labels, unit='word', space_token='<space>', oov_logp=-10.0, blank_index=0):
        """``labels``: the alphabet (list of single characters, blank included, upper-case for data/labels.*.json)."""
        if unit not in ('word', 'char'):
            raise ValueError("NGramLM: unit must be 'word' or 'char', got %r" % (unit,))
        labels = list(labels)
        grams = parse_arpa(path)
        order = max(grams)
        if order > MAX_ORDER:
            raise ValueError('NGramLM: order %d > %d is not supported by the device search' % (order, MAX_ORDER))
        space = ' ' if ' ' in labels else None
        spellable = set(c for i, c in enumerate(labels) if i != blank_index and c != space)
        specials = ('<s>', '</s>', '<unk>')
        vocab = {}
        if unit == 'char':
            for i, c in enumerate(labels):
                if c in spellable or c == space:
                    vocab[space_token if c == space else c] = i
            for k, s in enumerate(specials):
                vocab[s] = len(labels) + k

            def tok_id(t):
                if t in specials or t == space_token:
                    return vocab.get(t)
                if len(t) != 1:
                    raise ValueError('NGramLM: unit=char needs single-character tokens; %r is not one (the space '
                                     'label is written %r)' % (t, space_token))
                c = t.upper() if t.upper() in spellable else t
                return vocab[c] if c in spellable else None
        else:
            for toks, _, _ in grams[1]:
                t = toks[0]
                w = t if t in specials else t.upper()
                if w in specials or (w and all(c in spellable for c in w)):
                    vocab.setdefault(w, len(vocab))

            def tok_id(t):
                return vocab.get(t if t in specials else t.upper())

        ngrams, dropped = {}, 0
        for n in sorted(grams):
            for toks, p, bo in grams[n]:
                ids = [tok_id(t) for t in toks]
                if any(i is None for i in ids):
                    dropped += 1
                    continue
                ngrams[tuple(ids)] = (float(np.float32(p * LN10)), float(np.float32((bo or 0.0) * LN10)))
        if unit == 'char':
            # ids of labels the unigram section does not list stay out of the table: they score as OOV
            vocab = {t: i for t, i in vocab.items() if (i,) in ngrams}
        if dropped:
            log.warning('NGramLM: dropped %d n-grams with tokens the alphabet cannot spell (%s)', dropped, path)
        lm = cls(labels, unit, order, ngrams, vocab, oov_logp, space_token)
        lm.dropped = dropped
        return lm

    # ------------------------------------------------------------------ pure-Python scorer (the kernel's rule)
    def token_id(self, token):
        """Token string (case-folded; ``space_token`` or ' ' for the space in char mode) -> id, or None if OOV."""
        if self.unit == 'char' and token == ' ':
            token = self.space_token
        if token not in ('<s>', '</s>', '<unk>', self.space_token):
            token = token.upper()
        return self.vocab.get(token)

    def log_prob_ids(self, hist, w):
        """ln P(w | hist) by ARPA backoff; ``hist`` = token ids, oldest first (only the last order-1 are used);
        ``w`` = a token id or None (OOV).  Returns (ln p, id w enters the history as)."""
        if w is None or (w,) not in self.ngrams:
            return self.oov_logp, self.hist_unk_id
        hist = list(hist)[max(0, len(hist) - (self.order - 1)):] if self.order > 1 else []
        acc = 0.0
        for k in range(len(hist), 0, -1):
            h = tuple(hist[len(hist) - k:])
            e = self.ngrams.get(h + (w,))
            if e is not None:
                return acc + e[0], w
            b = self.ngrams.get(h)
            if b is not None:
                acc += b[1]
        return acc + self.ngrams[(w,)][0], w

    def log_prob(self, history, token):
        """ln P(token | history), history = token strings oldest first (start it with '<s>')."""
        return self.log_prob_ids([self.token_id(t) if self.token_id(t) is not None else self.hist_unk_id
                                  for t in history], self.token_id(token))[0]

    def word_id(self, label_ids):
        """Word id of a word spelled by alphabet indices (word mode), or None."""
        i = table_lookup(self.word_table, seq_hash(label_ids))
        return None if i < 0 else int(self.word_table[i, 1] & np.uint64(0xFFFFFFFF))

    def to(self, device):
        """Upload the tables once per device -> dict of device tensors (the kernel's view of them)."""
        import torch
        key = str(device)
        if key not in self._device_tables:
            up = {'ngram': torch.from_numpy(self.ngram_table.view(np.int64).copy()).to(device)}
            if self.word_table is not None:
                up['word'] = torch.from_numpy(self.word_table.view(np.int64).copy()).to(device)
            self._device_tables[key] = up
        return self._device_tables[key]
