#!/usr/bin/env python
"""Build an ARPA n-gram LM from training transcripts, for ``test.py --decoder beam --lm-path``.

    python tools/make_lm.py --order 3 --unit word --labels data/labels.en.json \\
        --data-dir DATA --manifest DATA/train_manifest.csv [--text more.txt] -o lm.arpa

Transcripts (the transcript files a manifest names, and/or plain text files with one transcript per line) go through
the project's ``ToLabel`` normalisation, so the LM spells words exactly as the alphabet does.  ``--unit char`` models
characters (the space is written ``<space>``), ``--unit word`` models words.  Sentences are padded with ``<s>`` /
``</s>``.  Probabilities use absolute discounting with back-off: a seen n-gram ``(h, w)`` gets ``(c(h w) - D) / c(h)``,
an unseen one ``bo(h) * P(w | h[1:])`` with ``bo(h)`` chosen so that every context's distribution over the vocabulary
(every token but ``<s>``) sums to 1; unigrams are maximum-likelihood.  An ARPA file from ``lmplz`` works equally.
"""
import argparse
import math
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aes-lac-2018_amd'))


def read_transcripts(labels, manifests=(), data_dir='', texts=()):
    """-> list of normalised transcripts (strings over the alphabet, spaces collapsed)."""
    from codes.transforms import ToLabel
    to_label = ToLabel(labels)
    classes = to_label.label_encoder.classes_
    raw = []
    for m in manifests:
        with open(m) as f:
            for line in f:
                if line.strip():
                    path = os.path.join(data_dir, line.strip().split(',')[1])
                    with open(path, encoding='utf8') as g:
                        raw.append(g.readline().strip())
    for t in texts:
        with open(t, encoding='utf8') as f:
            raw.extend(line.strip() for line in f if line.strip())
    out = []
    for r in raw:
        ids = to_label(r).reshape(-1)
        s = ' '.join(''.join(classes[ids]).split())
        if s:
            out.append(s)
    return out


def sentences(transcripts, unit):
    for s in transcripts:
        yield ['<s>'] + (s.split() if unit == 'word' else ['<space>' if c == ' ' else c for c in s]) + ['</s>']


def build_lm(sents, order, discount=None):
    """-> (grams {k: {tuple: log10 p}}, backoffs {tuple: log10 bo}) of an absolute-discounting back-off LM."""
    counts = [None] + [defaultdict(int) for _ in range(order)]
    for toks in sents:
        for k in range(1, order + 1):
            for i in range(len(toks) - k + 1):
                g = tuple(toks[i:i + k])
                if k == 1 and g == ('<s>',):
                    continue
                if k > 1 and '</s>' in g[:-1]:
                    continue
                counts[k][g] += 1
    counts[1][('<s>',)] = 0
    vocab = sorted(w for (w,) in counts[1] if w != '<s>')
    total = sum(c for g, c in counts[1].items() if g != ('<s>',))
    prob = {(w,): counts[1][(w,)] / total for w in vocab}
    follow = defaultdict(dict)                       # context -> {w: count}
    for k in range(2, order + 1):
        for g, c in counts[k].items():
            follow[g[:-1]][g[-1]] = c
    bo = {}

    def p(h, w):                                     # P(w | h) from the orders built so far
        e = prob.get(h + (w,))
        if e is not None:
            return e
        if not h:
            return 0.0
        return bo.get(h, 1.0) * p(h[1:], w)

    for k in range(2, order + 1):
        n1 = sum(1 for c in counts[k].values() if c == 1)
        n2 = sum(1 for c in counts[k].values() if c == 2)
        d = discount if discount is not None else min(0.9, max(0.1, n1 / (n1 + 2.0 * n2) if n1 + n2 else 0.5))
        for h in [h for h in follow if len(h) == k - 1]:
            seen = follow[h]
            ch = float(sum(seen.values()))
            lower = sum(p(h[1:], w) for w in seen)
            free = 1.0 - lower
            dd = d if (len(seen) < len(vocab) and free > 1e-9) else 0.0
            for w, c in seen.items():
                prob[h + (w,)] = (c - dd) / ch
            if dd > 0:
                bo[h] = (dd * len(seen) / ch) / free
    grams = {k: {} for k in range(1, order + 1)}
    for g, v in prob.items():
        grams[len(g)][g] = math.log10(v)
    grams[1][('<s>',)] = -99.0
    for k in range(2, order + 1):                   # contexts that are not themselves listed n-grams (none expected)
        for h in follow:
            if len(h) == k - 1 and h not in grams[k - 1] and h != ('<s>',):
                raise RuntimeError('context %r has no n-gram entry' % (h,))
    return grams, {h: math.log10(b) for h, b in bo.items()}


def write_arpa(path, grams, backoffs):
    order = max(grams)
    with open(path, 'w', encoding='utf8') as f:
        f.write('\\data\\\n')
        for k in range(1, order + 1):
            f.write('ngram %d=%d\n' % (k, len(grams[k])))
        for k in range(1, order + 1):
            f.write('\n\\%d-grams:\n' % k)
            for g in sorted(grams[k]):
                line = '%.7f\t%s' % (grams[k][g], ' '.join(g))
                if k < order and g in backoffs:
                    line += '\t%.7f' % backoffs[g]
                f.write(line + '\n')
        f.write('\n\\end\\\n')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--order', type=int, default=3)
    ap.add_argument('--unit', choices=['word', 'char'], default='word')
    ap.add_argument('--labels', default=os.path.join(ROOT, 'data', 'labels.en.json'))
    ap.add_argument('--data-dir', default='')
    ap.add_argument('--manifest', action='append', default=[], help='manifest CSV (audio,transcript,duration); repeatable')
    ap.add_argument('--text', action='append', default=[], help='text file, one transcript per line; repeatable')
    ap.add_argument('--discount', type=float, default=None, help='absolute discount D (default: n1 / (n1 + 2 n2))')
    ap.add_argument('-o', '--output', required=True)
    args = ap.parse_args(argv)
    if not 1 <= args.order <= 8:
        ap.error('--order must be in 1..8 (the device search supports up to 8)')
    trans = read_transcripts(args.labels, args.manifest, args.data_dir, args.text)
    if not trans:
        ap.error('no transcripts: give --manifest and/or --text')
    grams, bo = build_lm(sentences(trans, args.unit), args.order, args.discount)
    write_arpa(args.output, grams, bo)
    print('%s: %d-gram %s LM from %d transcripts (%s n-grams)' % (
        args.output, args.order, args.unit, len(trans), '/'.join(str(len(grams[k])) for k in sorted(grams))))


if __name__ == '__main__':
    main()
