"""CPU checks of the n-gram LM used by the device beam search (codes/lm.py), of tools/make_lm.py, and of the new ABI
entry points' revision: ARPA parsing, backoff, case folding, refusals, hash tables, host/device hash agreement."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]
LN10 = math.log(10.0)

ARPA = """\\data\\
ngram 1=7
ngram 2=4
ngram 3=2

\\1-grams:
-1.0\t<unk>
-99\t<s>\t-0.5
-0.7\t</s>
-0.6\tthe\t-0.3
-0.8\tcat\t-0.2
-0.9\tdog
-1.1\tcafé\t-0.4

\\2-grams:
-0.2\t<s> the\t-0.1
-0.3\tthe cat\t-0.25
-0.4\tcat </s>
-0.5\tthe café

\\3-grams:
-0.05\t<s> the cat
-0.6\tthe cat </s>

\\end\\
"""


def _f32(x):
    return float(np.float32(x))


@pytest.fixture
def arpa(tmp_path):
    p = tmp_path / 'tiny.arpa'
    p.write_text(ARPA, encoding='utf8')
    return str(p)


def test_arpa_parse_backoff_unk_and_case_folding(arpa):
    from codes.lm import NGramLM
    lm = NGramLM.from_arpa(arpa, LABELS, unit='word', oov_logp=-7.0)
    assert lm.order == 3 and lm.dropped == 2            # 'café' and 'the café' cannot be spelled
    assert lm.token_id('the') == lm.token_id('THE') and lm.token_id('CAFÉ') is None
    # present trigram
    assert lm.log_prob(['<s>', 'the'], 'cat') == pytest.approx(_f32(-0.05 * LN10), abs=1e-12)
    # missing trigram (the, cat, dog): bo(the cat) + P(dog | cat) = bo(the cat) + bo(cat) + P(dog)
    want = _f32(-0.25 * LN10) + _f32(-0.2 * LN10) + _f32(-0.9 * LN10)
    assert lm.log_prob(['the', 'cat'], 'dog') == pytest.approx(want, abs=1e-12)
    # missing context (dog has no backoff: counts 0), then the bigram
    assert lm.log_prob(['dog', 'cat'], '</s>') == pytest.approx(_f32(-0.4 * LN10), abs=1e-12)
    # OOV words score <unk>'s unigram, without backoff weights
    assert lm.log_prob(['<s>', 'the'], 'zebra') == pytest.approx(_f32(-1.0 * LN10), abs=1e-12)
    assert lm.oov_logp == _f32(-1.0 * LN10)


def test_oov_without_unk_uses_oov_logp(tmp_path):
    from codes.lm import NGramLM
    p = tmp_path / 'nounk.arpa'
    p.write_text(ARPA.replace('ngram 1=7', 'ngram 1=6').replace('-1.0\t<unk>\n', ''), encoding='utf8')
    lm = NGramLM.from_arpa(str(p), LABELS, unit='word', oov_logp=-7.0)
    assert lm.unk_id == -1 and lm.log_prob(['<s>'], 'zebra') == _f32(-7.0)


def test_char_mode_tokens_and_space(tmp_path):
    from codes.lm import NGramLM
    p = tmp_path / 'c.arpa'
    p.write_text('\\data\\\nngram 1=5\nngram 2=2\n\n\\1-grams:\n-99\t<s>\t-0.1\n-0.5\t</s>\n-0.4\ta\t-0.2\n'
                 '-0.6\t<space>\n-0.7\t#\n\n\\2-grams:\n-0.1\t<s> a\n-0.3\ta <space>\n\n\\end\\\n')
    lm = NGramLM.from_arpa(str(p), LABELS, unit='char')
    assert lm.dropped == 1                              # '#' is not in the alphabet
    assert lm.token_id('A') == LABELS.index('A') and lm.token_id(' ') == 1
    assert lm.log_prob(['<s>', 'a'], ' ') == pytest.approx(_f32(-0.3 * LN10), abs=1e-12)
    assert lm.log_prob(['<s>', ' '], 'a') == pytest.approx(_f32(-0.4 * LN10), abs=1e-12)


@pytest.mark.parametrize('text, unit, kw, msg', [
    (ARPA, 'phone', {}, 'unit must be'),
    (ARPA, 'char', {}, 'single-character tokens'),
    (ARPA.replace('ngram 2=4', 'ngram 2=5'), 'word', {}, 'announces'),
    (ARPA.replace('-0.9\tdog', 'x.9\tdog'), 'word', {}, 'malformed number'),
    (ARPA.replace('\\end\\', ''), 'word', {}, 'missing \\\\end'),
])
def test_refusals(tmp_path, text, unit, kw, msg):
    from codes.lm import NGramLM
    p = tmp_path / 'bad.arpa'
    p.write_text(text, encoding='utf8')
    with pytest.raises(ValueError, match=msg):
        NGramLM.from_arpa(str(p), LABELS, unit=unit, **kw)


def test_order_above_8_is_refused(tmp_path):
    from codes.lm import NGramLM
    head = '\\data\\\n' + ''.join('ngram %d=1\n' % k for k in range(1, 10))
    body = ''.join('\n\\%d-grams:\n-0.1\t%s\n' % (k, ' '.join(['a'] * k)) for k in range(1, 10))
    p = tmp_path / 'o9.arpa'
    p.write_text(head + body + '\n\\end\\\n')
    with pytest.raises(ValueError, match='order 9'):
        NGramLM.from_arpa(str(p), LABELS, unit='char')


def _corpus(tmp_path):
    rng = np.random.default_rng(1)
    words = ['hello', 'world', 'speech', 'test', 'amd', 'gpu', "don't", 'beam', 'the', 'a']
    p = tmp_path / 'corpus.txt'
    p.write_text('\n'.join(' '.join(rng.choice(words, size=rng.integers(1, 7))) for _ in range(120)) + '\n')
    return str(p)


def _make_lm(tmp_path, order, unit):
    out = str(tmp_path / ('%s%d.arpa' % (unit, order)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_lm.py'), '--order', str(order), '--unit', unit,
                        '--text', _corpus(tmp_path), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize('order, unit', [(4, 'char'), (3, 'word')])
def test_make_lm_distributions_sum_to_one(tmp_path, order, unit):
    from codes.lm import NGramLM
    lm = NGramLM.from_arpa(_make_lm(tmp_path, order, unit), LABELS, unit=unit)
    assert lm.dropped == 0 and lm.order == order
    vocab = [i for t, i in lm.vocab.items() if t != '<s>']
    contexts = [g for g in lm.ngrams if len(g) < order and g[-1] != lm.eos_id]
    assert len(contexts) > 20
    for h in contexts:
        s = sum(math.exp(lm.log_prob_ids(list(h), w)[0]) for w in vocab)
        assert abs(s - 1.0) < 1e-4, (h, s)


def test_tables_hold_every_ngram_and_no_other(tmp_path):
    from codes.lm import NGramLM, seq_hash, table_lookup
    lm = NGramLM.from_arpa(_make_lm(tmp_path, 3, 'word'), LABELS, unit='word')
    tab = lm.ngram_table
    assert (len(tab) & (len(tab) - 1)) == 0 and len(tab) >= 2 * len(lm.ngrams)
    for g, (p, bo) in lm.ngrams.items():
        i = table_lookup(tab, seq_hash(g))
        assert i >= 0
        payload = int(tab[i, 1])
        lo = np.array([payload & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]
        hi = np.array([payload >> 32], dtype=np.uint32).view(np.float32)[0]
        assert float(lo) == p and float(hi) == bo
    ids = sorted(set(i for g in lm.ngrams for i in g))
    absent = [(a, b, c) for a in ids for b in ids for c in ids if (a, b, c) not in lm.ngrams][:500]
    assert absent and all(table_lookup(tab, seq_hash(g)) < 0 for g in absent)
    for w, i in lm.vocab.items():
        if w not in ('<s>', '</s>', '<unk>'):
            assert lm.word_id([LABELS.index(c) for c in w]) == i
    assert lm.word_id([LABELS.index(c) for c in 'HELLOX']) is None


HASH_VECTORS = [[], [0], [1], [28, 3, 17], [-1, 5], list(range(40))]


def test_python_and_c_hash_agree(tmp_path):
    """codes/lm.py seq_hash == csrc/ds2_hash.h (the functions the kernel uses), compiled here as a host program."""
    from codes.lm import seq_hash
    src = tmp_path / 'h.cpp'
    body = ''.join('{ const int v[] = {%s}; uint64_t h = DS2_HASH_SEED; for (int i = 0; i < %d; ++i) h = ds2_hash_step(h, v[i]);'
                   ' printf("%%llu\\n", (unsigned long long)ds2_hash_key(h)); }\n' % (','.join(map(str, v or [0])), len(v))
                   for v in HASH_VECTORS)
    src.write_text('#include <stdio.h>\n#include "ds2_hash.h"\nint main() {\n%s return 0; }\n' % body)
    exe = tmp_path / 'h'
    cxx = os.environ.get('CXX', 'g++')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'aes-lac-2018_amd', 'csrc'), str(src), '-o',
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [seq_hash(v) for v in HASH_VECTORS]
    assert seq_hash([28, 3, 17]) == 4010985322569704704      # pinned: the tables of existing LM files depend on it


def test_beam_entry_points_are_declared_at_revision_404():
    from ds2hip import lib
    assert lib.ABI_VERSION == 404 and lib.query('ds2_version') == 404
    assert lib.query('ds2_ctc_beam_ws_bytes', 2, 10, 4) == 2 * (1 + 10 * 4) * 12
    assert 'ds2_ctc_beam_search_batch' in lib.SIGNATURES


def test_device_decoder_refusals():
    from codes.decoder import DeviceBeamCTCDecoder
    with pytest.raises(ValueError, match='1..128'):
        DeviceBeamCTCDecoder(LABELS, beam_width=129)
    import torch
    with pytest.raises(RuntimeError, match='device tensors'):
        DeviceBeamCTCDecoder(LABELS, beam_width=4).decode(torch.zeros(1, 3, len(LABELS)))


def test_lm_path_needs_the_beam_decoder():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '--lm-path', 'x.arpa', '--decoder', 'greedy'],
                       capture_output=True, text=True)
    assert r.returncode != 0 and '--lm-path needs --decoder beam' in r.stderr
