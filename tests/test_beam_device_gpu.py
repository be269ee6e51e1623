"""Device CTC beam search (ds2_ctc_beam_search_batch, csrc/ctc_beam.hip) against the host search
ds2_ctc_beam_search (no LM), the pure-Python contract tests/beam_ref.py (with a char or word LM), and exhaustive
enumeration of all alignments on tiny cases."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = ['_', ' ', "'"] + [chr(c) for c in range(ord('A'), ord('Z') + 1)]


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _device(probs, sizes, w, log_input=False, lm=None, alpha=0.0, beta=0.0, space_id=-1):
    from ds2hip import ops
    p = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    s = torch.tensor(sizes, dtype=torch.int32).cuda()
    out = ops.ctc_beam_search(p, s, w, 0, log_input, lm, alpha, beta, space_id)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _host(probs, n, w, log_input=False):
    from ds2hip import lib
    a = probs.shape[-1]
    ids, offs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    length, lp = ctypes.c_int(0), ctypes.c_float(0)
    lib.host_call('ds2_ctc_beam_search', np.ascontiguousarray(probs[:n]), n, a, 0, w, int(log_input), ids, offs,
                  len(ids), length, lp)
    return ids[:length.value].tolist(), lp.value


def _check_against_host(probs, sizes, w, log_input=False):
    labels, offsets, lens, score, ctc = _device(probs, sizes, w, log_input)
    for b, n in enumerate(sizes):
        want, want_lp = _host(probs[b], n, w, log_input)
        got = labels[b, :lens[b]].tolist()
        assert got == want, (b, n, w)
        assert abs(float(ctc[b]) - want_lp) <= 1e-6, (b, float(ctc[b]), want_lp)
        assert score[b] == ctc[b]
        lp = beam_ref.frame_log_probs(probs[b, :n], log_input)
        ref_lab, ref_off, _, _ = beam_ref.beam_search(lp, 0, w)
        assert got == ref_lab and offsets[b, :lens[b]].tolist() == ref_off
        assert not labels[b, lens[b]:].any()


@pytest.mark.parametrize('a', [29, 43])
@pytest.mark.parametrize('w', [1, 8, 16, 64, 128])
def test_no_lm_matches_the_host_search(a, w):
    rng = np.random.default_rng(1000 * a + w)
    t = 40 if w < 64 else 24
    probs = _softmax(rng.standard_normal((6, t, a)) * 2.5)
    _check_against_host(probs, [t, 0, 1, t - 3, 17, t], w)


def test_log_input_and_exact_zeros():
    rng = np.random.default_rng(7)
    probs = _softmax(rng.standard_normal((4, 30, 29)) * 2.0)
    _check_against_host(np.log(probs), [30, 30, 12, 1], 16, log_input=True)
    z = probs.copy()
    z[rng.random(z.shape) < 0.4] = 0.0
    z[..., 0] = np.maximum(z[..., 0], 0.05)
    _check_against_host(z, [30, 25, 30, 2], 16)


def _corpus_lm(tmp_path, order, unit):
    from codes.lm import NGramLM
    rng = np.random.default_rng(order)
    words = ['CAT', 'DOG', 'A', 'THE', 'BIRD', 'SEES', 'RUNS']
    sents = [' '.join(rng.choice(words, size=rng.integers(1, 5))) for _ in range(60)]
    txt = tmp_path / 'c.txt'
    txt.write_text('\n'.join(sents) + '\n')
    out = str(tmp_path / ('lm_%s%d.arpa' % (unit, order)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_lm.py'), '--order', str(order), '--unit', unit,
                        '--text', str(txt), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return NGramLM.from_arpa(out, LABELS, unit=unit), sents


def _spelled(rng, sents, b, t, a):
    """Noisy frames spelling corpus sentences (so that the LM sees in-vocabulary words), (b, t, a)."""
    x = rng.standard_normal((b, t, a)) * 1.5
    for i in range(b):
        s = sents[i % len(sents)]
        fr = 0
        for ch in s:
            if fr + 1 >= t:
                break
            x[i, fr, LABELS.index(ch)] += 3.0
            x[i, fr + 1, 0] += 2.0
            fr += 2
    return _softmax(x)


@pytest.mark.parametrize('unit', ['char', 'word'])
@pytest.mark.parametrize('order', [1, 2, 3, 4])
@pytest.mark.parametrize('w', [4, 16])
def test_lm_fusion_matches_the_reference(tmp_path, unit, order, w):
    lm, sents = _corpus_lm(tmp_path, order, unit)
    rng = np.random.default_rng(order * 10 + w)
    t = 40
    probs = _spelled(rng, sents, 4, t, 29)
    sizes = [t, 33, 1, t]
    alpha, beta = 0.7, 1.3
    labels, offsets, lens, score, ctc = _device(probs, sizes, w, lm=lm, alpha=alpha, beta=beta, space_id=1)
    for b, n in enumerate(sizes):
        lp = beam_ref.frame_log_probs(probs[b, :n], False)
        ref_lab, ref_off, ref_score, ref_ctc = beam_ref.beam_search(lp, 0, w, lm, alpha, beta, space_id=1)
        assert labels[b, :lens[b]].tolist() == ref_lab, (b, unit, order)
        assert offsets[b, :lens[b]].tolist() == ref_off
        assert abs(float(score[b]) - ref_score) <= 1e-6 * max(1.0, abs(ref_score))
        assert abs(float(ctc[b]) - ref_ctc) <= 1e-6 * max(1.0, abs(ref_ctc))


def _tiny_lm(tmp_path, labels, unit):
    from codes.lm import NGramLM
    if unit == 'char':
        text = ('\\data\\\nngram 1=5\nngram 2=4\n\n\\1-grams:\n-99\t<s>\t-0.3\n-0.6\t</s>\n-0.5\tA\t-0.2\n'
                '-0.9\tB\t-0.1\n-0.7\t<space>\n\n\\2-grams:\n-0.1\t<s> B\n-0.2\tA A\n-0.4\tB </s>\n-0.3\t<space> A\n'
                '\n\\end\\\n')
    else:
        text = ('\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-99\t<s>\t-0.2\n-0.5\t</s>\n-0.8\tab\t-0.3\n'
                '-0.6\ta\n-1.2\t<unk>\n\n\\2-grams:\n-0.2\t<s> ab\n-0.1\tab a\n-0.3\ta </s>\n\n\\end\\\n')
    p = tmp_path / ('tiny_%s.arpa' % unit)
    p.write_text(text)
    return NGramLM.from_arpa(str(p), labels, unit=unit)


@pytest.mark.parametrize('unit, a, t', [(None, 3, 6), (None, 4, 4), ('char', 4, 4), ('word', 4, 4), ('char', 3, 6)])
def test_exhaustive_argmax(tmp_path, unit, a, t):
    labels = ['_', ' ', 'A', 'B'][:a]
    lm = _tiny_lm(tmp_path, labels, unit) if unit else None
    alpha, beta = (0.9, 0.4) if unit else (0.0, 0.0)
    rng = np.random.default_rng(a * 7 + t)
    probs = _softmax(rng.standard_normal((5, t, a)) * 1.5)
    lab, _, lens, score, ctc = _device(probs, [t] * 5, 128, lm=lm, alpha=alpha, beta=beta, space_id=1)
    for b in range(5):
        lp = np.log(probs[b].astype(np.float64))
        total = {}
        for al in itertools.product(range(a), repeat=t):
            seq, prev = [], -1
            for c in al:
                if c != 0 and c != prev:
                    seq.append(c)
                prev = c
            v = sum(lp[i, c] for i, c in enumerate(al))
            k = tuple(seq)
            total[k] = np.logaddexp(total[k], v) if k in total else v
        fused = {k: v + (beam_ref.lm_score(lm, list(k), alpha, beta, 1) if lm else 0.0) for k, v in total.items()}
        best = max(fused, key=fused.get)
        second = max(v for k, v in fused.items() if k != best) if len(fused) > 1 else -math.inf
        assert fused[best] - second > 1e-6
        assert lab[b, :lens[b]].tolist() == list(best)
        assert abs(float(score[b]) - fused[best]) <= 1e-5 and abs(float(ctc[b]) - total[best]) <= 1e-5


@pytest.mark.parametrize('unit', ['char', 'word'])
def test_zero_weights_equal_no_lm_and_runs_are_bit_identical(tmp_path, unit):
    lm, sents = _corpus_lm(tmp_path, 3, unit)
    rng = np.random.default_rng(5)
    probs = _spelled(rng, sents, 8, 60, 29)
    sizes = [60, 0, 1, 59, 30, 60, 45, 2]
    base = _device(probs, sizes, 16)
    zero = _device(probs, sizes, 16, lm=lm, alpha=0.0, beta=0.0, space_id=1)
    for x, y in zip(base, zero):
        assert np.array_equal(x, y)
    one = _device(probs, sizes, 16, lm=lm, alpha=0.8, beta=1.0, space_id=1)
    two = _device(probs, sizes, 16, lm=lm, alpha=0.8, beta=1.0, space_id=1)
    for x, y in zip(one, two):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_decoder_class_and_argument_checks(tmp_path):
    from codes.decoder import BeamCTCDecoder, DeviceBeamCTCDecoder
    from ds2hip import lib, ops
    rng = np.random.default_rng(11)
    probs = torch.from_numpy(_softmax(rng.standard_normal((3, 50, 29)) * 2.0)).cuda()
    sizes = torch.tensor([50, 20, 35], dtype=torch.int32)
    dev = DeviceBeamCTCDecoder(LABELS, beam_width=16)
    host = BeamCTCDecoder(LABELS, beam_width=16)
    s_dev, _ = dev.decode(probs, sizes)
    s_host, _ = host.decode(probs, sizes)
    assert s_dev == s_host
    assert np.allclose(dev.last_ctc_log_probs, host.last_log_probs, atol=1e-6)
    assert dev.last_scores == dev.last_ctc_log_probs
    s = sizes.cuda()
    with pytest.raises(lib.Ds2Error, match='beam_width 129'):
        ops.ctc_beam_search(probs, s, 129)
    big = torch.zeros((1, 4, 129), device='cuda')
    with pytest.raises(lib.Ds2Error, match='alphabet size 129'):
        ops.ctc_beam_search(big, s[:1], 4)
