"""LMTuner, DeviceErrorRate and decode_labels against the path test.py takes: DeviceBeamCTCDecoder(alpha, beta).decode, then
Decoder.wer / Decoder.cer on the strings."""
import numpy as np
import pytest
import torch

from tests.test_beam_edges_gpu import LABELS, _make_lm, _spell

pytestmark = pytest.mark.gpu
T, A, W = 48, len(LABELS), 8
ALPHAS, BETAS = [0.0, 0.7, 1.9], [0.0, 1.5]


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    """Two batches (3 and 2 utterances) of probabilities that spell a corrupted sentence, with the sentences as targets."""
    lm, sents, _ = _make_lm(tmp_path_factory.mktemp('tune_lm'), 3, 'char')
    rng = np.random.default_rng(99)
    batches = []
    for bsz, first in ((3, 0), (2, 3)):
        refs = [sents[first + b][:T // 2 - 2] for b in range(bsz)]
        said = [r.replace('A', 'E', 1)[:len(r) - b] for b, r in enumerate(refs)]          # what the frames spell
        probs = torch.from_numpy(np.stack([_spell(rng, s, T, A, noise=2.0) for s in said]).astype(np.float32)).cuda()
        sizes = torch.tensor([T - 3 * b for b in range(bsz)], dtype=torch.int32)
        targets = torch.tensor([LABELS.index(c) for r in refs for c in r], dtype=torch.int32)
        target_sizes = torch.tensor([len(r) for r in refs], dtype=torch.int32)
        batches.append((probs, sizes, targets, target_sizes, refs))
    return lm, batches


def _string_path(decoder, batches):
    """test.py's loop: decode to strings, wer / cer per utterance, summed."""
    tot = {'word_dist': 0, 'char_dist': 0, 'ref_words': 0, 'ref_len': 0}
    for probs, sizes, _, _, refs in batches:
        decoded, _ = decoder.decode(probs, sizes)
        for hyp, ref in zip(decoded, refs):
            tot['word_dist'] += decoder.wer(hyp[0], ref)
            tot['char_dist'] += decoder.cer(hyp[0], ref)
            tot['ref_words'] += len(ref.split())
            tot['ref_len'] += len(ref)
    tot['wer'] = 100.0 * tot['word_dist'] / max(1, tot['ref_words'])
    tot['cer'] = 100.0 * tot['char_dist'] / max(1, tot['ref_len'])
    return tot


@pytest.fixture(scope='module')
def by_strings(setup):
    from codes.decoder import DeviceBeamCTCDecoder
    lm, batches = setup
    return {(a, b): _string_path(DeviceBeamCTCDecoder(LABELS, beam_width=W, lm=lm, alpha=a, beta=b), batches)
            for a in ALPHAS for b in BETAS}


@pytest.mark.parametrize('rows_per_launch', [4, 1024])
def test_tuner_equals_the_string_path(setup, by_strings, rows_per_launch):
    from codes.tune import LMTuner, best_point
    lm, batches = setup
    tuner = LMTuner(LABELS, lm, W, ALPHAS, BETAS, rows_per_launch=rows_per_launch)
    for probs, sizes, targets, target_sizes, _ in batches:
        tuner.add_batch(probs, sizes, targets, target_sizes)
    # 4 rows: one grid point per launch of the 3-utterance batch (at least one), two of the 2-utterance batch
    assert tuner.launches == (6 + 3 if rows_per_launch == 4 else 2)
    res = tuner.result()
    assert res['utterances'] == 5 and len(res['grid']) == 6
    assert [(e['alpha'], e['beta']) for e in res['grid']] == [(a, b) for a in ALPHAS for b in BETAS]       # alpha-major
    for e in res['grid']:
        want = by_strings[(e['alpha'], e['beta'])]
        for k, v in want.items():
            assert e[k] == v, (e['alpha'], e['beta'], k)
        assert e['char_sub'] + e['char_del'] + e['char_ins'] == e['char_dist']
        assert e['word_sub'] + e['word_del'] + e['word_ins'] == e['word_dist']
    assert res['ref_words'] == want['ref_words'] and res['ref_len'] == want['ref_len']
    assert res['best'] == best_point(res['grid'])
    assert len({(e['word_dist'], e['char_dist']) for e in res['grid']}) > 1          # the weights matter on this input


def test_device_error_rate_and_decode_labels(setup, by_strings):
    from codes.decoder import DeviceBeamCTCDecoder, GreedyDecoder
    from codes.metrics import DeviceErrorRate
    lm, batches = setup
    space = LABELS.index(' ')
    for dec in (GreedyDecoder(LABELS), DeviceBeamCTCDecoder(LABELS, beam_width=W),
                DeviceBeamCTCDecoder(LABELS, beam_width=W, lm=lm, alpha=0.7, beta=1.5)):
        meter = DeviceErrorRate(space)
        for probs, sizes, targets, target_sizes, _ in batches:
            labels, lens = dec.decode_labels(probs, sizes)
            assert labels.is_cuda and lens.is_cuda and labels.dtype == torch.int32 and lens.dtype == torch.int32
            strings = [[dec._to_string(row[:n])] for row, n in zip(labels.cpu().numpy(), lens.cpu().tolist())]
            assert strings == dec.decode(probs, sizes)[0]
            meter.update(labels, lens, targets, target_sizes)
        got, want = meter.compute(), _string_path(dec, batches)
        for k, v in want.items():
            assert got[k] == v, k
        assert got['utterances'] == 5
    assert want == by_strings[(0.7, 1.5)]
