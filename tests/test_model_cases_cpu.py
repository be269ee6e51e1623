"""The whole-step suite's cases are what they claim to be (tests/model_cases.py); no GPU.

Every case meets the conditioning limit (the float32 restatement of the oracle within 2e-4 * max|ref| of float64 on every
held tensor), the 'open' regime has no clipped activation at all and the 'seeded' one has many, and the case table covers
every backward route of ``DeepSpeech._backward_impl`` / ``Trainer._forward_backward`` that tests/test_model_fp64_gpu.py is
there to hold -- so that a red GPU test speaks about the product and a green one about all of it."""
import pytest

from oracle.model import conv_out_time
from tests import model_cases as mc

CASES = mc.cases()


def test_case_and_route_names_are_unique():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        routes = [r.name for r in c.routes]
        assert len(routes) == len(set(routes)), c.name


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_case_is_well_conditioned(case):
    ref = mc.reference(case)
    worst, where = mc.conditioning(ref)
    print('%s: worst e32 / max|ref| = %.2e (%s), loss %.4f' % (case.name, worst, where, ref['loss']))
    assert ref['loss'] == ref['loss'] and abs(ref['loss']) < float('inf') and ref['loss'] > 0
    for name, (m32, _) in ref['e32'].items():
        if ref['amax'][name] >= mc.CONDITION_FLOOR:
            assert m32 <= mc.CONDITION * ref['amax'][name], (name, m32, ref['amax'][name])
    # every family is present, and the gradients that are exactly zero are zero in float64
    assert {mc.family_of(name) for name in ref['r64']} == set(mc.FAMILIES)
    zero = ['grad:conv.0.bias', 'grad:conv.3.bias'] + (['grad:conv.1.bias'] if case.regime == 'open' else [])
    for name in zero:
        assert ref['amax'][name] < 1e-12, (name, ref['amax'][name])
    if conv_out_time(case.t_in) == 1:
        for name in ref['r64']:
            if 'weight_hh' in name:
                assert ref['amax'][name] == 0.0 and ref['e32'][name] == (0.0, 0.0), name


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_clip_regimes(case):
    clip = mc.reference(case)['clip']
    for k in ('conv1', 'conv2'):
        low, high, n = clip[k]
        if case.regime == 'open':
            assert low == 0 and high == 0, (k, clip[k])
        else:
            assert 0.4 * n <= low <= 0.6 * n, (k, clip[k])          # half of both conv outputs sit on the lower clip


def test_every_route_has_a_case():
    have = {(c.name, r.name) for c in CASES for r in c.routes}
    print()
    for pair in sorted(have):
        print('%-12s %s' % pair)
    want = [('prod-open', 'autograd')]
    # the production shape, 'seeded': every entry point, every stream arrangement, the hook both ways, the frozen conv block
    for route in ('autograd', 'fb_nan', 'trainer', 'fb_nan-no_overlap', 'trainer-no_overlap', 'fb_nan-no_defer',
                  'trainer-no_defer', 'hook-defer', 'hook-no_defer', 'hook-frozen_conv'):
        want.append(('prod-seeded', route))
    for bsz in (1, 5, 9, 13, 17, 33):
        want += [('B%d' % bsz, 'trainer'), ('B%d' % bsz, 'autograd')]
    for t in (1, 2):
        want += [('T%d' % t, 'fb_nan'), ('T%d' % t, 'trainer')]
    want += [('raw_dw', 'fb_nan-raw_dw'), ('raw_dw', 'trainer-raw_dw')]
    want += [('ragged', 'trainer'), ('ragged', 'autograd')]
    for w in want:
        assert w in have, w
    assert len(want) == len(have)                      # ... and nothing the enumeration above does not know

    by = {c.name: c for c in CASES}
    routes = {(c.name, r.name): r for c in CASES for r in c.routes}
    # the shapes and switches behind the names
    for name in ('prod-seeded', 'prod-open'):
        c = by[name]
        assert c.kwargs == {} and c.bsz == 10 and conv_out_time(c.t_in) == 26          # H = 800, five layers by default
    assert by['prod-seeded'].regime == 'seeded' and by['prod-open'].regime == 'open'
    for bsz in (1, 5, 9, 13, 17, 33):
        c = by['B%d' % bsz]
        assert c.bsz == bsz and c.kwargs == dict(rnn_hidden_size=800, num_rnn_layers=2) and conv_out_time(c.t_in) == 26
    for t in (1, 2):
        c = by['T%d' % t]
        assert conv_out_time(c.t_in) == t and c.bsz == 3 and c.kwargs == dict(rnn_hidden_size=32, num_rnn_layers=2)
    c = by['raw_dw']
    assert c.bsz == 10 and conv_out_time(c.t_in) == 26 and c.kwargs == dict(rnn_hidden_size=800, num_rnn_layers=2)
    assert all(r.raw_dw for r in c.routes) and {r.entry for r in c.routes} == {'fb', 'trainer'}     # acc_beta 0 and 1
    assert not any(r.raw_dw for cc in CASES if cc.name != 'raw_dw' for r in cc.routes)
    c = by['ragged']
    assert c.bsz == 4 and list(c.lengths) == [c.t_in, c.t_in - 17, c.t_in - 40, 51] and len(set(c.lengths)) == 4
    sizes = mc.out_sizes_of(mc.inputs_for(c)[2], conv_out_time(c.t_in)).tolist()
    assert sizes[0] == 26 and len(set(sizes)) == 4 and all(s >= 2 * n for s, n in zip(sizes, c.label_lens))
    r = routes[('prod-seeded', 'fb_nan-no_overlap')]
    assert not r.overlap and r.entry == 'fb' and not routes[('prod-seeded', 'trainer-no_overlap')].overlap
    for name in ('fb_nan-no_defer', 'trainer-no_defer', 'hook-no_defer'):
        r = routes[('prod-seeded', name)]
        assert r.overlap and not r.defer
    for name in ('hook-defer', 'hook-frozen_conv', 'trainer', 'fb_nan', 'autograd'):
        r = routes[('prod-seeded', name)]
        assert r.overlap and r.defer
    assert routes[('prod-seeded', 'hook-frozen_conv')].frozen and routes[('prod-seeded', 'hook-frozen_conv')].entry == 'hook'
    assert [r.name for c in CASES for r in c.routes if r.frozen] == ['hook-frozen_conv']


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_transcripts_are_feasible(case):
    _, labels, pct, sizes = mc.inputs_for(case)
    out = mc.out_sizes_of(pct, conv_out_time(case.t_in)).tolist()
    assert sizes.tolist() == list(case.label_lens) and labels.numel() == sum(case.label_lens)
    assert int(labels.min()) >= 1 and int(labels.max()) <= 28 if labels.numel() else True
    off = 0
    for n, t in zip(case.label_lens, out):
        lab = labels[off:off + n].tolist()
        off += n
        assert all(a != b for a, b in zip(lab, lab[1:]))            # no repeat: n labels need n frames
        assert n <= t
    _, other, _, _ = mc.inputs_for(case, other=True)
    assert not (mc.inputs_for(case)[0] == mc.inputs_for(case, other=True)[0]).all()
