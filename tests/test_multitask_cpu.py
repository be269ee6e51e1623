"""Multi-task model, data and config surface on the host: state_dict layout and same-seed initialisation against the
reference's MultiTaskModel, the multi-task collate, the weighted sampler's bins, and the refusals at config load."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_multitask import MT_KW, ToySource

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'multitask')


def _configs():
    from codes.utils.io_utils import AttrDict
    with open(os.path.join(GOLDEN, 'ref_multitask_configs.json')) as f:
        texts = json.load(f)
    return {name: AttrDict(json.loads(text)) for name, text in texts.items()}


@pytest.mark.parametrize('name', ['example-multi-task.json', 'multi-task.json', 'multi-task-schedule-sampling.json'])
def test_get_model_builds_the_reference_multitask_layout(name):
    from codes.model import MultiTaskModel
    from codes.utils import training_utils as tu
    cfg = _configs()[name]
    model = tu.get_model(cfg.model)
    assert isinstance(model, MultiTaskModel)
    sd = model.state_dict()
    assert not any(k.startswith('base_model.fc') for k in sd)
    assert sd['base_model.conv.0.weight'].shape == (32, 1, 41, 11)
    assert sd['base_model.rnns.4.rnn.weight_hh_l0_reverse'].shape == (2400, 800)
    for i, a in enumerate((29, 43)):                    # NUM_CLASSES per language, in langs order
        assert sd['heads.%d.fc.0.module.1.weight' % i].shape == (a, 800)
        for leaf in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'):
            assert 'heads.%d.fc.0.module.0.%s' % (i, leaf) in sd
    keys = list(sd)
    assert keys.index('heads.0.fc.0.module.0.weight') > keys.index('base_model.rnns.4.rnn.weight_hh_l0_reverse')


def test_same_seed_initialisation_equals_the_reference():
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    g = np.load(os.path.join(GOLDEN, 'ref_mt_tiny.npz'))
    torch.manual_seed(0)
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': dict(MT_KW, num_classes=999)}))
    sd = model.state_dict()
    want = sorted(k[len('init_sum_'):] for k in g.files if k.startswith('init_sum_'))
    assert sorted(k for k, v in sd.items() if v.is_floating_point()) == want
    for k in want:
        v = sd[k].numpy()
        assert v.sum(dtype=np.float64) == pytest.approx(float(g['init_sum_' + k]), rel=1e-5, abs=1e-4), k
        flat = v.reshape(-1)
        np.testing.assert_array_equal(flat[::max(1, flat.size // 256)][:256], g['init_sample_' + k], err_msg=k)


def test_flat_buffer_covers_base_then_heads():
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': dict(MT_KW)}))
    model._ensure_flat()
    flat = model._flat_p
    assert {id(p) for p in model.parameters()} == {id(p) for p in model._plist}
    for p, o in zip(model._plist, model._offsets):
        assert p.data_ptr() == flat.data_ptr() + 4 * o
    heads = [p for h in model.heads for p in h.parameters()]
    assert [id(p) for p in model._plist[-len(heads):]] == [id(p) for p in heads]


def _item(t_i, labels, task):
    return torch.full((t_i, 161), float(t_i)), labels, task


def test_multitask_collate_layout_and_percentages():
    from codes.data import collate_multitask
    batch = [_item(5, [1, 2], 1), _item(9, [3], 0), _item(7, [4, 5, 6], 1), _item(3, [7], 0)]
    inputs, targets, pct, sizes = collate_multitask(batch, 3)
    assert inputs[2] is None and targets[2] is None and pct[2] is None and sizes[2] is None
    assert inputs[0].shape == (2, 9, 161) and inputs[1].shape == (2, 9, 161)    # batch-wide T_max for every task
    assert inputs[0][0, :, 0].tolist() == [9.0] * 9
    assert inputs[0][1, :, 0].tolist() == [3.0] * 3 + [0.0] * 6
    assert inputs[1][1, :, 0].tolist() == [7.0] * 7 + [0.0] * 2
    np.testing.assert_allclose(pct[0].numpy(), [1.0, 3 / 9.0])
    np.testing.assert_allclose(pct[1].numpy(), [5 / 9.0, 7 / 9.0])
    assert targets[0].tolist() == [3, 7] and targets[1].tolist() == [1, 2, 4, 5, 6]
    assert sizes[0].tolist() == [1, 1] and sizes[1].tolist() == [2, 3]
    # task order in one tensor: the model's concatenation of the present tasks is the base storage
    assert inputs[1].data_ptr() == inputs[0].data_ptr() + inputs[0].numel() * 4
    # an absent task in a two-task batch
    inputs, targets, pct, sizes = collate_multitask([_item(4, [1], 1), _item(6, [2], 1)], 2)
    assert inputs[0] is None and inputs[1].shape == (2, 6, 161)
    np.testing.assert_allclose(pct[1].numpy(), [4 / 6.0, 1.0])


def test_concat_dataset_yields_the_task_index():
    from codes.data import ConcatAudioDataset

    class _DS(torch.utils.data.Dataset):
        def __init__(self, n, tag):
            self.n, self.tag, self.durations = n, tag, [float(i) for i in range(n)]

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            return (self.tag, i), [i]

    ds = ConcatAudioDataset([_DS(2, 'a'), _DS(3, 'b')])
    assert ds.cumulative_sizes == [2, 5] and ds.durations == [0.0, 1.0, 0.0, 1.0, 2.0]
    assert ds[1] == (('a', 1), [1], 0) and ds[2] == (('b', 0), [0], 1) and ds[4][2] == 1


def test_weighted_sampler_bins_equal_the_reference():
    from codes.sampler import WeightedBucketingRandomSampler
    with open(os.path.join(GOLDEN, 'ref_mt_sampler.json')) as f:
        g = json.load(f)
    src = ToySource(tuple(g['counts']))
    assert src.durations == g['durations']
    for sampling, per in g['bins'].items():
        s = WeightedBucketingRandomSampler(src, batch_size=g['batch_size'], sampling=sampling, num_epochs=g['num_epochs'])
        for epoch in sorted(per, key=int):
            if int(epoch):
                s.shuffle(int(epoch))
            assert s.bins == per[epoch], (sampling, epoch)
    with pytest.raises(ValueError, match='exactly 2'):
        WeightedBucketingRandomSampler(ToySource((2, 3, 4)), sampling='schedule', num_epochs=3)


@pytest.mark.parametrize('key,where,value', [('freeze_layers', 'model', 'all'), ('map_fc', 'model', 'map.json'),
                                             ('finetune', 'training', True)])
def test_finetuning_keys_in_a_multitask_config_are_refused(key, where, value):
    from codes.utils import training_utils as tu
    cfg = _configs()['multi-task.json']
    tu.check_multitask_config(cfg)                      # the shipped config itself loads
    cfg[where][key] = value
    with pytest.raises(ValueError, match='%s in a multi-task config' % key):
        tu.check_multitask_config(cfg)
    # the reference's own example carries freeze_layers: "all"
    with pytest.raises(ValueError, match='freeze_layers in a multi-task config'):
        tu.check_multitask_config(_configs()['example-multi-task.json'])


def test_test_py_refuses_a_multitask_checkpoint(tmp_path):
    import test as test_cli
    from codes.utils.io_utils import AttrDict
    cfg = _configs()['multi-task.json']
    path = str(tmp_path / 'mt.pth')
    torch.save({'args': {'config': AttrDict(cfg)}, 'state_dict': {}}, path)
    try:
        with pytest.raises(SystemExit, match='multi-task checkpoint'):
            test_cli.main(['--model-path', path, '--manifest', 'unused.csv'])
    finally:
        torch.set_grad_enabled(True)                    # (the refusal comes first; keep the process state as it was)


def test_trainer_needs_one_weight_per_head():
    from codes.engine import create_trainer
    from codes.utils import training_utils as tu
    from codes.utils.io_utils import AttrDict
    model = tu.get_model(AttrDict({'langs': ['en', 'pt_BR'], 'params': dict(MT_KW)}))
    with pytest.raises(ValueError, match='one weight per task'):
        create_trainer(model, None, None, 'cpu', task_weights=[1])
    with pytest.raises(ValueError, match='one weight per task'):
        create_trainer(model, None, None, 'cpu', task_weights=[1, 1, 1])


def test_raw_audio_multitask_collate_and_split():
    from codes.data import TaskCounts, collate_audio_multitask, split_tasks
    clips = [torch.full((n,), float(n)) for n in (300, 500, 200, 400)]
    batch = [(clips[0], [1, 2], 1), (clips[1], [3], 0), (clips[2], [4, 5, 6], 1), (clips[3], [7], 0)]
    wavs, targets, counts, sizes = collate_audio_multitask(batch, 3)
    assert isinstance(counts, TaskCounts) and tuple(counts) == (2, 2, 0)
    assert [int(w.numel()) for w in wavs] == [500, 400, 300, 200]                  # clips in task order
    assert targets[0].tolist() == [3, 7] and targets[1].tolist() == [1, 2, 4, 5, 6] and targets[2] is None
    assert sizes[0].tolist() == [1, 1] and sizes[1].tolist() == [2, 3] and sizes[2] is None
    spect = torch.arange(4 * 6 * 161, dtype=torch.float32).view(4, 6, 161)       # what the frontend makes of them
    pct = torch.tensor([1.0, 0.8, 0.6, 0.4])
    xs, ps = split_tasks(spect, pct, counts)
    assert xs[2] is None and ps[2] is None
    assert torch.equal(xs[0], spect[:2]) and torch.equal(xs[1], spect[2:]) and xs[1].data_ptr() == spect[2:].data_ptr()
    assert ps[0].tolist() == pytest.approx([1.0, 0.8]) and ps[1].tolist() == pytest.approx([0.6, 0.4])
