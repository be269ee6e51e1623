"""Factories driven by the JSON config (reference ``codes/utils/training_utils.py``).

Config schema (unchanged): ``model{name, langs, freeze_layers, map_fc, params}``,
``training{num_epochs, batch_size, max_norm, augment, finetune}``, ``optimizer{name, params, per_layer_lr}``,
``scheduler{name, params}``.  Additions: ``training.audio_scale`` (``audio_scale``) and the optional block
``training.noise{path, noise_levels, prob}`` (``get_noise``), ``training.reverb{path, prob, ...}`` (``get_reverb``), ``training.speed{factors, prob}`` (``get_speed``) and ``training.spec_augment{...}`` (``get_spec_augment``), and ``training.mwer{nbest, beam_width, ctc_weight, risk}`` (``get_mwer``).  Broken branches of the reference are implemented to their evident intent
(SURVEY.md section 4): ``langs[0]`` is the fine-tune target language, the new FC layer's *weight* is
normally initialised.
"""
import json
import logging
import os

import torch

from .. import transforms
from ..data import AudioDataLoader, AudioDataset, ConcatAudioDataset
from ..model import DeepSpeech, MultiTaskModel, SequenceWiseClassifier, _BatchNormParams, _LinearParams
from ..sampler import BucketingSampler, DistributedBucketingSampler, WeightedBucketingRandomSampler

LOG = logging.getLogger('aes-lac-2018')
NUM_CLASSES = {'pt_BR': 43, 'en': 29}


def get_default_transforms(data_dir, config, gpu_frontend=True, noise=True):
    """Waveform loader (+ per-utterance spectrogram when ``gpu_frontend`` is False) and one ToLabel per language
    (training_utils.py:18-34).  With ``gpu_frontend`` the spectrogram runs batched on the device after collate.
    ``training.noise`` of the config (``get_noise``) reaches the TRAINING transform only: its ``ToTensor`` draws the noise
    (``transforms.waveform_noise(train_t)`` is what the training ``BatchSpectrogram`` is built with), or, without
    ``gpu_frontend``, the ``NoiseInjection`` stands between the loader and the spectrogram as in the reference.
    ``training.spec_augment`` (``get_spec_augment``) travels the same way: the training ``ToTensor`` draws
    (``transforms.waveform_spec_augment(train_t)`` is what the training ``BatchSpectrogram`` is built with), or, without
    ``gpu_frontend``, the ``SpecAugment`` stands behind the spectrogram.
    ``training.reverb`` (``get_reverb``) likewise: the training ``ToTensor`` draws (``transforms.waveform_reverb(train_t)``
    is what the training ``BatchSpectrogram`` is built with), or, without ``gpu_frontend``, the ``Reverb`` stands in front
    of the ``NoiseInjection``.
    ``training.speed`` (``get_speed``) likewise: the training ``ToTensor`` draws, in front of the tempo draw
    (``transforms.waveform_speed(train_t)`` is what the training ``BatchSpectrogram`` is built with), and without
    ``gpu_frontend`` the per-clip ``ToTensor`` applies it itself, before its decode.
    ``noise=False`` (evaluation: ``load_model(return_transforms=True)``) does not even look at any of these blocks."""
    augment = bool(config.training.get('augment', False))       # tempo + gain on the training set only
    # gpu_frontend: workers hand on int16 clips + the drawn (tempo, gain); decode, WSOLA, gain and the spectrogram all run
    # on the device after collate.  Otherwise the reference's per-utterance contract (each transform returns a tensor).
    tail = [] if gpu_frontend else [transforms.ToSpectrogram(librosa_compat=True)]
    scale = audio_scale(config)
    bank = get_noise(data_dir, config, scale) if noise else None
    spec = get_spec_augment(config) if noise else None
    rir = get_reverb(data_dir, config) if noise else None
    speed = get_speed(config) if noise else None
    if gpu_frontend:
        train_t = transforms.Compose([transforms.ToTensor(augment=augment, defer=True, scale=scale, noise=bank,
                                                          spec_augment=spec, reverb=rir, speed=speed)])
    else:
        train_t = transforms.Compose([transforms.ToTensor(augment=augment, defer=False, scale=scale, speed=speed)] +
                                     ([rir] if rir is not None else []) + ([bank] if bank is not None else []) + tail + ([spec] if spec is not None else []))
    val_t = transforms.Compose([transforms.ToTensor(augment=False, defer=gpu_frontend, scale=scale)] + tail)
    target_t = [transforms.ToLabel(os.path.join(data_dir, 'labels.{}.json'.format(lang)), lang=lang,
                                   remove_accents=(lang != 'pt_BR')) for lang in config.model.langs]
    return train_t, val_t, target_t


def audio_scale(config):
    """``training.audio_scale`` of the JSON config (an addition to the reference's schema; saved with the checkpoint's
    ``args`` so ``test.py`` decodes the way the model was trained): 'unit' (default), 'int32' or a number -- the amplitude
    contract of the waveform loader (``transforms.ToTensor``)."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    return (training or {}).get('audio_scale', None)


def get_noise(data_dir, config, scale=None):
    """``training.noise`` of the JSON config (an addition to the reference's schema, whose NoiseInjection no config reaches):
    ``{"path": DIR, "noise_levels": [lo, hi], "prob": p}`` -> a ``transforms.NoiseInjection`` (None without the block);
    ``"resample": true`` converts files at another rate or channel count when the bank is built (the default refuses them).
    Independent of ``training.augment``; a relative ``path`` that does not exist from the working directory is looked up
    under ``--data-dir``.  The block is saved with the checkpoint's ``args``; nothing reads it at test time."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    block = (training or {}).get('noise', None)
    if not block:
        return None
    unknown = set(block) - {'path', 'noise_levels', 'prob', 'max_bank_seconds', 'resample'}
    if unknown or 'path' not in block:
        raise ValueError('training.noise takes path (required), noise_levels, prob, max_bank_seconds, resample; got %s'
                         % sorted(block))
    kwargs = {k: block[k] for k in ('noise_levels', 'prob', 'max_bank_seconds', 'resample') if k in block}
    return transforms.NoiseInjection(_resolve(block['path'], data_dir), scale=scale, **kwargs)


REVERB_KEYS = ('path', 'prob', 'max_rir_seconds', 'max_bank_seconds', 'resample')


def get_reverb(data_dir, config):
    """``training.reverb`` of the JSON config (an addition to the reference's schema): ``{"path": DIR, "prob": p,
    "max_rir_seconds": s, "max_bank_seconds": S, "resample": false}`` -> a ``transforms.Reverb`` (None without the block;
    ``"resample": true`` converts files at another rate or channel count, the default refuses them).  ``path`` is required;
    keys left out keep the constructor's defaults; an unknown key is refused by name.  Independent of ``training.augment``,
    ``training.noise`` and ``training.spec_augment``; a relative ``path`` that does not exist from the working directory is
    looked up under ``--data-dir``.  The block is saved with the checkpoint's ``args``; nothing reads it at test time."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    block = (training or {}).get('reverb', None)
    if not block:
        return None
    unknown = sorted(set(block) - set(REVERB_KEYS))
    if unknown:
        raise ValueError('training.reverb: unknown key(s) %s; it takes %s' % (', '.join(unknown), ', '.join(REVERB_KEYS)))
    if 'path' not in block:
        raise ValueError('training.reverb needs path (the directory of RIR files); got %s' % sorted(block))
    rir = transforms.Reverb(_resolve(block['path'], data_dir), **{k: block[k] for k in REVERB_KEYS[1:] if k in block})
    LOG.info('Reverberation on the training set: {}'.format(rir))
    return rir


SPEED_KEYS = ('factors', 'prob')


def get_speed(config):
    """``training.speed`` of the JSON config (an addition to the reference's schema): ``{"factors": [0.9, 1.0, 1.1],
    "prob": 1.0}`` -> a ``transforms.SpeedPerturb`` (None without the block).  Keys left out keep the constructor's defaults
    (``{}`` is all defaults); an unknown key is refused by name.  Independent of ``training.augment`` and of the other blocks;
    it reaches the training set only.  The block is saved with the checkpoint's ``args``; nothing reads it at test time."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    block = (training or {}).get('speed', None)
    if block is None:
        return None
    unknown = sorted(set(block) - set(SPEED_KEYS))
    if unknown:
        raise ValueError('training.speed: unknown key(s) %s; it takes %s' % (', '.join(unknown), ', '.join(SPEED_KEYS)))
    speed = transforms.SpeedPerturb(**{k: block[k] for k in SPEED_KEYS if k in block})
    LOG.info('Speed perturbation on the training set: {}'.format(speed))
    return speed


SPEC_AUGMENT_KEYS = ('freq_masks', 'freq_width', 'time_masks', 'time_width', 'time_ratio', 'time_warp', 'prob', 'mask_value')


def get_spec_augment(config):
    """``training.spec_augment`` of the JSON config (an addition to the reference's schema): a block whose keys are
    ``transforms.SpecAugment``'s keyword names -> that object; keys left out keep the constructor's defaults (``{}`` is all
    defaults), an unknown key is refused by name, and None comes back without the block.  Independent of
    ``training.augment`` and ``training.noise``.  The block is saved with the checkpoint's ``args``; nothing reads it at
    test time."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    block = (training or {}).get('spec_augment', None)
    if block is None:
        return None
    unknown = sorted(set(block) - set(SPEC_AUGMENT_KEYS))
    if unknown:
        raise ValueError('training.spec_augment: unknown key(s) %s; it takes %s' % (', '.join(unknown),
                                                                                   ', '.join(SPEC_AUGMENT_KEYS)))
    return transforms.SpecAugment(**{k: block[k] for k in SPEC_AUGMENT_KEYS if k in block})


MWER_KEYS = ('nbest', 'beam_width', 'ctc_weight', 'risk')
MWER_DEFAULTS = {'nbest': 4, 'beam_width': 8, 'ctc_weight': 0.01, 'risk': 'word'}
MWER_MAX_BEAM = 128                      # DS2_MWER_MAX_NBEST of include/ds2hip.h


def get_mwer(config, labels=None):
    """``training.mwer`` of the JSON config (an addition to the reference's schema): ``{"nbest": 4, "beam_width": 8,
    "ctc_weight": 0.01, "risk": "word"}`` -> the block with its defaults filled in, the keywords of
    ``codes.ctc.mwer_costs_and_grad`` (None without the block; ``{}`` is all defaults).  Refused by name when the config is
    loaded: an unknown key, ``beam_width`` outside 1..128, ``nbest`` outside 1..beam_width, a negative ``ctc_weight``, a
    ``risk`` other than word / char, a multi-task config, and -- with ``labels``, the alphabet as a list -- ``risk = word``
    on an alphabet without a space label.  The block is saved with the checkpoint's ``args``; nothing reads it at test time."""
    training = config.get('training', {}) if hasattr(config, 'get') else {}
    block = (training or {}).get('mwer', None)
    if block is None:
        return None
    unknown = sorted(set(block) - set(MWER_KEYS))
    if unknown:
        raise ValueError('training.mwer: unknown key(s) %s; it takes %s' % (', '.join(unknown), ', '.join(MWER_KEYS)))
    out = dict(MWER_DEFAULTS)
    out.update({k: block[k] for k in MWER_KEYS if k in block})
    for key in ('nbest', 'beam_width'):
        if isinstance(out[key], bool) or not isinstance(out[key], int):
            raise ValueError('training.mwer: %s must be an integer, got %r' % (key, out[key]))
    if not 1 <= out['beam_width'] <= MWER_MAX_BEAM:
        raise ValueError('training.mwer: beam_width %d is outside 1..%d' % (out['beam_width'], MWER_MAX_BEAM))
    if not 1 <= out['nbest'] <= out['beam_width']:
        raise ValueError('training.mwer: nbest %d is outside 1..beam_width = %d' % (out['nbest'], out['beam_width']))
    if isinstance(out['ctc_weight'], bool) or not isinstance(out['ctc_weight'], (int, float)) or \
            not 0 <= out['ctc_weight'] < float('inf'):
        raise ValueError('training.mwer: ctc_weight must be a finite number >= 0, got %r' % (out['ctc_weight'],))
    if out['risk'] not in ('word', 'char'):
        raise ValueError('training.mwer: risk must be "word" or "char", got %r' % (out['risk'],))
    langs = (config.get('model', None) or {}).get('langs', None)
    if isinstance(langs, (tuple, set, list)) and len(langs) > 1:
        raise ValueError('training.mwer in a multi-task config (model.langs = %s): MWER training covers one classifier'
                         % list(langs))
    if labels is not None and out['risk'] == 'word' and ' ' not in list(labels):
        raise ValueError('training.mwer: risk = "word" needs an alphabet with a space label; use risk = "char"')
    return out


def is_multitask(config):
    langs = config.model.langs
    return isinstance(langs, (tuple, set, list)) and len(langs) > 1


def check_multitask_config(config):
    """Refuse, when the config is loaded, what the reference's multi-task path cannot do either: its ``finetune_model`` reads
    ``model.fc``, which a MultiTaskModel does not have (training_utils.py:87-122)."""
    if not is_multitask(config):
        return
    for key, where in (('finetune', config.get('training', {}) or {}), ('freeze_layers', config.model),
                       ('map_fc', config.model)):
        if where.get(key, None):
            raise ValueError('%s in a multi-task config (model.langs = %s): fine-tuning surgery replaces model.fc, which '
                             'a multi-task model does not have -- the reference fails here too' % (key, list(config.model.langs)))


def get_model(model_dict):
    params = dict(model_dict.get('params', {}) or {})
    # The drop-in covers ONE frontend geometry: 320-sample windows (20 ms at 16 kHz, 161 frequency bins) -- what every shipped
    # config and the reference's released checkpoints use.  The reference derives the model's input width for any window
    # (codes/model.py:124,148-151); the HIP conv, BatchNorm-layout and STFT kernels are specialised for 161 bins, so a config
    # that asks for another one is refused HERE, when it is loaded, with the reason -- not later inside the constructor.
    if int(params.get('window_size', 320)) != 320:
        raise ValueError('model.params.window_size = %r: this MI355X path implements window_size = 320 only (161 frequency '
                         'bins; conv / BatchNorm / STFT kernels are specialised for it) -- see README.md "What the drop-in '
                         'does not cover"' % (params['window_size'],))
    if isinstance(model_dict.langs, (tuple, set, list)) and len(model_dict.langs) > 1:
        # training_utils.py:37-44: a shared base without classifier, one head per language (NUM_CLASSES[lang]; a
        # num_classes in params is ignored, as the reference's base ignores it)
        params['include_classifier'] = False
        model_dict['params'] = params
        base = DeepSpeech(**params)
        heads = [SequenceWiseClassifier(base._rnn_hidden_size, NUM_CLASSES[lang]) for lang in model_dict.langs]
        return MultiTaskModel(base, heads)
    params.setdefault('num_classes', NUM_CLASSES[model_dict.langs[0]])
    model_dict['params'] = params
    return DeepSpeech(**params)


def _freeze_layers(model, freeze_layers):
    if freeze_layers is None:
        return model
    if isinstance(freeze_layers, str):
        freeze_layers = [freeze_layers]
    count = 0
    for name in freeze_layers:
        target = model if name == 'all' else getattr(model, name)
        if isinstance(target, torch.nn.Module):
            for m in target.modules():
                if isinstance(m, _BatchNormParams):
                    # the reference puts the BatchNorm of a frozen LAYER (not of 'all', whose parameters() is neither a
                    # Tensor nor a Module there: :66-67,72-74) in eval mode (:52-54,73) -- until the trainer's
                    # ``model.train()`` at the top of the first step undoes it (codes/engine.py:51; Trainer.update)
                    if name != 'all':
                        m.eval()
            params = target.parameters()
        else:
            params = [target]
        for p in params:
            count += p.numel()
            p.requires_grad = False
    LOG.info('\tFreezed {} parameters'.format(count))
    return model


def _resolve(path, data_dir):
    """A relative path of the config that does not exist from the working directory is looked up under ``--data-dir``
    (the scripts/*.json of the reference name ``map_en-pt_BR.json`` bare; the file lives in ``data/``)."""
    if os.path.isabs(path) or os.path.exists(path) or not data_dir:
        return path
    return os.path.join(data_dir, path)


def finetune_model(model, obj, data_dir=None):
    """Freeze layers and, when the alphabet changes, swap the last FC (training_utils.py:87-122)."""
    freeze_layers = obj.get('freeze_layers', None)
    lang = obj['langs'][0] if 'langs' in obj else obj['lang']
    num_classes = NUM_CLASSES[lang]
    map_fc = obj.get('map_fc', None)
    model = _freeze_layers(model, freeze_layers)
    head = model.fc[0].module
    old = head[1]
    if old.out_features != num_classes or (freeze_layers and freeze_layers[0] == 'all'):
        LOG.info('\tChanging the last FC layer')
        new = _LinearParams(old.in_features, num_classes).to(old.weight.device)
        with torch.no_grad():
            torch.nn.init.normal_(new.weight, 0, 0.01)
            if map_fc is not None:
                LOG.info('\t Mapping FC weights')
                pairs = json.load(open(_resolve(map_fc, data_dir)))
                old_idx, new_idx = zip(*pairs)
                new.weight.index_copy_(0, torch.tensor(new_idx, device=new.weight.device),
                                       old.weight.detach().index_select(0, torch.tensor(old_idx,
                                                                                        device=old.weight.device)))
        head[1] = new
        model._num_classes = num_classes
        model._flat_p = None                 # parameters changed: re-pack lazily
    return model


def get_optimizer(params, obj):
    return getattr(torch.optim, obj.get('name', 'SGD'))(params, **obj.params)


def get_scheduler(optimizer, obj):
    return getattr(torch.optim.lr_scheduler, obj.get('name', 'ExponentialLR'))(optimizer, **obj.params)


def get_per_params_lr(model, obj):
    """Per-layer learning-rate groups (training_utils.py:133-159): [[name, lr], ..., ['base']]."""
    per_layer_lr = obj.get('per_layer_lr', None)
    if per_layer_lr is None:
        return model.parameters()
    groups, taken, has_base = [], set(), False
    for conf in per_layer_lr:
        if conf[0] == 'base':
            has_base = True
            continue
        ps = list(getattr(model, conf[0]).parameters())
        g = {'params': ps}
        if len(conf) > 1:
            g['lr'] = conf[1]
        groups.append(g)
        taken.update(id(p) for p in ps)
    if has_base:
        groups.append({'params': [p for p in model.parameters() if id(p) not in taken]})
    return groups


def _is_deferred(transform):
    """True if no stage of ``transform`` is a waveform loader that decodes on the device per utterance."""
    stages = getattr(transform, 'transforms', [transform])
    return all(getattr(t, 'defer', True) for t in stages if isinstance(t, transforms.ToTensor))


def get_data_loaders(train_transforms, val_transforms, target_transforms, args, raw_audio=True):
    if not isinstance(target_transforms, (list, tuple)):
        target_transforms = [target_transforms]
    if len(target_transforms) != 1:
        return _multitask_loaders(train_transforms, val_transforms, target_transforms, args, raw_audio)
    train_set = AudioDataset(args.data_dir, args.train_manifest[0], train_transforms, target_transforms[0])
    val_set = AudioDataset(args.data_dir, args.val_manifest[0], val_transforms, target_transforms[0])
    bsz = args.config.training.batch_size
    if args.distributed:
        sampler = DistributedBucketingSampler(train_set, batch_size=bsz)
    else:
        sampler = BucketingSampler(train_set, batch_size=bsz)
    pin = bool(raw_audio) and torch.cuda.is_available()     # page-locked int16 batches: asynchronous uploads one bin ahead
    workers = args.num_workers
    if workers > 0 and not all(_is_deferred(t) for t in (train_transforms, val_transforms)):
        # a per-utterance (non-deferred) waveform transform runs device kernels: it cannot live in a forked worker
        LOG.warning('the waveform transforms decode on the GPU per utterance (defer=False): loading with num_workers=0')
        workers = 0
    train_loader = AudioDataLoader(train_set, num_workers=workers, batch_sampler=sampler, raw_audio=raw_audio,
                                   pin_memory=pin)
    val_loader = AudioDataLoader(val_set, batch_size=bsz, num_workers=workers, raw_audio=raw_audio,
                                 pin_memory=pin)
    if raw_audio and torch.cuda.is_available():
        from ..data import DevicePrefetcher
        train_loader, val_loader = DevicePrefetcher(train_loader), DevicePrefetcher(val_loader)
    return train_loader, val_loader


def _multitask_loaders(train_transforms, val_transforms, target_transforms, args, raw_audio):
    """One manifest per language (training_utils.py:160-210): ConcatAudioDataset, ``training.sampling`` (default 'equal')
    through WeightedBucketingRandomSampler, or DistributedBucketingSampler over the concatenation with --distributed."""
    n = len(target_transforms)
    if len(args.train_manifest) != n or len(args.val_manifest) != n:
        raise ValueError('a multi-task config with %d languages needs %d train and %d val manifests' % (n, n, n))
    if not raw_audio and any(_has_waveform_stage(t) for t in (train_transforms, val_transforms)):
        raise ValueError('raw_audio=False needs transforms that end in a spectrogram (gpu_frontend=False)')
    train_set = ConcatAudioDataset([AudioDataset(args.data_dir, m, train_transforms, t)
                                    for m, t in zip(args.train_manifest, target_transforms)])
    val_set = ConcatAudioDataset([AudioDataset(args.data_dir, m, val_transforms, t)
                                  for m, t in zip(args.val_manifest, target_transforms)])
    training = args.config.training
    bsz = training.batch_size
    if args.distributed:
        sampler = DistributedBucketingSampler(train_set, batch_size=bsz)
    else:
        sampler = WeightedBucketingRandomSampler(train_set, batch_size=bsz, sampling=training.get('sampling', 'equal'),
                                                 num_epochs=training.num_epochs)
    workers = args.num_workers
    if workers > 0 and not all(_is_deferred(t) for t in (train_transforms, val_transforms)):
        workers = 0                  # (a per-utterance transform that runs device kernels cannot live in a forked worker)
    pin = bool(raw_audio) and torch.cuda.is_available()
    train_loader = AudioDataLoader(train_set, num_workers=workers, batch_sampler=sampler, num_tasks=n, raw_audio=raw_audio,
                                   pin_memory=pin)
    val_loader = AudioDataLoader(val_set, batch_size=bsz, num_workers=workers, num_tasks=n, raw_audio=raw_audio,
                                 pin_memory=pin)
    if raw_audio and torch.cuda.is_available():         # the same staging as single-task: upload + frontend one bin ahead
        from ..data import DevicePrefetcher
        train_loader, val_loader = DevicePrefetcher(train_loader), DevicePrefetcher(val_loader)
    return train_loader, val_loader


def _has_waveform_stage(transform):
    stages = getattr(transform, 'transforms', [transform])
    return any(isinstance(t, transforms.ToTensor) for t in stages) and \
        not any(isinstance(t, transforms.ToSpectrogram) for t in stages)
