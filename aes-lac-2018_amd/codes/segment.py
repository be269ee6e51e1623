"""Cutting a recording of any length into the clips the model was trained on (not in the reference, which cuts its
corpora with dataset scripts and sox).  ``Segmenter`` turns seconds, decibels and a percentile into the blocks, level bins
and rank of ``ds2_vad_segment`` (``csrc/vad.hip``; the rule is written down in ``include/ds2hip.h``) and runs it on the
int16 samples already on the device: an energy threshold above the recording's own noise floor, short gaps closed, short
blips dropped, the rest padded and split at its quietest block when it is longer than ``max_segment``."""
import math

import numpy as np
import torch

from ds2hip import ops

BLOCK = ops.VAD_BLOCK                      # samples per block: 10 ms at 16 kHz
SAMPLE_RATE = 16000
BLOCKS_PER_S = SAMPLE_RATE // BLOCK        # 100
FULL_SCALE = 3 * BLOCK * 32768 ** 2        # a full-scale square over the 480 samples of S[j]: 0 dBFS
DB_PER_BIN = 0.7526                        # a quarter octave of energy: 10 log10(2) / 4


def level_bin(s):
    """The kernel's level bin of an energy S (Python int): S below 4, else 4 floor(log2 S) + the next two bits."""
    s = int(s)
    if s < 4:
        return s
    e = s.bit_length() - 1
    return 4 * e + ((s >> (e - 2)) & 3)


def db_to_bin(db):
    """dBFS (relative to a full-scale square over 480 samples) -> level bin: -60 -> 75, -30 -> 115."""
    return level_bin(math.ceil(FULL_SCALE * 10.0 ** (float(db) / 10.0)))


def bin_to_db(k):
    """The lower edge of level bin ``k`` in dBFS (None for bin 0, whose lower edge is silence)."""
    k = int(k)
    low = k if k < 4 else (4 if k < 8 else (4 + k % 4) << (k // 4 - 2))
    return None if low == 0 else 10.0 * math.log10(low / float(FULL_SCALE))


def seconds_to_blocks(seconds):
    return int(round(BLOCKS_PER_S * float(seconds)))


class Segmenter(object):
    """``segment(pcm)`` -> ``(segments, stats)``: segments (n_seg, 2) int64 numpy, [first sample, end sample) in ascending
    order; stats = {blocks (n_seg, 2) the same in 10 ms blocks, noise_floor_db, threshold_db (lower edges of their level
    bins), speech_seconds (speech after gap closing and blip removal, before padding), nb}.

    max_segment / min_speech / min_silence / pad in seconds (rounded to 10 ms blocks); ``percentile`` the share of blocks
    taken as the noise floor; ``margin_db`` what speech must exceed it by; ``min_db`` / ``max_db`` clamp the threshold
    (``max_db`` is what lets a recording that is speech throughout still count as speech).  Nobody has measured what the
    defaults do to WER on any corpus."""

    def __init__(self, max_segment=15.0, min_speech=0.25, min_silence=0.3, pad=0.1, percentile=0.1, margin_db=12.0,
                 min_db=-60.0, max_db=-30.0):
        self.max_len = seconds_to_blocks(max_segment)
        self.min_speech = seconds_to_blocks(min_speech)
        self.min_silence = seconds_to_blocks(min_silence)
        self.pad = seconds_to_blocks(pad)
        self.percentile = float(percentile)
        self.margin_bins = int(round(float(margin_db) / DB_PER_BIN))
        if not -200.0 <= float(min_db) <= 20.0:
            raise ValueError('Segmenter: min_db = %r is no level in dBFS' % (min_db,))
        if not -200.0 <= float(max_db) <= 20.0:
            raise ValueError('Segmenter: max_db = %r is no level in dBFS' % (max_db,))
        self.min_bin, self.max_bin = db_to_bin(min_db), db_to_bin(max_db)
        if self.max_len < 4:
            raise ValueError('Segmenter: max_segment = %r s is shorter than 4 blocks of 10 ms' % (max_segment,))
        if self.min_speech < 2:
            raise ValueError('Segmenter: min_speech = %r s is shorter than 2 blocks of 10 ms' % (min_speech,))
        if self.pad < 0:
            raise ValueError('Segmenter: pad = %r s is negative' % (pad,))
        if 2 * self.pad >= self.min_silence:
            raise ValueError('Segmenter: min_silence = %r s must be longer than twice pad = %r s, or padded segments could '
                             'touch' % (min_silence, pad))
        if not 0.0 <= self.percentile <= 1.0:
            raise ValueError('Segmenter: percentile = %r is outside 0 .. 1' % (percentile,))
        if not 0 <= self.margin_bins < ops.VAD_BINS:
            raise ValueError('Segmenter: margin_db = %r is outside 0 .. %.0f dB' % (margin_db, DB_PER_BIN * ops.VAD_BINS))
        for name, db, k in (('min_db', min_db, self.min_bin), ('max_db', max_db, self.max_bin)):
            if not 0 <= k < ops.VAD_BINS:
                raise ValueError('Segmenter: %s = %r dBFS has no level bin' % (name, db))

    def rank(self, nb):
        return max(min(nb - 1, int(math.floor(self.percentile * nb))), 0)

    def segment(self, pcm, device='cuda'):
        if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16 or pcm.dim() != 1:
            raise ValueError('Segmenter.segment takes a 1-D int16 tensor (16 kHz mono samples)')
        if not pcm.is_cuda:
            pcm = pcm.to(device)
        n = int(pcm.numel())
        nb = (n + BLOCK - 1) // BLOCK
        segs, info = ops.vad_segment(pcm.contiguous(), self.rank(nb), self.margin_bins, self.min_bin, self.max_bin,
                                     self.min_speech, self.min_silence, self.pad, self.max_len)
        blocks = segs.numpy().astype(np.int64)
        samples = np.minimum(blocks * BLOCK, n)
        return samples, {'blocks': blocks, 'noise_floor_db': bin_to_db(info['floor_bin']) if n else None,
                         'threshold_db': bin_to_db(info['thr']) if n else None,
                         'speech_seconds': info['speech_blocks'] / float(BLOCKS_PER_S), 'nb': info['nb']}
