"""CTC forced alignment: when was each character and word of a KNOWN transcript spoken, and how well does it fit
(not in the reference).  The decoders' ``offsets`` time what the model itself would have written; this takes the
transcript as the constraint: ``ds2_ctc_align`` (``csrc/ctc_align.hip``) finds the best single alignment of every
utterance of a minibatch in one launch, and the host part below turns its frames into characters, words and seconds.
"""
import numpy as np
import torch

from ds2hip import ops

from .preprocessing import OrderedLabelEncoder

FRAME_SHIFT_S = 0.01                # the spectrogram's hop: 160 samples at 16 kHz (codes/transforms.py)


def group_words(chars):
    """chars: [(char, start_frame, end_frame)] -> [(word, start, end)]: the runs between spaces, each from its first
    character's start to its last character's end.  Leading, trailing and repeated spaces make no word."""
    words, run = [], []
    for c, s, e in list(chars) + [(' ', -1, -1)]:
        if c == ' ':
            if run:
                words.append((''.join(r[0] for r in run), run[0][1], run[-1][2]))
            run = []
        else:
            run.append((c, s, e))
    return words


class ForcedAligner(object):
    """``align(probs (B,T,A), sizes, targets, target_sizes)`` with the evaluator's tensors (``probs`` on the device, flat
    ``targets``) returns one dict per utterance: ``score`` (log-score of the best alignment, -inf if there is none),
    ``score_per_frame`` (score / frames; the figure to prune mis-transcribed clips by), ``chars`` [(char, start_frame,
    end_frame)] and ``words`` [(word, start_frame, end_frame)], frames inclusive; an utterance without an alignment has
    empty lists.  ``log_input=True`` if ``probs`` are log-probabilities."""

    def __init__(self, label_encoder, blank_index=0, log_input=False):
        if isinstance(label_encoder, str):
            label_encoder = list(label_encoder)
        if isinstance(label_encoder, (set, list)):
            label_encoder = OrderedLabelEncoder().fit(label_encoder)
        self.label_encoder = label_encoder
        self.blank_index, self.log_input = int(blank_index), bool(log_input)

    @staticmethod
    def frame_to_seconds(t):
        """Centre of the model's output step ``t`` in seconds: (2 t + 5) * 0.01.

        conv2 (time stride 1, 11 taps, no padding) centres step t on conv1 step t + 5; conv1 (time stride 2, padding 10,
        11 taps) centres its step u on spectrogram frame 2 u - 10 + 5 = 2 u - 5; so step t sits on frame 2 (t + 5) - 5 =
        2 t + 5.  Spectrogram frames are 10 ms apart and centred on their sample (``center=True``), so frame f is at
        f * 0.01 s and the resolution is 20 ms.  The same geometry gives ``ops.conv_out_frames``: t1 = (t_in + 20 - 11)
        // 2 + 1 conv1 steps and t1 - 10 output steps; with 2 t1 <= t_in + 11 the last step's centre 2 (t1 - 11) + 5 is at
        most frame t_in - 6, so every centre lies inside the clip."""
        return (2 * int(t) + 5) * FRAME_SHIFT_S

    def _chars(self, labels, starts, ends):
        if len(labels) == 0:
            return []
        text = self.label_encoder.inverse_transform(labels)
        return [(str(c), int(s), int(e)) for c, s, e in zip(text, starts, ends)]

    def align(self, probs, sizes, targets, target_sizes):
        if not probs.is_cuda:
            raise RuntimeError('ForcedAligner.align runs on device tensors only')
        dev = probs.device
        bsz = probs.shape[0]
        lens_h = torch.as_tensor(target_sizes).to('cpu', torch.int32).reshape(-1)
        offs_h = torch.cumsum(lens_h, 0, dtype=torch.int32) - lens_h
        lmax = int(lens_h.max()) if bsz else 0
        sizes_h = torch.as_tensor(sizes).to('cpu', torch.int32).reshape(-1)
        targets_h = torch.as_tensor(targets).to('cpu', torch.int32).reshape(-1)
        states, starts, ends, score = ops.ctc_align(
            probs.detach().contiguous().float(), sizes_h.to(dev), targets_h.to(dev), offs_h.to(dev), lens_h.to(dev), lmax,
            self.blank_index, self.log_input)
        starts, ends, score = starts.cpu().numpy(), ends.cpu().numpy(), score.cpu().numpy()
        targets_n, t_max = targets_h.numpy(), int(probs.shape[1])
        out = []
        for b in range(bsz):
            n, o = int(lens_h[b]), int(offs_h[b])
            frames = min(max(int(sizes_h[b]), 0), t_max)
            sc = float(score[b])
            chars = self._chars(targets_n[o:o + n], starts[b, :n], ends[b, :n]) if np.isfinite(sc) else []
            out.append({'score': sc, 'score_per_frame': sc / max(frames, 1), 'chars': chars, 'words': group_words(chars)})
        return out
