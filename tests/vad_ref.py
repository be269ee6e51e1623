"""The segmentation rule of include/ds2hip.h ("voice-activity segmentation", steps 1-8) restated in numpy and Python
integers, from the header's text and not from the kernel.  ``vad_ref`` returns the segments, ``info`` and the masks after
steps 3, 4 and 5, so a test can assert that a case really sits on the edge it is meant to sit on."""
import numpy as np

BLOCK = 160
BINS = 192


def level_bin(s):
    s = int(s)
    if s < 4:
        return s
    e = s.bit_length() - 1
    return 4 * e + ((s >> (e - 2)) & 3)


def block_energies(pcm):
    """(E, S): exact Python-int energies of the blocks and of every block with its two neighbours."""
    x = np.asarray(pcm, dtype=np.int16).astype(np.int64).reshape(-1)
    nb = -(-len(x) // BLOCK)
    padded = np.zeros(nb * BLOCK, np.int64)
    padded[:len(x)] = x
    e = [int(v) for v in (padded * padded).reshape(nb, BLOCK).sum(axis=1)]             # at most 160 * 2^30: exact in int64
    s = [(e[j - 1] if j > 0 else 0) + e[j] + (e[j + 1] if j + 1 < nb else 0) for j in range(nb)]
    return e, s


def runs(mask, value):
    """Maximal runs [s, e) of ``value`` in a 0/1 list."""
    out, j, n = [], 0, len(mask)
    while j < n:
        if mask[j] == value:
            k = j
            while k < n and mask[k] == value:
                k += 1
            out.append((j, k))
            j = k
        else:
            j += 1
    return out


def vad_ref(pcm, rank, margin_bins, min_bin, max_bin, min_speech, min_silence, pad, max_len):
    """-> dict(segs (n_seg, 2) int32, info [8], S, bins, m3, m4, m5)."""
    n = len(pcm)
    if n == 0:
        return {'segs': np.zeros((0, 2), np.int32), 'info': [0] * 8, 'S': [], 'bins': [], 'm3': [], 'm4': [], 'm5': []}
    _, s_all = block_energies(pcm)
    nb = len(s_all)
    bins = [level_bin(s) for s in s_all]
    hist = [0] * BINS
    for b in bins:
        hist[b] += 1
    cum, floor_bin = 0, None
    for k in range(BINS):
        cum += hist[k]
        if cum > rank:
            floor_bin = k
            break
    thr = min(max(floor_bin + margin_bins, min_bin), max_bin)
    m3 = [int(b >= thr) for b in bins]
    m4 = list(m3)
    for s, e in runs(m3, 0):                                         # step 4
        if e - s < min_silence and s > 0 and e < nb:
            m4[s:e] = [1] * (e - s)
    m5 = list(m4)
    for s, e in runs(m4, 1):                                         # step 5
        if e - s < min_speech:
            m5[s:e] = [0] * (e - s)
    h = (max_len + 1) // 2
    segs = []
    for s, e in runs(m5, 1):
        s, e = max(0, s - pad), min(nb, e + pad)                     # step 6
        while e - s > max_len:                                       # step 7
            lo, hi = s + h, min(s + max_len, e - h)
            c = min(range(lo, hi + 1), key=lambda i: (s_all[i], i))
            segs.append((s, c))
            s = c
        segs.append((s, e))
    info = [len(segs), floor_bin, thr, sum(m5), nb, 0, 0, 0]
    return {'segs': np.asarray(segs, np.int32).reshape(-1, 2), 'info': info, 'S': s_all, 'bins': bins, 'm3': m3, 'm4': m4,
            'm5': m5}


def pcm_from_blocks(loud, amp=1000, last=BLOCK):
    """int16 samples of a block pattern: block j holds ``amp`` (a number, or one per block) where ``loud[j]`` is set and 0
    elsewhere; the last block has ``last`` samples."""
    loud = np.asarray(loud)
    amps = np.broadcast_to(np.asarray(amp, np.int64), loud.shape)
    x = np.repeat(np.where(loud != 0, amps, 0), BLOCK).astype(np.int16)
    return x[:len(x) - (BLOCK - last)]


def six_clip_recording():
    """The six clips of tests/test_cli_gpu.py:_corpus (white noise at -20 dBFS, 16000 + 1700 i samples, one generator seeded
    with 0) joined by 0.6 s of -60 dBFS noise, with the same before the first and after the last.
    -> (int16 samples, [(first sample, end sample) of every clip])."""
    rng = np.random.default_rng(0)
    clips = [(np.clip(0.1 * rng.standard_normal(16000 + 1700 * i), -1, 1) * 32767).astype(np.int16) for i in range(6)]
    quiet = np.random.default_rng(1)
    parts, at, bounds = [], 0, []
    for c in clips:
        parts.append(np.rint(32.767 * quiet.standard_normal(9600)).astype(np.int16))
        at += 9600
        bounds.append((at, at + len(c)))
        parts.append(c)
        at += len(c)
    parts.append(np.rint(32.767 * quiet.standard_normal(9600)).astype(np.int16))
    return np.concatenate(parts), bounds
