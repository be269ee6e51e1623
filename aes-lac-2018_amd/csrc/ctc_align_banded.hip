// Banded CTC forced alignment: ds2_ctc_align's max-sum recursion restricted to a moving band of W states per frame, so that
// work and workspace are T x W instead of T x (2 L + 1) -- an hour of audio against its whole transcript in one launch.
//
// One workgroup per utterance, ONE launch, no workgroup waits on another.  Everything that ctc_align.hip says about the
// recursion, its fp64 scores and the per-frame term holds here, and the shared parts are ctc_path_common.h's; what differs:
//   band        at frame t the admissible states are lo[t] <= s < lo[t] + W (and s < S = 2 L + 1).  State s lives in SLOT
//               s mod W of the score row and of the frame's W back-pointer bytes, so a band that slides moves no data: the
//               slot of a state that leaves the band is taken over by the state W above it.  Thread tid owns the slots
//               tid + NTHR k, k < K = W / NTHR (lane-contiguous, so the three LDS reads per state are conflict-free and the
//               pointer bytes of a wave are one 64-byte run).  The state a slot holds follows from lo[t] alone:
//               s = lo[t] + ((slot - lo[t]) mod W).
//   predecessors s - d (d = 0, 1, 2) of frame t - 1 are read from slot (slot - d) mod W and count only if
//               lo[t-1] <= s - d < lo[t-1] + W: otherwise that slot holds another state's score (or nothing) and the
//               predecessor is -inf, as the definition (the full recursion with inadmissible cells forced to -inf) has it.
//               Nothing needs resetting.  Frame 0 reads the virtual row {state 0: 0, rest -inf} with band [0, W).
//   lo          staged through LDS with the emissions, a chunk of frames ahead; every thread reads the frame's value (a
//               broadcast) and compares it with the previous frame's: lo < 0, a decrease, a step of W or more (two bands
//               that share no state) or lo >= S (a band that admits no state) ends the recursion for the whole workgroup
//               at once -- "no alignment".
//   symbols     a thread keeps the symbol and the skip flag of each of its K states in registers and re-reads them from
//               labels (L2-resident) only when the band's movement puts another state into that slot.
//   score       float64: an hour's path score is about -1e5.
// Score rows: 2 x W doubles of dynamic LDS (128 KiB at W = 8192; the static part is 17 KiB).
// Critical path: T barriers per utterance, then T dependent LDS reads of one thread.
//
// GAP = true is ds2_ctc_align_banded_gap (include/ds2hip.h, "banded CTC alignment with gaps"): the same states, band, scores
// and ties; only the EMISSION of the eligible blank states (the two end blanks and the blanks beside a space label) differs:
// it is max(lp[t][blank], f[t]) with f[t] = max_a lp[t][a] - gap_penalty, and a frame where f[t] wins strictly is a gap frame.
//   mrow        f[t] of the staged chunk's frames, computed from the chunk's emissions in LDS once per chunk, 8 lanes per
//               frame (one more barrier per chunk, none per frame); every thread reads the frame's value as a broadcast.
//   eligibility bit 9 of symskip[k], set with the symbol when the slot takes over a state (a blank slot then reads the two
//               labels beside it, where the plain form reads none).
//   gap flag    bit 2 of the back-pointer byte (code | gap << 2), written by the recursion; the back-trace steps by
//               (byte & 3) and writes gap[t] from the byte of the state it walks through.
// The GAP = false instantiations contain none of this.
#include "ctc_path_common.h"

namespace {

using namespace ctc_path;

constexpr int BAND_MIN = DS2_ALIGN_BAND_MIN, BAND_MAX = DS2_ALIGN_BAND_MAX;

template <int W, int NTHR, int K, bool GAP>
__global__ __launch_bounds__(NTHR) void ctc_align_banded_kernel(
    const float* __restrict__ probs, const int32_t* __restrict__ sizes, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ label_lens, const int32_t* __restrict__ lo_all,
    int T, int A, int lmax, int blank, int log_input, uint8_t* bp_all, int32_t* __restrict__ states,
    int32_t* __restrict__ starts, int32_t* __restrict__ ends, double* __restrict__ score, int space, float gap_penalty,
    uint8_t* __restrict__ gap_all) {
    static_assert(NTHR * K == W || (K == 1 && NTHR > W), "every slot has one owner");
    extern __shared__ double rowbuf[];   // [2][W], slot = state mod W
    __shared__ float em[2][EM_FLOATS];
    __shared__ int lo_s[2][MAX_CH];
    __shared__ float mrow[GAP ? 2 : 1][GAP ? MAX_CH : 1];   // GAP: f[t] = max_a lp[t][a] - gap_penalty of the staged frames
    __shared__ int bad;

    const int tid = threadIdx.x;
    const AlignUtt u = align_prologue<NTHR, GAP>(sizes, labels, label_offsets, label_lens, T, A, lmax, blank, states, starts,
                                                 ends, gap_all, bad);
    const int tl = u.tl, S = u.S;
    const int32_t* lab = u.lab;
    for (int i = tid; i < W; i += NTHR) {
        rowbuf[i] = (i == 0) ? 0.0 : NEG_INF;               // the virtual row before frame 0
        rowbuf[W + i] = NEG_INF;
    }
    __syncthreads();

    uint8_t* bp = bp_all + (size_t)blockIdx.x * T * W;
    double final_v = NEG_INF;
    int final_s = -1;
    const bool ok = !bad;
    if (ok && tl > 0) {
        int held[K], symskip[K];                            // the state each owned slot holds; its symbol | skip << 8 | eligible << 9
#pragma unroll
        for (int k = 0; k < K; ++k) held[k] = -1, symskip[k] = 0;
        // staging roles besides the stager's: thread tid < CH carries the chunk's lo[tid]
        ChunkStager stage(probs + (size_t)blockIdx.x * T * A, tid, tl, A);
        const int CH = stage.CH, nchunk = stage.nchunk;
        const int32_t* lo_row = lo_all + (size_t)blockIdx.x * T;
        int rlo = 0;
        const auto term = [&](float a, int) { return log_input ? a : logf(a); };   // log 0 = -inf, log of a negative = NaN
        auto stage_load = [&](int c) {
            stage.load(c);
            rlo = 0;
            if (tid < CH && c * CH + tid < tl) rlo = lo_row[c * CH + tid];
        };
        auto stage_store = [&](int buf) {
            stage.store(em[buf], term);
            if (tid < CH) lo_s[buf][tid] = rlo;
        };
        stage_load(0);
        stage_store(0);
        __syncthreads();
        int cur = 0, t = 0, lo_prev = 0;
        bool dead = false;
        for (int c = 0; c < nchunk && !dead; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) stage_load(c + 1);                    // in flight while this chunk's frames are worked on
            const int fend = min(CH, tl - c * CH);
            if constexpr (GAP) {
                // (the chunk's emissions are behind the barrier that ended the last chunk; mrow[c & 1]'s last readers were in
                // chunk c - 2)
                // 8 lanes per frame (threads 0..255 are four whole waves at every NTHR), then an xor butterfly: one thread per
                // frame would put A dependent LDS reads in front of the chunk's first frame (measured: DESIGN.md)
                if (tid < 8 * MAX_CH) {
                    const int r = tid >> 3, part = tid & 7;
                    float m = -INFINITY;                    // (no NaN in em)
                    if (r < fend)
                        for (int a = part; a < A; a += 8) m = fmaxf(m, em[c & 1][r * A + a]);
                    m = fmaxf(m, __shfl_xor(m, 1));
                    m = fmaxf(m, __shfl_xor(m, 2));
                    m = fmaxf(m, __shfl_xor(m, 4));
                    if (part == 0 && r < fend) mrow[c & 1][r] = (m == -INFINITY) ? -INFINITY : m - gap_penalty;
                }
                __syncthreads();
            }
            for (int f = 0; f < fend; ++f) {
                const int lo_t = lo_s[c & 1][f];
                if (lo_t < lo_prev || lo_t >= S || lo_t - lo_prev >= W) {   // the same value in every thread: all leave together
                    dead = true;
                    break;
                }
                const double* prev = rowbuf + cur * W;
                double* nxt = rowbuf + (cur ^ 1) * W;
                const float* e = em[c & 1] + f * A;
                float fgap = 0.f;
                if constexpr (GAP) fgap = mrow[c & 1][f];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int j = tid + NTHR * k;
                    const unsigned su = (unsigned)lo_t + (unsigned)((j - lo_t) & (W - 1));
                    if ((NTHR <= W || j < W) && su < (unsigned)S) {
                        const int s = (int)su;
                        if (s != held[k]) {
                            int sym = blank, skip = 0, elig = 0;
                            if (s & 1) {
                                sym = lab[s >> 1];
                                skip = s >= 3 && sym != lab[(s >> 1) - 1];
                            } else if constexpr (GAP) {     // (0 < s < 2 L: labels s/2 - 1 and s/2 both exist)
                                elig = s == 0 || s == S - 1 || lab[(s >> 1) - 1] == space || lab[s >> 1] == space;
                            }
                            held[k] = s;
                            symskip[k] = sym | (skip << 8) | (elig << 9);
                        }
                        const int d = s - lo_prev;          // >= 0; the predecessor s - i is in frame t-1's band iff d - i is in 0..W-1
                        const double r0 = prev[j], r1 = prev[(j - 1) & (W - 1)], r2 = prev[(j - 2) & (W - 1)];
                        float ev = e[symskip[k] & 255];
                        int gapf = 0;
                        if constexpr (GAP) {
                            gapf = ((symskip[k] >> 9) & 1) && fgap > ev;            // strict, in fp32
                            ev = gapf ? fgap : ev;
                        }
                        const double x0 = (unsigned)d < (unsigned)W ? r0 : NEG_INF;
                        const double x1 = (unsigned)(d - 1) < (unsigned)W ? r1 : NEG_INF;
                        const double x2 = (((symskip[k] >> 8) & (GAP ? 1 : -1)) && (unsigned)(d - 2) < (unsigned)W) ? r2 : NEG_INF;
                        double best = x0;                   // the tie rule, written out: profiles/align_refactor.md, "Time"
                        int code = 0;
                        if (x1 > best) {
                            best = x1;
                            code = 1;
                        }
                        if (x2 > best) {
                            best = x2;
                            code = 2;
                        }
                        nxt[j] = (best == NEG_INF) ? NEG_INF : best + (double)ev;
                        bp[(size_t)t * W + j] = (uint8_t)(GAP ? code | (gapf << 2) : code);
                    }
                }
                if (more && f == fend - 1) stage_store((c + 1) & 1);    // (its last readers passed chunk c - 1's final barrier)
                __syncthreads();
                cur ^= 1;
                ++t;
                lo_prev = lo_t;
            }
        }
        if (!dead) {
            // every thread reads the same two cells: S-1 first, S-2 only if strictly better; each only inside the last band
            const double* last = rowbuf + cur * W;
            const int d = S - 1 - lo_prev;
            if ((unsigned)d < (unsigned)W) {
                final_v = last[(S - 1) & (W - 1)];
                final_s = S - 1;
            }
            if (S > 1 && (unsigned)(d - 1) < (unsigned)W && last[(S - 2) & (W - 1)] > final_v) {
                final_v = last[(S - 2) & (W - 1)];
                final_s = S - 2;
            }
        }
    }
    const bool has_path = align_has_path<NTHR, GAP>(u, ok, final_v);
    if (tid == 0) score[blockIdx.x] = final_v == final_v ? final_v : NEG_INF;
    // A state on the path is in its frame's band, so its byte is the one in slot (state mod W) of that frame; the window's other
    // bytes are never walked.
    if (has_path) align_backtrace<NTHR, GAP>(u, bp, W, W - 1, final_s);
}

template <int W, int NTHR, int K, bool GAP>
int launch(const char* fn, int B, hipStream_t st, const float* probs, const int32_t* sizes, const int32_t* labels,
           const int32_t* label_offsets, const int32_t* label_lens, const int32_t* lo, int T, int A, int lmax, int blank,
           int log_input, uint8_t* ws, int32_t* states, int32_t* starts, int32_t* ends, double* score, int space,
           float gap_penalty, uint8_t* gap) {
    auto kernel = ctc_align_banded_kernel<W, NTHR, K, GAP>;
    const size_t dyn = (size_t)2 * W * sizeof(double);
    if (dyn + 20 * 1024 > 64 * 1024 &&                      // (the static part is 17 KiB)
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) !=
            hipSuccess) {
        ds2_set_error("%s: %zu bytes of dynamic LDS are not available (band %d)", fn, dyn, W);
        return DS2_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kernel, dim3(B), dim3(NTHR), dyn, st, probs, sizes, labels, label_offsets, label_lens, lo, T, A, lmax,
                       blank, log_input, ws, states, starts, ends, score, space, gap_penalty, gap);
    return DS2_OK;
}

// the checks and the dispatch of both entry points; GAP picks the instantiation, fn names the entry in messages
template <bool GAP>
int run(const char* fn, const float* probs, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
        const int32_t* label_lens, const int32_t* lo, int B, int T, int A, int max_label_len, int band, int blank, int space,
        float gap_penalty, int log_input, void* ws, size_t ws_bytes, int32_t* states, int32_t* starts, int32_t* ends,
        uint8_t* gap, double* score, void* stream) {
    if (band < BAND_MIN || band > BAND_MAX || (band & (band - 1)) != 0) {
        ds2_set_error("%s: band %d is not a power of two in %d..%d", fn, band, BAND_MIN, BAND_MAX);
        return DS2_ERR_ARG;
    }
    if (max_label_len < 0 || max_label_len > (INT32_MAX - 1) / 2) {
        ds2_set_error("%s: max_label_len %d is outside 0..%d (2 L + 1 states are counted in an int32)", fn, max_label_len,
                      (INT32_MAX - 1) / 2);
        return DS2_ERR_ARG;
    }
    int rc = check_align_args(fn, true, GAP, probs, sizes, label_offsets, label_lens, lo, B, T, A, max_label_len, blank, space,
                              gap_penalty, ws, ws_bytes, ds2_ctc_align_banded_ws_bytes(B, T, band), states, starts, ends, gap,
                              score);
    if (rc != DS2_OK || B == 0) return rc;
#define DS2_BANDED(W_, N_, K_)                                                                                         \
    rc = launch<W_, N_, K_, GAP>(fn, B, (hipStream_t)stream, probs, sizes, labels, label_offsets, label_lens, lo, T, A, \
                                 max_label_len, blank, log_input, (uint8_t*)ws, states, starts, ends, score, space,    \
                                 gap_penalty, gap)
    switch (band) {
        case 64: DS2_BANDED(64, 256, 1); break;
        case 128: DS2_BANDED(128, 256, 1); break;
        case 256: DS2_BANDED(256, 256, 1); break;
        case 512: DS2_BANDED(512, 512, 1); break;
        case 1024: DS2_BANDED(1024, 1024, 1); break;
        case 2048: DS2_BANDED(2048, 1024, 2); break;
        case 4096: DS2_BANDED(4096, 1024, 4); break;
        default: DS2_BANDED(8192, 1024, 8); break;
    }
#undef DS2_BANDED
    if (rc != DS2_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ds2_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
        return DS2_ERR_LAUNCH;
    }
    return DS2_OK;
}

}  // namespace

extern "C" size_t ds2_ctc_align_banded_ws_bytes(int B, int T, int band) {
    if (B < 0 || T < 0 || band < 0) return 0;
    return (size_t)B * T * band + 16;
}

extern "C" int ds2_ctc_align_banded(const float* probs, const int32_t* sizes, const int32_t* labels,
                                    const int32_t* label_offsets, const int32_t* label_lens, const int32_t* lo, int B, int T,
                                    int A, int max_label_len, int band, int blank, int log_input, void* ws, size_t ws_bytes,
                                    int32_t* states, int32_t* starts, int32_t* ends, double* score, void* stream) {
    return run<false>("ds2_ctc_align_banded", probs, sizes, labels, label_offsets, label_lens, lo, B, T, A, max_label_len, band,
                      blank, -1, 0.f, log_input, ws, ws_bytes, states, starts, ends, nullptr, score, stream);
}

// the gap form keeps the same back-pointer bytes (the gap flag is a spare bit of each), so the same workspace
extern "C" size_t ds2_ctc_align_banded_gap_ws_bytes(int B, int T, int band) {
    return ds2_ctc_align_banded_ws_bytes(B, T, band);
}

extern "C" int ds2_ctc_align_banded_gap(const float* probs, const int32_t* sizes, const int32_t* labels,
                                        const int32_t* label_offsets, const int32_t* label_lens, const int32_t* lo, int B,
                                        int T, int A, int max_label_len, int band, int blank, int space, float gap_penalty,
                                        int log_input, void* ws, size_t ws_bytes, int32_t* states, int32_t* starts,
                                        int32_t* ends, uint8_t* gap, double* score, void* stream) {
    return run<true>("ds2_ctc_align_banded_gap", probs, sizes, labels, label_offsets, label_lens, lo, B, T, A, max_label_len,
                     band, blank, space, gap_penalty, log_input, ws, ws_bytes, states, starts, ends, gap, score, stream);
}
