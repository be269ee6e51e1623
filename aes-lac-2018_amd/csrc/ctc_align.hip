// CTC forced alignment (max-sum / Viterbi over the transcript's extended sequence) with back-trace, gfx950.
//
// One workgroup per utterance, one state per thread (256 / 512 / 1024 threads for up to that many of the 2 L + 1 states
// blank, l1, blank, ..., lL, blank of the minibatch's longest transcript), ONE launch:
//   recursion   v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if ext[s] is a label != ext[s-2]) + e[t][ext[s]], carried
//               in fp64; e is the input itself (log_input) or its fp32 log, NaN -> -inf.  Ties: stay, then s-1, then s-2
//               (strict > in that order), at the end S-1 before S-2 -- part of the contract, so a result is bit-reproducible
//               and independent of the rest of the batch.  The row lives in LDS, double-buffered, one barrier per frame;
//               emissions are staged through LDS a chunk of frames at a time and loaded a chunk ahead, as in ctc.hip
//               (probs is (B,T,A) here, so a chunk is one contiguous run of floats).  Frame 0 runs through the same loop
//               from a virtual row {0, -inf, ...}, which admits exactly states 0 and 1.
//   pointers    one byte per (t, s) (0 stay / 1 / 2) to the caller's workspace, lane-contiguous byte stores nothing waits for.
//   back-trace  after a device-scope fence and a barrier: BT_F frames at a time, from the last frame down.  The path
//               descends by at most 2 states per frame, so the BT_F x BT_W window of pointer bytes below the state the path
//               has at the chunk's last frame holds every byte the walk can touch: all threads load it into LDS with
//               independent loads, thread 0 walks it there, all threads write states / starts / ends.  T / BT_F global
//               round trips instead of T dependent ones.
// Critical path: T barriers per utterance, then T dependent LDS reads of one thread.
#include "ds2_common.h"

namespace {

constexpr int MAX_S = 1024;              // 2 L + 1 <= 1023
constexpr int EM_FLOATS = 1024;          // per staging buffer: CH = min(32, 1024 / A) frames
constexpr int EM_NLD = 4;                // staging loads per thread and chunk (threads 0..255 do the staging)
constexpr int MAX_A = 256;               // CH >= 4
constexpr int BT_F = 64;                 // back-trace: frames per window
constexpr int BT_W = 2 * BT_F;           // ... and states per window row (the walk needs 2 (BT_F - 1) + 1)
#define NEG_INF_D (-(double)INFINITY)

// row stride of the back-pointer bytes
inline size_t bp_stride(int max_label_len) { return ((size_t)2 * max_label_len + 1 + 15) & ~(size_t)15; }

template <int NTHR>
__global__ __launch_bounds__(NTHR) void ctc_align_kernel(
    const float* __restrict__ probs, const int32_t* __restrict__ sizes, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ label_lens, int T, int A, int lmax, int blank,
    int log_input, uint8_t* bp_all, size_t sp, int32_t* __restrict__ states, int32_t* __restrict__ starts,
    int32_t* __restrict__ ends, float* __restrict__ score) {
    __shared__ int ext[MAX_S];
    __shared__ double rowbuf[2][MAX_S + 4];
    __shared__ float em[2][EM_FLOATS];
    __shared__ uint8_t win[BT_F][BT_W];
    __shared__ int path[BT_F + 2];       // path[1 + f] = state at frame t_lo + f; [0] / [n + 1] = the frames around the window
    __shared__ int bad;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lraw = label_lens[b];
    const bool len_ok = Lraw >= 0 && Lraw <= lmax;
    const int L = len_ok ? Lraw : 0;
    const int tl = min(max(sizes[b], 0), T);
    const int S = 2 * L + 1;
    if (tid == 0) bad = len_ok ? 0 : 1;
    __syncthreads();
    const int32_t* lab = labels + label_offsets[b];
    for (int s = tid; s < S; s += NTHR) {
        int sym = blank;
        if (s & 1) {
            sym = lab[s >> 1];
            if (sym < 0 || sym >= A || sym == blank) {      // reported as infeasible, never used as an index
                sym = blank;
                bad = 1;
            }
        }
        ext[s] = sym;
    }
    for (int i = tid; i < MAX_S + 4; i += NTHR) {
        rowbuf[0][i] = (i == 2) ? 0.0 : NEG_INF_D;          // cell s + 2 holds state s; cells 0, 1 stay -inf guards
        rowbuf[1][i] = NEG_INF_D;
    }
    __syncthreads();

    int32_t* st_out = states + (size_t)b * T;
    int32_t* start_out = starts + (size_t)b * lmax;
    int32_t* end_out = ends + (size_t)b * lmax;
    for (int t = tl + tid; t < T; t += NTHR) st_out[t] = -1;
    for (int l = L + tid; l < lmax; l += NTHR) start_out[l] = end_out[l] = -1;

    uint8_t* bp = bp_all + (size_t)b * T * sp;
    const int s = tid;
    const bool live = s < S;
    double final_v = NEG_INF_D;
    int final_s = -1;
    if (!bad && tl > 0) {
        const int sym = live ? ext[s] : 0;
        const bool skip = live && s >= 2 && (s & 1) && ext[s] != ext[s - 2];
        // staging roles: thread tid < 256 carries elements idx = tid + 256 i of a chunk (CH frames of A floats, contiguous)
        const int CH = min(32, EM_FLOATS / A), nper = CH * A;
        const int nchunk = (tl + CH - 1) / CH;
        const float* pb = probs + (size_t)b * T * A;
        float ra[EM_NLD];
        auto stage_load = [&](int c) {
            const int left = (tl - c * CH) * A;             // floats of valid frames from this chunk's start on
#pragma unroll
            for (int i = 0; i < EM_NLD; ++i) {
                const int idx = tid + 256 * i;
                ra[i] = 0.f;
                if (tid < 256 && idx < nper && idx < left) ra[i] = pb[(size_t)c * nper + idx];
            }
        };
        auto stage_store = [&](float* dst) {
#pragma unroll
            for (int i = 0; i < EM_NLD; ++i) {
                const int idx = tid + 256 * i;
                if (tid < 256 && idx < nper) {
                    float a = ra[i];
                    asm volatile("" : "+v"(a));             // keeps the wait for the loads HERE, at the chunk's last frame
                    if (!log_input) a = logf(a);            // log 0 = -inf, log of a negative = NaN
                    dst[idx] = (a == a) ? a : -INFINITY;
                }
            }
        };
        stage_load(0);
        stage_store(em[0]);
        __syncthreads();
        int cur = 0, t = 0;
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) stage_load(c + 1);                    // in flight while this chunk's frames are worked on
            const float* e = em[c & 1] + sym;
            const int fend = min(CH, tl - c * CH);
            for (int f = 0; f < fend; ++f) {
                const double* prev = rowbuf[cur];
                double* nxt = rowbuf[cur ^ 1];
                if (live) {
                    const double x0 = prev[s + 2], x1 = prev[s + 1], x2r = prev[s];
                    const float ev = e[f * A];
                    const double x2 = skip ? x2r : NEG_INF_D;
                    double best = x0;
                    int code = 0;
                    if (x1 > best) {
                        best = x1;
                        code = 1;
                    }
                    if (x2 > best) {
                        best = x2;
                        code = 2;
                    }
                    nxt[s + 2] = (best == NEG_INF_D) ? NEG_INF_D : best + (double)ev;
                    bp[(size_t)t * sp + s] = (uint8_t)code;
                }
                if (more && f == fend - 1) stage_store(em[(c + 1) & 1]);    // (its last readers passed chunk c - 1's final barrier)
                __syncthreads();
                cur ^= 1;
                ++t;
            }
        }
        // every thread reads the same two cells: S-1 first, S-2 only if strictly better
        const double* last = rowbuf[cur];
        final_v = last[S + 1];
        final_s = S - 1;
        if (S > 1 && last[S] > final_v) {
            final_v = last[S];
            final_s = S - 2;
        }
    } else if (!bad && tl == 0 && L == 0) {
        final_v = 0.0;                                      // the empty path of an empty transcript
    }
    if (tid == 0) score[b] = (float)final_v;
    const bool feasible = final_v != NEG_INF_D && final_v == final_v;
    if (!feasible || tl == 0) {
        for (int t = tid; t < tl; t += NTHR) st_out[t] = -1;
        for (int l = tid; l < L; l += NTHR) start_out[l] = end_out[l] = -1;
        return;
    }

    // ---- back-trace: the pointer bytes were written by this workgroup's own waves
    __threadfence();
    __syncthreads();
    int s_hi = final_s, after = -2;                         // state at frame t_hi - 1; state at frame t_hi (-2: none)
    for (int t_hi = tl; t_hi > 0; t_hi -= BT_F) {
        const int t_lo = max(0, t_hi - BT_F), n = t_hi - t_lo;
        const int s_lo = max(0, s_hi - (BT_W - 1));
        for (int idx = tid; idx < n * BT_W; idx += NTHR) {
            const int f = idx / BT_W, col = s_lo + (idx % BT_W);
            win[f][idx % BT_W] = (col <= s_hi) ? bp[(size_t)(t_lo + f) * sp + col] : (uint8_t)0;
        }
        __syncthreads();
        if (tid == 0) {
            int w = s_hi;
            path[n + 1] = after;
            for (int f = n - 1; f >= 0; --f) {
                path[1 + f] = w;
                const int code = win[f][max(w - s_lo, 0)];  // (w >= s_hi - 2 (n - 1 - f) >= s_lo on a path; the clamp is for the index only)
                w = max(w - min(code, 2), 0);               // the step below row 0 may leave the window: it is the next one's top
            }
            path[0] = t_lo > 0 ? w : -2;
        }
        __syncthreads();
        for (int f = tid; f < n; f += NTHR) {
            const int w = path[1 + f], t = t_lo + f;
            st_out[t] = w;
            if (w & 1) {
                if (path[f] != w) start_out[w >> 1] = t;
                if (path[2 + f] != w) end_out[w >> 1] = t;
            }
        }
        after = path[1];
        s_hi = path[0];
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t ds2_ctc_align_ws_bytes(int B, int T, int max_label_len) {
    if (B < 0 || T < 0 || max_label_len < 0) return 0;
    return (size_t)B * T * bp_stride(max_label_len) + 16;
}

extern "C" int ds2_ctc_align(const float* probs, const int32_t* sizes, const int32_t* labels, const int32_t* label_offsets,
                             const int32_t* label_lens, int B, int T, int A, int max_label_len, int blank, int log_input,
                             void* ws, size_t ws_bytes, int32_t* states, int32_t* starts, int32_t* ends, float* score,
                             void* stream) {
    if (max_label_len < 0 || 2 * (long)max_label_len + 1 >= MAX_S) {
        ds2_set_error("ds2_ctc_align: max_label_len %d is outside 0..%d (one state per thread, 2 L + 1 <= %d)",
                      max_label_len, (MAX_S - 2) / 2, MAX_S - 1);
        return DS2_ERR_ARG;
    }
    if (A < 1 || A > MAX_A) {
        ds2_set_error("ds2_ctc_align: alphabet size %d is outside 1..%d", A, MAX_A);
        return DS2_ERR_ARG;
    }
    DS2_CHECK_ARG(B >= 0 && T >= 0 && blank >= 0 && blank < A);
    if (B == 0) return DS2_OK;
    // (labels may be NULL when every transcript is empty: it is read only below a positive label_lens[b])
    DS2_CHECK_ARG(sizes && label_offsets && label_lens && score && (probs || T == 0));
    DS2_CHECK_ARG((states || T == 0) && ((starts && ends) || max_label_len == 0));
    if (ws_bytes < ds2_ctc_align_ws_bytes(B, T, max_label_len) || !ws) {
        ds2_set_error("ds2_ctc_align: workspace of %zu bytes < ds2_ctc_align_ws_bytes = %zu", ws_bytes,
                      ds2_ctc_align_ws_bytes(B, T, max_label_len));
        return DS2_ERR_ARG;
    }
    const int smax = 2 * max_label_len + 1;
#define DS2_CTC_ALIGN(N_)                                                                                              \
    hipLaunchKernelGGL(ctc_align_kernel<N_>, dim3(B), dim3(N_), 0, (hipStream_t)stream, probs, sizes, labels,           \
                       label_offsets, label_lens, T, A, max_label_len, blank, log_input, (uint8_t*)ws,                   \
                       bp_stride(max_label_len), states, starts, ends, score)
    if (smax <= 256) DS2_CTC_ALIGN(256);
    else if (smax <= 512) DS2_CTC_ALIGN(512);
    else DS2_CTC_ALIGN(1024);
#undef DS2_CTC_ALIGN
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
