// What the CTC best-path kernels over a (B,T,A) input share: ctc_align.hip, ctc_align_banded.hip (both forms) and
// ctc_keyword.hip.  (ctc.hip and ctc_mwer.hip sum over the paths of a (T,B,A) input; their parts are in ctc_common.h.)
//
//   staging     a row's emissions go through LDS a chunk of CH = min(32, 1024 / A) frames at a time, loaded a chunk ahead as
//               in ctc.hip: probs is (B,T,A) here, so a chunk is one contiguous run of floats.  ChunkStager::load puts chunk
//               c + 1 into registers while chunk c's frames are worked on; ::store applies the caller's per-element term and
//               writes the other LDS buffer, NaN -> -inf, and pins the wait for the loads to the place it is called from.
//   tie rule    stay, then s-1, then s-2 (strict > in that order), at the end S-1 before S-2 -- part of the contract, so a
//               result is bit-reproducible and independent of the rest of the batch (best_of3; the banded kernels keep it
//               written out, see profiles/align_refactor.md).
//   alignment   align_prologue clamps an utterance's sizes, validates its labels and fills what no path will write;
//               align_has_path ends an utterance that has no alignment.
//   pointers    one byte per (t, s) (0 stay / 1 / 2; the gap form's flag is bit 2) to the caller's workspace, lane-contiguous
//               byte stores nothing waits for.
//   back-trace  after a device-scope fence and a barrier: BT_F frames at a time, from the last frame down.  The path
//               descends by at most 2 states per frame, so the BT_F x BT_W window of pointer bytes below the state the path
//               has at the chunk's last frame holds every byte the walk can touch: all threads load it into LDS with
//               independent loads, thread 0 walks it there, all threads write states / starts / ends.  T / BT_F global
//               round trips instead of T dependent ones (align_backtrace).
//   host        the refusals the entry points have in common, under the entry point's own name.
#pragma once
#include "ds2_common.h"

namespace ctc_path {

constexpr int EM_FLOATS = 1024;          // per staging buffer: CH = min(32, 1024 / A) frames
constexpr int EM_NLD = 4;                // staging loads per thread and chunk (threads 0..255 do the staging)
constexpr int MAX_CH = 32;
constexpr int MAX_A = 256;               // CH >= 4
constexpr int BT_F = 64;                 // back-trace: frames per window
constexpr int BT_W = 2 * BT_F;           // ... and states per window row (the walk needs 2 (BT_F - 1) + 1)
constexpr double NEG_INF = -(double)INFINITY;

// Thread tid < 256 carries elements idx = tid + 256 i of a chunk (CH frames of A floats, contiguous) of the row `pb`.
struct ChunkStager {
    const float* pb;
    int tid, tl, A, CH, nper, nchunk;
    float ra[EM_NLD];

    __device__ __forceinline__ ChunkStager(const float* row, int tid_, int tl_, int A_)
        : pb(row), tid(tid_), tl(tl_), A(A_), CH(min(MAX_CH, EM_FLOATS / A_)), nper(CH * A_), nchunk((tl_ + CH - 1) / CH) {}

    // also(i) runs where element i of chunk c is this thread's to load: inside the chunk and inside the row's valid frames
    template <class Also>
    __device__ __forceinline__ void load(int c, Also also) {
        const int left = (tl - c * CH) * A;                 // floats of valid frames from this chunk's start on
#pragma unroll
        for (int i = 0; i < EM_NLD; ++i) {
            const int idx = tid + 256 * i;
            ra[i] = 0.f;
            if (tid < 256 && idx < nper && idx < left) {
                ra[i] = pb[(size_t)c * nper + idx];
                also(i);
            }
        }
    }
    __device__ __forceinline__ void load(int c) {
        load(c, [](int) {});
    }
    // dst[idx] = op(the loaded float, i), NaN -> -inf
    template <class Op>
    __device__ __forceinline__ void store(float* dst, Op op) const {
#pragma unroll
        for (int i = 0; i < EM_NLD; ++i) {
            const int idx = tid + 256 * i;
            if (tid < 256 && idx < nper) {
                float a = ra[i];
                asm volatile("" : "+v"(a));                 // keeps the wait for the loads HERE, where the caller put the store
                a = op(a, i);
                dst[idx] = (a == a) ? a : -INFINITY;
            }
        }
    }
};

// the tie rule: stay (0), then s-1 (1), then s-2 (2), each only if strictly better
__device__ __forceinline__ double best_of3(double x0, double x1, double x2, int& code) {
    double best = x0;
    code = 0;
    if (x1 > best) {
        best = x1;
        code = 1;
    }
    if (x2 > best) {
        best = x2;
        code = 2;
    }
    return best;
}

// one utterance of an alignment launch: its clamped sizes, its labels and its rows of the outputs
struct AlignUtt {
    int L, tl, S;                        // labels, frames, states 2 L + 1
    const int32_t* lab;
    int32_t *st_out, *start_out, *end_out;
    uint8_t* gap_out;                    // GAP only
};

// Clamps L and tl, raises `bad` (one int of LDS) for a length or a label out of range -- reported as infeasible, never used as
// an index -- and writes -1 past tl and past L.  `bad` may be read after the caller's next barrier (once: it is an LDS read).
template <int NTHR, bool GAP>
__device__ __forceinline__ AlignUtt align_prologue(const int32_t* __restrict__ sizes, const int32_t* __restrict__ labels,
                                                   const int32_t* __restrict__ label_offsets,
                                                   const int32_t* __restrict__ label_lens, int T, int A, int lmax, int blank,
                                                   int32_t* __restrict__ states, int32_t* __restrict__ starts,
                                                   int32_t* __restrict__ ends, uint8_t* __restrict__ gap_all, int& bad) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lraw = label_lens[b];
    const bool len_ok = Lraw >= 0 && Lraw <= lmax;
    AlignUtt u;
    u.L = len_ok ? Lraw : 0;
    u.tl = min(max(sizes[b], 0), T);
    u.S = 2 * u.L + 1;
    if (tid == 0) bad = len_ok ? 0 : 1;
    __syncthreads();
    u.lab = labels + label_offsets[b];
    for (int l = tid; l < u.L; l += NTHR) {
        const int sym = u.lab[l];
        if (sym < 0 || sym >= A || sym == blank) bad = 1;
    }
    u.st_out = states + (size_t)b * T;
    u.start_out = starts + (size_t)b * lmax;
    u.end_out = ends + (size_t)b * lmax;
    u.gap_out = GAP ? gap_all + (size_t)b * T : nullptr;
    for (int t = u.tl + tid; t < T; t += NTHR) {
        u.st_out[t] = -1;
        if constexpr (GAP) u.gap_out[t] = 0;
    }
    for (int l = u.L + tid; l < lmax; l += NTHR) u.start_out[l] = u.end_out[l] = -1;
    return u;
}

// final_v is what the recursion left (-inf where it did not run); the empty path of an empty transcript scores 0.  Returns
// false, with -1 in the utterance's frames and labels, where there is no path to trace.
template <int NTHR, bool GAP>
__device__ __forceinline__ bool align_has_path(const AlignUtt& u, bool ok, double& final_v) {
    const int tid = threadIdx.x;
    if (ok && u.tl == 0 && u.L == 0) final_v = 0.0;
    const bool feasible = final_v != NEG_INF && final_v == final_v;
    if (feasible && u.tl != 0) return true;
    for (int t = tid; t < u.tl; t += NTHR) {
        u.st_out[t] = -1;
        if constexpr (GAP) u.gap_out[t] = 0;
    }
    for (int l = tid; l < u.L; l += NTHR) u.start_out[l] = u.end_out[l] = -1;
    return false;
}

// The walk from state final_s at frame tl - 1.  The byte of (t, s) is bp[t * stride + (s & mask)]: the pointer bytes were
// written by this workgroup's own waves.
template <int NTHR, bool GAP>
__device__ __forceinline__ void align_backtrace(const AlignUtt& u, const uint8_t* bp, size_t stride, int mask, int final_s) {
    __shared__ uint8_t win[BT_F][BT_W];
    __shared__ int path[BT_F + 2];       // path[1 + f] = state at frame t_lo + f; [0] / [n + 1] = the frames around the window
    __shared__ uint8_t pgap[GAP ? BT_F : 1];                // GAP: the gap flag of the path's frames in a window
    const int tid = threadIdx.x;
    __threadfence();
    __syncthreads();
    int s_hi = final_s, after = -2;                         // state at frame t_hi - 1; state at frame t_hi (-2: none)
    for (int t_hi = u.tl; t_hi > 0; t_hi -= BT_F) {
        const int t_lo = max(0, t_hi - BT_F), n = t_hi - t_lo;
        const int s_lo = max(0, s_hi - (BT_W - 1));
        for (int idx = tid; idx < n * BT_W; idx += NTHR) {
            const int f = idx / BT_W, col = s_lo + (idx % BT_W);
            win[f][idx % BT_W] = (col <= s_hi) ? bp[(size_t)(t_lo + f) * stride + (col & mask)] : (uint8_t)0;
        }
        __syncthreads();
        if (tid == 0) {
            int w = s_hi;
            path[n + 1] = after;
            for (int f = n - 1; f >= 0; --f) {
                path[1 + f] = w;
                int code = win[f][max(w - s_lo, 0)];        // (w >= s_hi - 2 (n - 1 - f) >= s_lo on a path; the clamp is for the index only)
                if constexpr (GAP) {
                    pgap[f] = (uint8_t)((code >> 2) & 1);
                    code &= 3;
                }
                w = max(w - min(code, 2), 0);               // the step below row 0 may leave the window: it is the next one's top
            }
            path[0] = t_lo > 0 ? w : -2;
        }
        __syncthreads();
        for (int f = tid; f < n; f += NTHR) {
            const int w = path[1 + f], t = t_lo + f;
            u.st_out[t] = w;
            if constexpr (GAP) u.gap_out[t] = pgap[f];
            if (w & 1) {
                if (path[f] != w) u.start_out[w >> 1] = t;
                if (path[2 + f] != w) u.end_out[w >> 1] = t;
            }
        }
        after = path[1];
        s_hi = path[0];
        __syncthreads();
    }
}

// ---- host side: refusals under the entry point's name `fn`

#define CTC_PATH_CHECK_ARG(fn, cond)                                /* DS2_CHECK_ARG under the entry point's name */ \
    do {                                                                                                            \
        if (!(cond)) {                                                                                              \
            ds2_set_error("%s: bad argument: %s", fn, #cond);                                                       \
            return DS2_ERR_ARG;                                                                                     \
        }                                                                                                           \
    } while (0)

inline int check_alphabet(const char* fn, int A) {
    if (A >= 1 && A <= MAX_A) return DS2_OK;
    ds2_set_error("%s: alphabet size %d is outside 1..%d", fn, A, MAX_A);
    return DS2_ERR_ARG;
}

inline int check_workspace(const char* fn, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes >= need && ws) return DS2_OK;
    ds2_set_error("%s: workspace of %zu bytes < %s_ws_bytes = %zu", fn, ws_bytes, fn, need);
    return DS2_ERR_ARG;
}

// What the three alignment entry points check after their own size limits, in the order the refusals fire.  `banded` entries
// take lo, the GAP entry space, gap_penalty and gap besides (the two forms of each pointer test differ in their text only by
// those).  B = 0 is DS2_OK before any pointer is looked at: the caller returns then.
inline int check_align_args(const char* fn, bool banded, bool GAP, const float* probs, const int32_t* sizes,
                            const int32_t* label_offsets, const int32_t* label_lens, const int32_t* lo, int B, int T, int A,
                            int max_label_len, int blank, int space, float gap_penalty, const void* ws, size_t ws_bytes,
                            size_t ws_need, const int32_t* states, const int32_t* starts, const int32_t* ends,
                            const uint8_t* gap, const void* score) {
    if (check_alphabet(fn, A) != DS2_OK) return DS2_ERR_ARG;
    CTC_PATH_CHECK_ARG(fn, B >= 0 && T >= 0 && blank >= 0 && blank < A);
    if (GAP && !(gap_penalty >= 0.f)) {                     // (a NaN fails the comparison)
        ds2_set_error("%s: gap_penalty %g is negative or NaN", fn, (double)gap_penalty);
        return DS2_ERR_ARG;
    }
    if (GAP && (space < -1 || space >= A || space == blank)) {
        ds2_set_error("%s: space %d is neither -1 nor a symbol of 0..%d other than blank %d", fn, space, A - 1, blank);
        return DS2_ERR_ARG;
    }
    if (B == 0) return DS2_OK;
    // (labels may be NULL when every transcript is empty: it is read only below a positive label_lens[b])
    if (banded) {
        CTC_PATH_CHECK_ARG(fn, sizes && label_offsets && label_lens && score && (probs || T == 0) && (lo || T == 0));
        CTC_PATH_CHECK_ARG(fn, (states || T == 0) && ((starts && ends) || max_label_len == 0) && (!GAP || gap || T == 0));
    } else {
        CTC_PATH_CHECK_ARG(fn, sizes && label_offsets && label_lens && score && (probs || T == 0));
        CTC_PATH_CHECK_ARG(fn, (states || T == 0) && ((starts && ends) || max_label_len == 0));
    }
    return check_workspace(fn, ws, ws_bytes, ws_need);
}

}  // namespace ctc_path
