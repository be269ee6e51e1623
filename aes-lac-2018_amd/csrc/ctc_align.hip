// CTC forced alignment (max-sum / Viterbi over the transcript's extended sequence) with back-trace, gfx950.
//
// One workgroup per utterance, one state per thread (256 / 512 / 1024 threads for up to that many of the 2 L + 1 states
// blank, l1, blank, ..., lL, blank of the minibatch's longest transcript), ONE launch:
//   recursion   v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if ext[s] is a label != ext[s-2]) + e[t][ext[s]], carried
//               in fp64; e is the input itself (log_input) or its fp32 log, NaN -> -inf.  The row lives in LDS,
//               double-buffered, one barrier per frame.  Frame 0 runs through the same loop from a virtual row
//               {0, -inf, ...}, which admits exactly states 0 and 1.
// Emission staging, the tie rule, the pointer bytes and the back-trace are ctc_path_common.h's.
// Critical path: T barriers per utterance, then T dependent LDS reads of one thread.
#include "ctc_path_common.h"

namespace {

using namespace ctc_path;

constexpr int MAX_S = 1024;              // 2 L + 1 <= 1023

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
    __shared__ int bad;

    const int tid = threadIdx.x;
    const AlignUtt u = align_prologue<NTHR, false>(sizes, labels, label_offsets, label_lens, T, A, lmax, blank, states, starts,
                                                   ends, nullptr, bad);
    const int tl = u.tl, S = u.S;
    // INVARIANT: ext[] may hold out-of-range symbols when `bad` is set; it is read only under `ok` below
    for (int s = tid; s < S; s += NTHR) ext[s] = (s & 1) ? u.lab[s >> 1] : blank;
    for (int i = tid; i < MAX_S + 4; i += NTHR) {
        rowbuf[0][i] = (i == 2) ? 0.0 : NEG_INF;            // cell s + 2 holds state s; cells 0, 1 stay -inf guards
        rowbuf[1][i] = NEG_INF;
    }
    __syncthreads();

    uint8_t* bp = bp_all + (size_t)blockIdx.x * T * sp;
    const int s = tid;
    const bool live = s < S;
    double final_v = NEG_INF;
    int final_s = -1;
    const bool ok = !bad;
    if (ok && tl > 0) {
        const int sym = live ? ext[s] : 0;
        const bool skip = live && s >= 2 && (s & 1) && ext[s] != ext[s - 2];
        ChunkStager stage(probs + (size_t)blockIdx.x * T * A, tid, tl, A);
        const int CH = stage.CH, nchunk = stage.nchunk;
        const auto term = [&](float a, int) { return log_input ? a : logf(a); };   // log 0 = -inf, log of a negative = NaN
        stage.load(0);
        stage.store(em[0], term);
        __syncthreads();
        int cur = 0, t = 0;
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) stage.load(c + 1);                    // in flight while this chunk's frames are worked on
            const float* e = em[c & 1] + sym;
            const int fend = min(CH, tl - c * CH);
            for (int f = 0; f < fend; ++f) {
                const double* prev = rowbuf[cur];
                double* nxt = rowbuf[cur ^ 1];
                if (live) {
                    const double x0 = prev[s + 2], x1 = prev[s + 1], x2r = prev[s];
                    const float ev = e[f * A];
                    const double x2 = skip ? x2r : NEG_INF;
                    int code;
                    const double best = best_of3(x0, x1, x2, code);
                    nxt[s + 2] = (best == NEG_INF) ? NEG_INF : best + (double)ev;
                    bp[(size_t)t * sp + s] = (uint8_t)code;
                }
                if (more && f == fend - 1) stage.store(em[(c + 1) & 1], term);    // (its last readers passed chunk c - 1's final barrier)
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
    }
    const bool has_path = align_has_path<NTHR, false>(u, ok, final_v);
    if (tid == 0) score[blockIdx.x] = (float)final_v;
    if (has_path) align_backtrace<NTHR, false>(u, bp, sp, -1, final_s);
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
    const int rc = check_align_args(__func__, false, false, probs, sizes, label_offsets, label_lens, nullptr, B, T, A,
                                    max_label_len, blank, -1, 0.f, ws, ws_bytes, ds2_ctc_align_ws_bytes(B, T, max_label_len),
                                    states, starts, ends, nullptr, score);
    if (rc != DS2_OK || B == 0) return rc;
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
