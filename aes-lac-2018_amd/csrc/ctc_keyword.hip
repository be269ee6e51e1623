// CTC keyword search: where, in every utterance of a batch, was each of K phrases said, and how far from the model's own best
// path is that reading (include/ds2hip.h, "keyword search", has the definition).  gfx950.
//
// Two launches on the stream:
//   row maxima  m[b][t] = max_a logp[b][t][a] (NaN as -inf) for t < sizes[b], into the caller's workspace: one sub-wave group
//               of G = min(64, pow2 >= A) lanes per frame, xor-butterfly.  Done ONCE per call: an utterance's frames are
//               shared by the K / 4 workgroups that search it, and the maximum is the same for all of them.
//   search      one WAVE per (utterance, keyword); lane j carries label state 2 j and the blank state 2 j + 1 behind it, so
//               64 lanes hold the S = 2 L - 1 <= 127 states and a frame needs ONE exchange: lane j - 1 hands lane j the
//               better of its blank (s-1 of lane j's label) and, where the labels differ, its label (s-2), s-1 winning a
//               tie -- which with "stay first" is the contract's order stay, s-1, s-2.  The blank's predecessors are its own
//               lane's.  Lane 0 takes the fresh start (0, t) instead.  No barrier and no LDS row per frame.
//               The 4 waves of a workgroup take 4 keywords of the SAME utterance and share its normalised emissions
//               e = logp - m, staged through LDS a chunk of frames at a time and loaded a chunk ahead (ctc_path_common.h):
//               one barrier per chunk.  Lane L - 1 owns D[t] and st[t] and runs the clustering pass on them in registers.
// Critical path: T dependent steps of one wave (shuffle, compare, fp64 add); all pairs run side by side.
// No workgroup waits on another; no atomics; outputs leave through ordinary vector stores.
#include "ctc_path_common.h"

#include <limits.h>

namespace {

using namespace ctc_path;

constexpr int KW_MAX_LEN = 64;           // DS2_KWS_MAX_LEN: one label per lane
constexpr int KW_MAX_HITS = 64;
constexpr int KW_WAVES = 4;              // keywords per workgroup
constexpr int KW_NTHR = 64 * KW_WAVES;
static_assert(KW_NTHR == 256, "every thread stages");

inline size_t rowmax_bytes(int B, int T) { return (((size_t)B * T * sizeof(float)) + 15) & ~(size_t)15; }

// group g of G lanes takes frame g of the flattened (b, t); frames at or past sizes[b] are neither read nor written
__global__ __launch_bounds__(256) void kws_rowmax_kernel(const float* __restrict__ logp, const int32_t* __restrict__ sizes,
                                                         long rows, int T, int A, int G, float* __restrict__ rowmax) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = gid / G;
    const int col = (int)(gid % G);
    bool live = row < rows;
    if (live) {
        const int b = (int)(row / T), t = (int)(row % T);
        live = t < min(max(sizes[b], 0), T);
    }
    float m = -INFINITY;
    if (live) {
        const float* p = logp + (size_t)row * A;
        for (int a = col; a < A; a += G) {
            const float x = p[a];
            if (x > m) m = x;                               // (a NaN compares false: it counts as -inf)
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                      // all 64 lanes take part; a group only mixes with itself
        const float y = __shfl_xor(m, o, 64);
        if (o < G && y > m) m = y;
    }
    if (live && col == 0) rowmax[row] = m;
}

__global__ __launch_bounds__(KW_NTHR) void ctc_keyword_kernel(
    const float* __restrict__ logp, const float* __restrict__ rowmax, const int32_t* __restrict__ sizes,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ label_lens,
    const double* __restrict__ min_score, int T, int A, int K, int KG, int blank, int max_hits, int32_t* __restrict__ hits,
    double* __restrict__ hit_score, int32_t* __restrict__ n_hits) {
    __shared__ float em[2][EM_FLOATS];
    __shared__ int hit_buf[KW_WAVES][KW_MAX_HITS][2];       // the hits as they are emitted: no global store inside the frame loop
    __shared__ double score_buf[KW_WAVES][KW_MAX_HITS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / KG;
    const int k = (blockIdx.x % KG) * KW_WAVES + wave;
    const int tl = min(max(sizes[b], 0), T);

    // ---- this wave's keyword: lane j < L holds label j; a keyword that cannot be searched has no hits
    bool ok = k < K;
    int L = 0;
    if (ok) {
        L = label_lens[k];
        ok = L >= 1 && L <= KW_MAX_LEN;
    }
    int sym = 0;                                            // (dead lanes read column 0: their states feed nobody below them)
    bool bad = false;
    if (ok && lane < L) {
        const int s = labels[label_offsets[k] + lane];
        bad = s < 0 || s >= A || s == blank;                // reported, never used as an index
        if (!bad) sym = s;
    }
    ok = ok && !__any(bad);
    const int last = ok ? L - 1 : 0;                        // the lane of state S - 1
    const int sym_next = __shfl_down(sym, 1, 64);
    const bool skip_next = lane + 1 < L && sym_next != sym; // lane + 1's label may be entered from this lane's label
    double thr = ok ? min_score[k] : NEG_INF;
    asm volatile("" : "+v"(thr));                           // waited for HERE: inside the frame loop it would wait for the staging loads too

    const size_t pair = (size_t)b * K + (k < K ? k : 0);
    int32_t* hit_out = hits + pair * max_hits * 2;
    double* score_out = hit_score + pair * max_hits;

    // ---- staging: with each float its frame's row maximum
    ChunkStager stage(logp + (size_t)b * T * A, tid, tl, A);
    const int CH = stage.CH, nchunk = stage.nchunk;
    const float* mb = rowmax + (size_t)b * T;
    float rm[EM_NLD];
    int fr[EM_NLD];
#pragma unroll
    for (int i = 0; i < EM_NLD; ++i) fr[i] = (tid + KW_NTHR * i) / A;
    auto stage_load = [&](int c) {
#pragma unroll
        for (int i = 0; i < EM_NLD; ++i) rm[i] = 0.f;
        stage.load(c, [&](int i) { rm[i] = mb[c * CH + fr[i]]; });
    };
    // the one fp32 subtraction; -inf - -inf and inf - inf are NaN
    const auto term = [&](float a, int i) { return ((a == a) ? a : -INFINITY) - rm[i]; };

    double v_lab = NEG_INF, v_blk = NEG_INF;
    int st_lab = -1, st_blk = -1;
    bool have = false;                                      // the current hit of the clustering pass (lane `last` only)
    double h_score = NEG_INF;
    int h_start = -1, h_end = -1, count = 0;
    auto emit = [&]() {
        if (count < max_hits) {
            hit_buf[wave][count][0] = h_start;
            hit_buf[wave][count][1] = h_end;
            score_buf[wave][count] = h_score;
        }
        ++count;
    };

    stage_load(0);
    stage.store(em[0], term);
    __syncthreads();
    int t = 0;
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        if (more) stage_load(c + 1);                        // in flight while this chunk's frames are worked on
        if (ok) {
            const float* e = em[c & 1];
            const int fend = min(CH, tl - c * CH);
            for (int f = 0; f < fend; ++f, ++t) {
                const double el = (double)e[f * A + sym], eb = (double)e[f * A + blank];
                // what lane + 1's label sees below it: s-1 (this blank), then s-2 (this label) if strictly better
                double cv = v_blk;
                int cs = st_blk;
                if (skip_next && v_lab > cv) {
                    cv = v_lab;
                    cs = st_lab;
                }
                double pv = __shfl_up(cv, 1, 64);
                int ps = __shfl_up(cs, 1, 64);
                if (lane == 0) {                            // state 0: a fresh start at this frame
                    pv = 0.0;
                    ps = t;
                }
                double bv = v_blk;                          // blank 2 j + 1: stay, then label 2 j
                int bs = st_blk;
                if (v_lab > bv) {
                    bv = v_lab;
                    bs = st_lab;
                }
                double lv = v_lab;                          // label 2 j: stay, then what came up from lane j - 1
                int ls = st_lab;
                if (pv > lv) {
                    lv = pv;
                    ls = ps;
                }
                v_blk = bv + eb;
                st_blk = bs;
                v_lab = lv + el;
                st_lab = ls;
                if (lane == last && v_lab >= thr) {         // the candidate (D[t], st[t], t); a NaN threshold admits none
                    bool take = !have;
                    if (have && st_lab > h_end) {
                        emit();
                        take = true;
                    } else if (have && (v_lab > h_score || (v_lab == h_score && st_lab == h_start))) {
                        take = true;
                    }
                    if (take) {
                        have = true;
                        h_score = v_lab;
                        h_start = st_lab;
                        h_end = t;
                    }
                }
            }
        }
        if (more) stage.store(em[(c + 1) & 1], term);       // after the chunk's frames (its last readers passed chunk c - 1's final barrier)
        __syncthreads();
    }
    if (lane == last && have) emit();
    __syncthreads();                                        // lane `last`'s rows, for the whole wave to write out
    if (k >= K) return;
    const int total = __shfl(count, last, 64);
    if (lane == 0) n_hits[pair] = total;
    for (int r = lane; r < max_hits; r += 64) {             // the hits, then -1 / -inf in the rows past the count
        const bool hit = r < total;
        hit_out[2 * r] = hit ? hit_buf[wave][r][0] : -1;
        hit_out[2 * r + 1] = hit ? hit_buf[wave][r][1] : -1;
        score_out[r] = hit ? score_buf[wave][r] : NEG_INF;
    }
}

}  // namespace

extern "C" size_t ds2_ctc_keyword_search_ws_bytes(int B, int T) {
    if (B < 0 || T < 0) return 0;
    return rowmax_bytes(B, T) + 16;
}

extern "C" int ds2_ctc_keyword_search(const float* logp, const int32_t* sizes, const int32_t* labels,
                                      const int32_t* label_offsets, const int32_t* label_lens, const double* min_score,
                                      int B, int T, int A, int K, int blank, int max_hits, void* ws, size_t ws_bytes,
                                      int32_t* hits, double* hit_score, int32_t* n_hits, void* stream) {
    if (check_alphabet(__func__, A) != DS2_OK) return DS2_ERR_ARG;
    if (K < 1 || K > 65535) {
        ds2_set_error("ds2_ctc_keyword_search: %d keywords is outside 1..65535", K);
        return DS2_ERR_ARG;
    }
    if (max_hits < 1 || max_hits > KW_MAX_HITS) {
        ds2_set_error("ds2_ctc_keyword_search: max_hits %d is outside 1..%d", max_hits, KW_MAX_HITS);
        return DS2_ERR_ARG;
    }
    DS2_CHECK_ARG(B >= 0 && T >= 0 && blank >= 0 && blank < A);
    const int KG = (K + KW_WAVES - 1) / KW_WAVES;
    DS2_CHECK_ARG((long)B * T <= INT_MAX / 64 && (long)B * KG <= INT_MAX);
    if (B == 0) return DS2_OK;
    DS2_CHECK_ARG(sizes && labels && label_offsets && label_lens && min_score && hits && hit_score && n_hits);
    DS2_CHECK_ARG(logp || T == 0);
    if (check_workspace(__func__, ws, ws_bytes, ds2_ctc_keyword_search_ws_bytes(B, T)) != DS2_OK) return DS2_ERR_ARG;
    float* rowmax = (float*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    if (T > 0) {
        int G = 1;
        while (G < A && G < 64) G *= 2;
        const long rows = (long)B * T;
        hipLaunchKernelGGL(kws_rowmax_kernel, dim3(ds2_cdiv(rows * G, 256)), dim3(256), 0, (hipStream_t)stream, logp, sizes,
                           rows, T, A, G, rowmax);
        DS2_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ctc_keyword_kernel, dim3(B * KG), dim3(KW_NTHR), 0, (hipStream_t)stream, logp, rowmax, sizes, labels,
                       label_offsets, label_lens, min_score, T, A, K, KG, blank, max_hits, hits, hit_score, n_hits);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
