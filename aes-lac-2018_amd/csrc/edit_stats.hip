// Word and character error counts of R hypothesis rows against their references, from label ids (ds2_edit_stats).
// Not in the reference (its test.py turns labels into strings and calls python-Levenshtein per utterance);
// include/ds2hip.h has the definition, tests/edit_ref.py states it in Python.  DESIGN.md "LM weight tuning".
//
// One workgroup (256 threads) per (row, level), level 0 = characters, 1 = words; no inter-workgroup communication.
//   1. items: each thread owns ES_CHUNK = 8 consecutive labels of a side; one block scan per side gives every kept label
//      (characters: every non-space label) or word start (words: a non-space label at position 0 or after a space) its index.
//      Characters are copied into LDS; a word becomes (start | length << 16, 32-bit hash of its labels).
//   2. the Levenshtein table is swept by anti-diagonals d = i + j (i hypothesis items, j reference items).  A cell is one
//      64-bit word, dist << 48 | S << 32 | D << 16 | I, so taking a predecessor and adding the cell's own operation is one
//      add.  ONE array x[] of m + n + 1 words, indexed by j - i + m, holds the sweep: cell (i, j) overwrites (i-1, j-1) in
//      its own slot, and its two other predecessors (i, j-1) and (i-1, j) are the neighbouring slots, which hold diagonal
//      d - 1 and are not written during step d (slots of one parity are written in one step).  One barrier per diagonal.
//   3. two words are equal if hash and length agree AND their labels do (read from global memory; the hash only filters).
// The tie rule (equal items: the diagonal; otherwise the cheapest of substitution, deletion, insertion in that order) is
// per cell, so the counts carried forward are those of a back-trace under the same rule; no back-pointer is stored.
// Totals are 64-bit integer atomic adds: the sums do not depend on the order of arrival.
#include "ds2_common.h"

namespace {

constexpr int ES_THREADS = DS2_EDIT_THREADS;
constexpr int ES_MAX = DS2_EDIT_MAX_ITEMS;
constexpr int ES_CHUNK = ES_MAX / ES_THREADS;          // labels of one side per thread in the item pass
static_assert(ES_CHUNK * ES_THREADS == ES_MAX, "a thread owns a whole chunk");
static_assert(ES_MAX <= 4096, "cell fields are 16 bits wide and a start fits under the length");

constexpr uint64_t OP_SUB = (1ull << 48) | (1ull << 32);
constexpr uint64_t OP_DEL = (1ull << 48) | (1ull << 16);
constexpr uint64_t OP_INS = (1ull << 48) | 1ull;

struct EsLds {
    uint64_t x[2 * ES_MAX + 1];        // the sweep, slot j - i + m
    int32_t a[2][ES_MAX];              // [side] characters: the label; words: start | length << 16
    uint32_t h[2][ES_MAX / 2 + 1];     // words: the hash (a side of ES_MAX labels has at most ES_MAX / 2 words)
    int wave_tot[ES_THREADS / 64];
};

// block-wide exclusive scan of one int per thread (all threads call it)
__device__ inline int es_exscan(int v, int* total, EsLds& s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s.wave_tot[wave] = x;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < ES_THREADS / 64; ++w) {
        const int t = s.wave_tot[w];
        if (w < wave) base += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return base + x - v;
}

// the items of one side (seq[0..len)) into s.a[side] / s.h[side]; returns their number (all threads call it)
__device__ int es_items(const int32_t* __restrict__ seq, int len, int level, int space, int side, EsLds& s) {
    const int p0 = min((int)threadIdx.x * ES_CHUNK, len), p1 = min(p0 + ES_CHUNK, len);
    int cnt = 0;
    for (int p = p0; p < p1; ++p) {
        const bool keep = seq[p] != space;
        cnt += level == 0 ? keep : (keep && (p == 0 || seq[p - 1] == space));
    }
    int total;
    int at = es_exscan(cnt, &total, s);
    for (int p = p0; p < p1; ++p) {
        const int c = seq[p];
        if (c == space) continue;
        if (level == 0) {
            s.a[side][at++] = c;
        } else if (p == 0 || seq[p - 1] == space) {
            uint32_t h = 2166136261u;
            int e = p;
            for (; e < len && seq[e] != space; ++e) h = (h ^ (uint32_t)seq[e]) * 16777619u;
            s.a[side][at] = p | ((e - p) << 16);
            s.h[side][at++] = h;
        }
    }
    return total;
}

__global__ void __launch_bounds__(ES_THREADS)
edit_stats_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int hyp_stride,
                  const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_offsets,
                  const int32_t* __restrict__ ref_lens, int N, int max_ref_len, const int32_t* __restrict__ ref_index,
                  const int32_t* __restrict__ group, int G, int space, int32_t* __restrict__ stats,
                  long long* __restrict__ totals) {
    __shared__ EsLds s;
    const int r = blockIdx.x >> 1, level = blockIdx.x & 1, tid = threadIdx.x;
    int32_t* out = stats + (size_t)r * 10 + 5 * level;
    // validity, the same decision in both of the row's workgroups
    const int hl = hyp_len[r];
    const int ri = ref_index ? ref_index[r] : r;
    const int g = group ? group[r] : 0;
    bool ok = hl >= 0 && hl <= hyp_stride && ri >= 0 && ri < N && g >= 0 && (!group || g < G);
    int rl = 0;
    if (ok) {
        rl = ref_lens[ri];
        ok = rl >= 0 && rl <= max_ref_len;
    }
    if (!ok) {
        if (tid < 5) out[tid] = -1;
        return;
    }
    const int32_t* hs = hyp + (size_t)r * hyp_stride;
    const int32_t* rs = ref + ref_offsets[ri];
    const int m = es_items(hs, hl, level, space, 0, s);
    const int n = es_items(rs, rl, level, space, 1, s);
    if (tid == 0) s.x[m] = 0;
    __syncthreads();
    for (int d = 1; d <= m + n; ++d) {
        const int lo = max(0, d - n), hi = min(d, m);
        for (int i = lo + tid; i <= hi; i += ES_THREADS) {
            const int j = d - i, slot = j - i + m;
            uint64_t v;
            if (i == 0) {
                v = (uint64_t)j * OP_DEL;
            } else if (j == 0) {
                v = (uint64_t)i * OP_INS;
            } else {
                const uint64_t diag = s.x[slot];
                const int a = s.a[0][i - 1], b = s.a[1][j - 1];
                bool eq;
                if (level == 0) {
                    eq = a == b;
                } else {
                    eq = (a >> 16) == (b >> 16) && s.h[0][i - 1] == s.h[1][j - 1];
                    if (eq) {
                        const int32_t* pa = hs + (a & 0xFFFF);
                        const int32_t* pb = rs + (b & 0xFFFF);
                        for (int q = 0, len = a >> 16; q < len && eq; ++q) eq = pa[q] == pb[q];
                    }
                }
                if (eq) {
                    v = diag;
                } else {
                    v = diag + OP_SUB;
                    const uint64_t del = s.x[slot - 1] + OP_DEL, ins = s.x[slot + 1] + OP_INS;
                    if ((del >> 48) < (v >> 48)) v = del;
                    if ((ins >> 48) < (v >> 48)) v = ins;
                }
            }
            s.x[slot] = v;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t v = s.x[n];      // cell (m, n)
        const int32_t res[5] = {(int32_t)(v >> 48), (int32_t)((v >> 32) & 0xFFFF), (int32_t)((v >> 16) & 0xFFFF),
                                (int32_t)(v & 0xFFFF), n};
        for (int q = 0; q < 5; ++q) {
            out[q] = res[q];
            if (group) atomicAdd((unsigned long long*)(totals + (size_t)g * 10 + 5 * level + q), (unsigned long long)res[q]);
        }
    }
}

}  // namespace

extern "C" size_t ds2_edit_stats_ws_bytes(int R, int hyp_stride, int max_ref_len) {
    (void)R;
    (void)hyp_stride;
    (void)max_ref_len;
    return 0;       // the sweep lives in LDS
}

extern "C" int ds2_edit_stats(const int32_t* hyp, const int32_t* hyp_len, int R, int hyp_stride, const int32_t* ref,
                              const int32_t* ref_offsets, const int32_t* ref_lens, int N, int max_ref_len,
                              const int32_t* ref_index, const int32_t* group, int G, int space_id, void* ws, size_t ws_bytes,
                              int32_t* stats, int64_t* totals, void* stream) {
    (void)ws;
    (void)ws_bytes;
    if (hyp_stride < 0 || hyp_stride > ES_MAX) {
        ds2_set_error("ds2_edit_stats: hyp_stride %d is outside 0..%d (DS2_EDIT_MAX_ITEMS)", hyp_stride, ES_MAX);
        return DS2_ERR_ARG;
    }
    if (max_ref_len < 0 || max_ref_len > ES_MAX) {
        ds2_set_error("ds2_edit_stats: max_ref_len %d is outside 0..%d (DS2_EDIT_MAX_ITEMS)", max_ref_len, ES_MAX);
        return DS2_ERR_ARG;
    }
    DS2_CHECK_ARG(R >= 0 && R <= (1 << 30) && N >= 0 && G >= 0);
    if (R == 0) return DS2_OK;
    DS2_CHECK_ARG(hyp_len && stats && ref_offsets && ref_lens);
    DS2_CHECK_ARG(hyp || hyp_stride == 0);
    DS2_CHECK_ARG(ref || max_ref_len == 0);
    DS2_CHECK_ARG(!group || totals);
    hipLaunchKernelGGL(edit_stats_kernel, dim3(2 * R), dim3(ES_THREADS), 0, (hipStream_t)stream, hyp, hyp_len, hyp_stride, ref,
                       ref_offsets, ref_lens, N, max_ref_len, ref_index, group, G, space_id, stats, (long long*)totals);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
