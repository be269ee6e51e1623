// The parts of the CTC forward-backward that ctc.hip (ds2_ctc_loss_grad) and ctc_mwer.hip (ds2_ctc_mwer_grad) share: the bounded
// fp32 log-sum-exp helpers, the per-frame row log-sum-exp kernel and ONE row's alpha / beta recursion.  ctc.hip's header comment
// has the scheme (K0, K1) and the reasons; the code below is what stood there, with the recursion's per-utterance pointers
// (labels, time length, output row, cost slots) made arguments so that many label rows can share one utterance's activations.
#pragma once
#include "ds2_common.h"

namespace {

constexpr int MAX_S = 1024;  // 2*L+1 <= 1024
#define NEG_INF_D (-(double)INFINITY)

// exp / log of the bounded part on the hardware exp2 / log2 units (1 ulp): arguments are <= 0 and the sum lies in
// [1, 3], so no range handling is needed; the library expf / logf cost ~100 more instructions per state per frame on
// the recursion's critical path (0.75 -> 0.5 us per frame).
__device__ __forceinline__ float exp_neg(float x) { return __builtin_amdgcn_exp2f(1.4426950408889634f * x); }
__device__ __forceinline__ float log_1to3(float s) { return 0.6931471805599453f * __builtin_amdgcn_logf(s); }

// log(1 + x) for x in [0, 2]: the series below 1/64 (next term x^5 / 5: 1e-8 relative), where 1 + x would round x away
__device__ __forceinline__ float log1p_0to2(float x) {
    const float small = x * (1.f - x * (0.5f - x * (0.33333334f - x * 0.25f)));
    return x < 0.015625f ? small : log_1to3(1.f + x);
}

__device__ __forceinline__ double lse2m(double a, double b) {
    const double m = fmax(a, b);
    if (m == NEG_INF_D) return m;
    return m + (double)log1p_0to2(exp_neg((float)(fmin(a, b) - m)));
}
__device__ __forceinline__ double lse3m(double a, double b, double c) {
    const double m = fmax(fmax(a, b), c);
    if (m == NEG_INF_D) return m;
    const float da = (float)(a - m), db = (float)(b - m), dc = (float)(c - m);      // one of them is 0: the largest term, exp = 1
    const float lo = fminf(fminf(da, db), dc), mid = __builtin_amdgcn_fmed3f(da, db, dc);
    return m + (double)log1p_0to2(exp_neg(lo) + exp_neg(mid));
}

__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ acts, int rows, int A,
                                                      float* __restrict__ rmx, float* __restrict__ rl1p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* p = acts + (size_t)row * A;
    float mx = -INFINITY;
    for (int k = lane; k < A; k += 64) mx = fmaxf(mx, p[k]);
    mx = wave_max(mx);
    float s = 0.f, nmax = 0.f;                          // the entries equal to the maximum are counted, not exponentiated
    for (int k = lane; k < A; k += 64) {
        const float v = p[k];
        if (v == mx) nmax += 1.f;
        else s += expf(v - mx);
    }
    s = wave_sum(s);
    nmax = wave_sum(nmax);
    if (lane == 0) {
        rmx[row] = mx;
        rl1p[row] = log1pf(s + (nmax - 1.f));
    }
}

// One state per thread: NTHR = 256 / 512 / 1024 threads for up to that many states (2 L + 1 of the longest transcript of the
// minibatch), so a minibatch of short transcripts does not pay the barrier of sixteen waves.
//
// Emissions.  State s of frame t needs (acts[t][b][ext[s]] - rmx[t][b]) - rl1p[t][b].  Fetched per frame they put a global-memory round
// trip on every step of the recursion (round 1-3: a "prefetch" whose subtraction made the compiler wait for it at once, and a
// vmcnt(0) that also covered the previous frame's alpha / beta store: 0.47 us per frame, 185 us for T = 391).  Now whole
// frames are staged through LDS, CH at a time: the loads of chunk c + 1 are issued before chunk c's first frame and land in
// the other LDS buffer at its last one -- one memory wait per CH frames, and a frame is LDS reads -> log-sum-exp -> LDS write
// -> barrier.
constexpr int EM_FLOATS = 1024;          // per buffer: CH = min(32, 1024 / A) frames (A = 29: 32, A = 43: 23, A = 256: 4)
constexpr int EM_NLD = 4;                // staging loads per thread and chunk (256 threads do the staging)

// One label row's recursion in one direction (dirn 0: alpha, forward in time; 1: beta, backward), run by a whole workgroup of
// NTHR threads.  lab / L: the row's labels; b: the column of acts (T,B,A) it reads; tl: its frame count (already clamped to T);
// out: the row's (T, smax) alpha or beta plane; ll_out / cost: where direction 0 leaves log p and -log p.
template <int NTHR>
__device__ __forceinline__ void ctc_alphabeta_row(
    const float* __restrict__ acts, const float* __restrict__ rmx, const float* __restrict__ rl1p,
    const int32_t* __restrict__ lab, const int L, const int tl, const int b, const int dirn, int T, int B, int A, int smax,
    double* __restrict__ out, double* __restrict__ ll_out, float* __restrict__ cost) {
    __shared__ int ext[MAX_S];
    __shared__ double rowbuf[2][MAX_S + 4];
    __shared__ float em[2][EM_FLOATS];

    const int tid = threadIdx.x;
    const int S = 2 * L + 1;
    for (int s = tid; s < S; s += NTHR) ext[s] = (s & 1) ? lab[s >> 1] : 0;
    for (int i = tid; i < MAX_S + 4; i += NTHR) {
        rowbuf[0][i] = NEG_INF_D;
        rowbuf[1][i] = NEG_INF_D;
    }
    __syncthreads();
    if (tl <= 0) {
        if (dirn == 0 && tid == 0) {
            const float c = (L == 0) ? 0.f : INFINITY;
            *cost = c;
            *ll_out = -(double)c;
        }
        return;
    }
    const int s = tid;
    const bool live = s < S;
    const int sym = live ? ext[s] : 0;
    const bool skip = dirn == 0 ? (live && (s >= 2) && (ext[s] != 0) && (ext[s] != ext[s - 2]))
                                : ((s + 2 < S) && (ext[s] != 0) && (ext[s] != ext[s + 2]));
    // rowbuf[.][s + 1] holds state s; cells 0 and S+1.. stay -inf guards
    const int i1 = dirn == 0 ? s : s + 2, i2 = dirn == 0 ? max(s - 1, 0) : s + 3;     // cells of the two other predecessors
    const int tstart = dirn == 0 ? 0 : tl - 1;
    const int tstep = dirn == 0 ? 1 : -1;
    if (live) {
        const float* arow = acts + ((size_t)tstart * B + b) * A;
        const float m0 = rmx[(size_t)tstart * B + b], p0 = rl1p[(size_t)tstart * B + b];
        const bool on = dirn == 0 ? (s <= 1) : (s >= S - 2);
        const double v = on ? (double)((arow[sym] - m0) - p0) : NEG_INF_D;
        rowbuf[0][s + 1] = v;
        out[(size_t)tstart * smax + s] = v;
    }
    // staging roles: thread tid < 256 carries elements idx = tid + 256 i of a chunk, idx = f A + k (frame f of the chunk, symbol k)
    const int CH = min(32, EM_FLOATS / A), nper = CH * A;
    const int nsteps = tl - 1;                          // recursion steps 1 .. tl - 1; step n works on frame tstart + tstep n
    const int nchunk = (nsteps + CH - 1) / CH;
    int st_f[EM_NLD], st_k[EM_NLD];
#pragma unroll
    for (int i = 0; i < EM_NLD; ++i) {
        const int idx = tid + 256 * i;
        st_f[i] = (tid < 256 && idx < nper) ? idx / A : -1;
        st_k[i] = idx - (idx / A) * A;
    }
    float ra[EM_NLD], rl[EM_NLD], rp[EM_NLD];
    auto stage_load = [&](int c) {
#pragma unroll
        for (int i = 0; i < EM_NLD; ++i) {
            ra[i] = rl[i] = rp[i] = 0.f;
            const int n = 1 + c * CH + st_f[i];
            if (st_f[i] >= 0 && n < tl) {
                const size_t row = (size_t)(tstart + tstep * n) * B + b;
                ra[i] = acts[row * A + st_k[i]];
                rl[i] = rmx[row];
                rp[i] = rl1p[row];
            }
        }
    };
    auto stage_store = [&](float* dst) {
#pragma unroll
        for (int i = 0; i < EM_NLD; ++i)
            if (st_f[i] >= 0) {
                float a = ra[i];
                asm volatile("" : "+v"(a));      // keeps the subtraction (and with it the wait for the loads) HERE, at the chunk's
                dst[tid + 256 * i] = (a - rl[i]) - rp[i];  // last frame: hoisted in front of the frame loop it would wait at the chunk's first
            }
    };
    if (nchunk > 0) {
        stage_load(0);
        stage_store(em[0]);
    }
    __syncthreads();
    int cur = 0;
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        if (more) stage_load(c + 1);                    // in flight while this chunk's frames are worked on
        const float* e = em[c & 1] + sym;
        const int fend = min(CH, nsteps - c * CH);
        int t = tstart + tstep * (1 + c * CH);
        for (int f = 0; f < fend; ++f) {
            const double* prev = rowbuf[cur];
            double* nxt = rowbuf[cur ^ 1];
            if (live) {
                // all four LDS reads go out together (the third predecessor is read whether it counts or not)
                const double x0 = prev[s + 1], x1 = prev[i1], x2r = prev[i2];
                const float ev = e[f * A];
                const double val = lse3m(x0, x1, skip ? x2r : NEG_INF_D) + (double)ev;
                nxt[s + 1] = val;
                out[(size_t)t * smax + s] = val;
            }
            if (more && f == fend - 1) stage_store(em[(c + 1) & 1]);    // (its last readers passed chunk c - 1's final barrier)
            __syncthreads();
            cur ^= 1;
            t += tstep;
        }
    }
    if (dirn == 0 && tid == 0) {
        const double* last = rowbuf[cur];
        const double ll = lse2m(last[S], S > 1 ? last[S - 1] : NEG_INF_D);  // states S-1 and S-2
        *ll_out = ll;
        *cost = (float)(-ll);
    }
}

}  // namespace
