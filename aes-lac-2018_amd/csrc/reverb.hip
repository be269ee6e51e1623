// Reverberation augmentation on the device (gfx950): per clip of a minibatch, y = x * h (a room impulse response of the bank,
// causal, cut to the clip's length), optionally scaled back to the clip's own energy.  The reference has no such stage; the
// rule is written down in include/ds2hip.h under "reverberation".
//
// Compute bound, unlike its neighbours: K taps per output sample.  The sum is a Toeplitz GEMM on the exact-fp32 matrix
// instruction v_mfma_f32_16x16x4_f32: for the 256 outputs y[n0 + i + 16 j] of one tile (i = row, j = column)
//     y[n0 + i + 16 j] = sum_u A[i][u] B[u][j],   A[i][u] = h[i - u] (0 outside [0, K)),   B[u][j] = x[n0 + 16 j + u],
// u = -(K - 1) .. 15, walked upwards (so each output adds its taps from the last one down to h[0], one fma per tap in one
// accumulator: the bits of a plain fmaf chain in that order).  A workgroup of four waves produces RV_TILE consecutive outputs
// of one clip, every wave RV_NT tiles that share the A operand.  Taps and the clip's window go through LDS in passes of RV_STEP
// values of u, fetched into registers one pass ahead; both are zero-filled by a predicate on the INDEX, so nothing outside the
// clip or outside the RIR is ever loaded.  The B operand's stride-16 reads would hit four banks; the window is stored with one pad word per 16 (index r at
// r + r / 16), which spreads the 64 lanes of a read over 61 banks.
//
// The same sum in plain VALU form (reverb_valu_kernel: eight consecutive outputs per lane, a sliding register window) is kept
// beside it as the timing baseline; DS2_REVERB_FORM=valu selects it.
//
// Level: every workgroup leaves ONE (Ex, Ey) float64 pair per tile in ws -- a lane's values in index order, a shuffle tree, the
// four waves in order -- and the scale kernel adds a clip's pairs in index order.  No atomics; a clip's bits depend on the clip
// and its RIR alone.
#include <stdlib.h>
#include <string.h>

#include "ds2_common.h"

namespace {

constexpr int RV_TILE = DS2_REVERB_TILE;               // outputs of one clip per workgroup
constexpr int RV_STEP = DS2_REVERB_TAPS_STEP;          // values of u (taps) staged per pass
constexpr int RV_NT = RV_TILE / (4 * 256);             // 16x16 output tiles per wave
constexpr int RV_XWIN = RV_TILE + RV_STEP;             // clip samples staged per pass
constexpr int RV_HWIN = RV_STEP + 16;                  // taps staged per pass (the 16 rows of A are 16 shifts)
constexpr int64_t RV_MAX_TILES = 1 << 20;              // grid cap: 2^31 samples of one clip in one pass
static_assert(RV_NT >= 1 && RV_TILE == RV_NT * 1024 && RV_STEP % 8 == 0 && RV_TILE % 2048 == 0, "tile geometry");

__device__ __forceinline__ int rv_pad(int r) { return r + (r >> 4); }

struct ReverbClip {
    int64_t lo, n, ntiles;                             // the clip in the flat buffer; its number of workgroup tiles
    int64_t rlo;                                       // its RIR in the bank
    int k;                                             // taps (0: no draw)
};

__device__ inline ReverbClip reverb_clip(const int64_t* __restrict__ offsets, const int64_t* __restrict__ rir_lo,
                                         const int64_t* __restrict__ rir_len, int b) {
    ReverbClip c;
    c.lo = offsets[b];
    c.n = max(offsets[b + 1] - c.lo, (int64_t)0);
    c.ntiles = (c.n + RV_TILE - 1) / RV_TILE;
    c.rlo = rir_lo[b];
    c.k = (int)min(max(rir_len[b], (int64_t)0), (int64_t)DS2_REVERB_MAX_TAPS);
    return c;
}

// One pass's operands on their way from memory to LDS: the window of the clip from xbase (clip-relative) and the taps from
// kbase.  An index outside the clip / the RIR yields 0 and loads the nearest sample INSIDE it instead (n, K >= 1 here), so the
// loads need no branch and still never leave the clip or the RIR.  Loading and storing are separate steps: the loads of the
// next pass are in flight while this one is multiplied.
constexpr int RV_XREG = RV_XWIN / 256, RV_HREG = (RV_HWIN + 255) / 256;
static_assert(RV_XWIN % 256 == 0, "the window is staged in whole rounds of the workgroup");
struct ReverbStage {
    float xv[RV_XREG], hv[RV_HREG];
};

__device__ __forceinline__ void reverb_load(ReverbStage& st, const float* __restrict__ x, const float* __restrict__ h,
                                            const ReverbClip& c, int64_t xbase, int kbase, int tid) {
#pragma unroll
    for (int i = 0; i < RV_XREG; ++i) {
        const int64_t idx = xbase + tid + 256 * i;
        const float v = x[min(max(idx, (int64_t)0), c.n - 1)];
        st.xv[i] = (idx >= 0 && idx < c.n) ? v : 0.f;
    }
#pragma unroll
    for (int i = 0; i < RV_HREG; ++i) {
        const int k = kbase + tid + 256 * i;
        const float v = h[min(max(k, 0), c.k - 1)];
        st.hv[i] = (k >= 0 && k < c.k) ? v : 0.f;
    }
}

__device__ __forceinline__ void reverb_store(const ReverbStage& st, float* xs, float* hs, int tid) {
#pragma unroll
    for (int i = 0; i < RV_XREG; ++i) xs[rv_pad(tid + 256 * i)] = st.xv[i];
#pragma unroll
    for (int i = 0; i < RV_HREG; ++i)
        if (tid + 256 * i < RV_HWIN) hs[tid + 256 * i] = st.hv[i];
}

// first pass of the tile at m0 whose window reaches the clip: in the passes before it every product is 0
__device__ __forceinline__ int reverb_first_pass(const ReverbClip& c, int64_t m0) {
    const int64_t d = (int64_t)c.k - RV_XWIN - m0;                       // a pass at v0 < d lies wholly before the clip
    return d <= 0 ? 0 : (int)((d + RV_STEP - 1) / RV_STEP) * RV_STEP;
}

// a clip without a draw: the tile is copied bit for bit
__device__ __forceinline__ void reverb_copy_tile(const float* wav, float* out, const ReverbClip& c, int64_t m0, int tid) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(wav + c.lo);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + c.lo);
    for (int64_t i = m0 + tid, i1 = min(m0 + RV_TILE, c.n); i < i1; i += 256) dst[i] = src[i];
}

// (Ex, Ey) of a workgroup's tiles into its slot: ex, ey are the lanes' own sums
__device__ __forceinline__ void reverb_partial(double ex, double ey, double (*part)[4], double* slot, int tid) {
    ex = wave_sum_d(ex);
    ey = wave_sum_d(ey);
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = ex;
        part[1][tid >> 6] = ey;
    }
    __syncthreads();
    if (tid == 0) {
        slot[0] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
        slot[1] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
}

__device__ __forceinline__ double reverb_ex_tile(const float* __restrict__ x, const ReverbClip& c, int64_t m0, int tid) {
    double ex = 0.0;
    for (int64_t i = m0 + tid, i1 = min(m0 + RV_TILE, c.n); i < i1; i += 256) {
        const double v = (double)x[i];
        ex = fma(v, v, ex);                            // float operand: the product is exact in double
    }
    return ex;
}

// Workgroup (x, b) produces tiles x, x + gridDim.x, ... of clip b (one tile when the workspace was sized by
// ds2_reverb_ws_bytes for the longest clip).  out never aliases wav (refused by the host).
__global__ __launch_bounds__(256) void reverb_mfma_kernel(const float* __restrict__ wav, const int64_t* __restrict__ offsets,
                                                          const float* __restrict__ bank,
                                                          const int64_t* __restrict__ rir_lo,
                                                          const int64_t* __restrict__ rir_len, int keep_level,
                                                          float* __restrict__ out, float* __restrict__ gain,
                                                          double* __restrict__ ws) {
    __shared__ float xs[RV_XWIN + RV_XWIN / 16 + 1];
    __shared__ float hs[RV_HWIN];
    __shared__ double part[2][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const ReverbClip c = reverb_clip(offsets, rir_lo, rir_len, b);
    if (blockIdx.x == 0 && tid == 0 && gain && (!keep_level || c.k == 0 || c.n == 0)) gain[b] = 1.f;
    if ((int64_t)blockIdx.x >= c.ntiles) return;
    if (c.k == 0) {
        for (int64_t t = blockIdx.x; t < c.ntiles; t += gridDim.x) reverb_copy_tile(wav, out, c, t * RV_TILE, tid);
        return;
    }
    const float* x = wav + c.lo;
    const float* h = bank + c.rlo;
    float* y = out + c.lo;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int nv = c.k + 15;                           // values of u
    double ex = 0.0, ey = 0.0;
    for (int64_t t = blockIdx.x; t < c.ntiles; t += gridDim.x) {
        const int64_t m0 = t * RV_TILE;
        f32x4 acc[RV_NT];
#pragma unroll
        for (int a = 0; a < RV_NT; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
        int v0 = reverb_first_pass(c, m0);
        ReverbStage st;
        if (v0 < nv) reverb_load(st, x, h, c, m0 + v0 - (c.k - 1), c.k - v0 - RV_STEP, tid);
        for (; v0 < nv; v0 += RV_STEP) {
            __syncthreads();                           // the pass before this one has been read
            reverb_store(st, xs, hs, tid);
            __syncthreads();
            if (v0 + RV_STEP < nv) reverb_load(st, x, h, c, m0 + v0 + RV_STEP - (c.k - 1), c.k - v0 - 2 * RV_STEP, tid);
            // sixteen values of u per round, four steps of four.  Lane (j, g) at step s: A = h[j - u] = hs[j + RV_STEP - 1 -
            // 4 s - g];  B = xs[tile + 16 j + 4 s + g], padded: 17 per 16.  Steps past u = 15 find A = 0.
            const int rounds = (min(RV_STEP, nv - v0) + 15) >> 4;
            const float* ha = hs + j + RV_STEP - 1 - g;
            const float* xb = xs + wave * RV_NT * 272 + 17 * j + g;
            for (int rd = 0; rd < rounds; ++rd, ha -= 16, xb += 17) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float av = ha[-4 * s];
#pragma unroll
                    for (int a = 0; a < RV_NT; ++a)
                        acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[a * 272 + 4 * s], acc[a], 0, 0, 0);
                }
            }
        }
        // C/D: column j = lane & 15, rows 4 g .. 4 g + 3: four consecutive samples per lane
#pragma unroll
        for (int a = 0; a < RV_NT; ++a) {
            const int64_t n = m0 + (wave * RV_NT + a) * 256 + 16 * j + 4 * g;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < c.n) {
                    const float v = acc[a][r];
                    y[n + r] = v;
                    ey = fma((double)v, (double)v, ey);
                }
        }
        if (keep_level) ex += reverb_ex_tile(x, c, m0, tid);
    }
    if (keep_level) reverb_partial(ex, ey, part, ws + ((int64_t)b * gridDim.x + blockIdx.x) * 2, tid);
}

// The same sum on the vector ALU: lane tid owns outputs m0 + 8 tid .. + 7; per tap one new window value and eight fmaf.
// Every output adds its taps from the last one down to h[0] as the matrix form does, without that form's zero products.
__global__ __launch_bounds__(256) void reverb_valu_kernel(const float* __restrict__ wav, const int64_t* __restrict__ offsets,
                                                          const float* __restrict__ bank,
                                                          const int64_t* __restrict__ rir_lo,
                                                          const int64_t* __restrict__ rir_len, int keep_level,
                                                          float* __restrict__ out, float* __restrict__ gain,
                                                          double* __restrict__ ws) {
    __shared__ float xs[RV_XWIN + RV_XWIN / 16 + 1];
    __shared__ float hs[RV_HWIN];
    __shared__ double part[2][4];
    constexpr int PER = RV_TILE / 256;
    static_assert(PER == 8, "the register window is written for eight outputs per lane");
    const int b = blockIdx.y, tid = threadIdx.x;
    const ReverbClip c = reverb_clip(offsets, rir_lo, rir_len, b);
    if (blockIdx.x == 0 && tid == 0 && gain && (!keep_level || c.k == 0 || c.n == 0)) gain[b] = 1.f;
    if ((int64_t)blockIdx.x >= c.ntiles) return;
    if (c.k == 0) {
        for (int64_t t = blockIdx.x; t < c.ntiles; t += gridDim.x) reverb_copy_tile(wav, out, c, t * RV_TILE, tid);
        return;
    }
    const float* x = wav + c.lo;
    const float* h = bank + c.rlo;
    float* y = out + c.lo;
    double ex = 0.0, ey = 0.0;
    for (int64_t t = blockIdx.x; t < c.ntiles; t += gridDim.x) {
        const int64_t m0 = t * RV_TILE;
        float acc[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) acc[i] = 0.f;
        // pass p holds taps [K - (p + 1) STEP, K - p STEP) at hs[0 .. STEP) and the window from m0 - (K - 1) + p STEP:
        // tap hs[q] meets output m0 + o at xs[o + STEP - 1 - q]
        int v0 = reverb_first_pass(c, m0);
        ReverbStage st;
        if (v0 < c.k) reverb_load(st, x, h, c, m0 + v0 - (c.k - 1), c.k - v0 - RV_STEP, tid);
        for (; v0 < c.k; v0 += RV_STEP) {
            __syncthreads();
            reverb_store(st, xs, hs, tid);
            __syncthreads();
            if (v0 + RV_STEP < c.k) reverb_load(st, x, h, c, m0 + v0 + RV_STEP - (c.k - 1), c.k - v0 - 2 * RV_STEP, tid);
            float w[2 * PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) w[i] = xs[rv_pad(PER * tid + i)];
            for (int d0 = 0; d0 < RV_STEP; d0 += PER) {
#pragma unroll
                for (int i = 0; i < PER; ++i) w[PER + i] = xs[rv_pad(PER * tid + d0 + PER + i)];
#pragma unroll
                for (int dd = 0; dd < PER; ++dd) {
                    const float tap = hs[RV_STEP - 1 - d0 - dd];
#pragma unroll
                    for (int i = 0; i < PER; ++i) acc[i] = fmaf(tap, w[dd + i], acc[i]);
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) w[i] = w[PER + i];
            }
        }
        const int64_t n = m0 + PER * tid;
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (n + i < c.n) {
                y[n + i] = acc[i];
                ey = fma((double)acc[i], (double)acc[i], ey);
            }
        if (keep_level) ex += reverb_ex_tile(x, c, m0, tid);
    }
    if (keep_level) reverb_partial(ex, ey, part, ws + ((int64_t)b * gridDim.x + blockIdx.x) * 2, tid);
}

// Scale: the same grid.  Every workgroup adds up its clip's pairs in index order (every lane the same loads: they come from
// L2), derives the gain and scales its tiles of out in place, one rounded multiply per sample.
__global__ __launch_bounds__(256) void reverb_scale_kernel(const int64_t* __restrict__ offsets,
                                                           const int64_t* __restrict__ rir_lo,
                                                           const int64_t* __restrict__ rir_len,
                                                           const double* __restrict__ ws, float* __restrict__ out,
                                                           float* __restrict__ gain) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const ReverbClip c = reverb_clip(offsets, rir_lo, rir_len, b);
    if ((int64_t)blockIdx.x >= c.ntiles || c.k == 0) return;    // (gain = 1 of such a clip: written by the first kernel)
    const int64_t np = min(c.ntiles, (int64_t)gridDim.x);
    const double* slot = ws + (int64_t)b * gridDim.x * 2;
    double ex = 0.0, ey = 0.0;
    for (int64_t k = 0; k < np; ++k) {
        ex += slot[2 * k];
        ey += slot[2 * k + 1];
    }
    float gn = 1.f;
    if (ey > 0.0) {
        const float f = (float)sqrt(ex / ey);
        if (isfinite(f)) gn = f;
    }
    if (blockIdx.x == 0 && tid == 0 && gain) gain[b] = gn;
    if (gn == 1.f) return;
    float* y = out + c.lo;
    for (int64_t t = blockIdx.x; t < c.ntiles; t += gridDim.x)
        for (int64_t i = t * RV_TILE + tid, i1 = min((t + 1) * RV_TILE, c.n); i < i1; i += 256) y[i] = __fmul_rn(gn, y[i]);
}

}  // namespace

extern "C" size_t ds2_reverb_ws_bytes(int B, size_t max_clip_len) {
    if (B < 1) B = 1;
    size_t tiles = (max_clip_len + RV_TILE - 1) / RV_TILE;
    if (tiles < 1) tiles = 1;
    if (tiles > (size_t)RV_MAX_TILES) tiles = (size_t)RV_MAX_TILES;
    return (size_t)B * tiles * 2 * sizeof(double);
}

extern "C" int ds2_reverb(const float* wav, const int64_t* offsets, int B, const float* bank, const int64_t* rir_lo,
                          const int64_t* rir_len, int keep_level, float* out, float* gain, void* ws, size_t ws_bytes,
                          void* stream) {
    DS2_CHECK_ARG(wav && offsets && bank && rir_lo && rir_len && out && ws);
    DS2_CHECK_ARG(out != wav);                                           // out of place: every output reads K inputs
    DS2_CHECK_ARG(B >= 1 && B <= 65535 && (keep_level == 0 || keep_level == 1));
    DS2_CHECK_ARG(ws_bytes >= (size_t)B * 2 * sizeof(double));           // at least one pair per clip
    // the workspace fixes the grid: ws_bytes / (16 B) tiles per clip (a longer clip's workgroups take several tiles each)
    size_t tiles = ws_bytes / ((size_t)B * 2 * sizeof(double));
    if (tiles > (size_t)RV_MAX_TILES) tiles = (size_t)RV_MAX_TILES;
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const char* form = getenv("DS2_REVERB_FORM");                        // selection switch: "valu" = the timing baseline
    if (form && !strcmp(form, "valu"))
        hipLaunchKernelGGL(reverb_valu_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, offsets, bank, rir_lo, rir_len,
                           keep_level, out, gain, (double*)ws);
    else
        hipLaunchKernelGGL(reverb_mfma_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, offsets, bank, rir_lo, rir_len,
                           keep_level, out, gain, (double*)ws);
    DS2_CHECK_LAUNCH();
    if (keep_level) {
        hipLaunchKernelGGL(reverb_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, offsets, rir_lo, rir_len,
                           (const double*)ws, out, gain);
        DS2_CHECK_LAUNCH();
    }
    return DS2_OK;
}
