// Speed perturbation / per-clip ratio on the device (gfx950): B mono int16 clips of a flat buffer, each converted by ITS OWN
// reduced ratio L / M with its own polyphase table, in one launch that reads nothing back.  The arithmetic of a clip is that of
// ds2_resample (csrc/resample.hip) at one channel, operation for operation: one fmaf chain per output from +0 over k = 0 .. K - 1
// upwards, zeros of the padding included, so a clip's output bits equal those of ds2_resample launched on that clip alone
// (include/ds2hip.h, "speed perturbation / per-clip ratio").
//
// The structure is the one resample.hip measured as right (bound by LDS reads): a workgroup produces DS2_RESAMPLE_TILE
// consecutive outputs of one clip (tiles counted from the clip's own start, workgroup x takes tiles x, x + gridDim.x, ...) in
// passes of `sub` outputs whose input span fits the RS_XCAP floats of LDS it is staged into.  Up to DS2_RESAMPLE_VAR_TABLES
// tables travel to the kernel BY VALUE (validated on the host, with their `sub` and their choice "taps in LDS / taps through
// the cache" worked out there); a clip's table id is read from the device and everything that follows from it is uniform over
// the workgroup, so that choice is a uniform branch between two instances of the same loop.  The dynamic LDS is sized for the
// largest LDS-resident table of the launch.  The device cannot report an error: a clip whose table id is outside the list or
// whose length is negative is skipped, and outputs at or past max_out (which sizes the grid) are not written.
#include "ds2_common.h"

namespace {

constexpr int RS_TILE = DS2_RESAMPLE_TILE;             // outputs of one clip per workgroup tile
constexpr int RS_XCAP = 8192;                          // frames staged per pass (32 KiB)
constexpr int RS_TCAP = 24576;                         // taps kept in LDS (96 KiB); a larger table is read through the cache
constexpr int RS_PER = RS_TILE / 256;                  // outputs per lane and pass, at most
constexpr int64_t RS_MAX_GROUPS = 4096;                // workgroups of one launch, about (a longer clip's take several tiles)
static_assert(RS_TILE % 256 == 0 && RS_PER >= 1, "tile geometry");
static_assert(RS_XCAP > 1023 + 1 && (RS_XCAP + RS_TCAP) * 4 <= 160 * 1024, "LDS budget of one CU");

struct VarTable {
    int L, M, K;
    int tap_offset;                                    // floats into the tap bank
    int sub;                                           // outputs per pass: their input span fits RS_XCAP
    int lds;                                           // the (L, K) table fits RS_TCAP: read from LDS
};

struct VarTables {
    VarTable t[DS2_RESAMPLE_VAR_TABLES];
};

// The tiles blockIdx.x, blockIdx.x + gridDim.x, ... of one clip: resample_kernel's loop at C = 1.
template <bool LDS_TAPS>
__device__ __forceinline__ void var_clip(const int16_t* __restrict__ x, int64_t n, int64_t n_out, int L, int M, int K, int sub,
                                         const float* __restrict__ taps, int16_t* __restrict__ y, float* xs, float* ts) {
    const int tid = threadIdx.x;
    const int64_t ntiles = (n_out + RS_TILE - 1) / RS_TILE;
    if (LDS_TAPS)
        for (int i = tid; i < L * K; i += 256) ts[i] = taps[i];           // (visible after the first pass's barrier)
    const int h = (K - 1) >> 1;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t m_end = min((tile + 1) * RS_TILE, n_out);
        for (int64_t ms = tile * RS_TILE; ms < m_end; ms += sub) {
            const int cnt = (int)min((int64_t)sub, m_end - ms);
            const int64_t t0 = ms * M;                                    // int64: positions pass 2^31 in a long clip
            const int64_t base = t0 / L - h;                              // first frame of the pass (may lie before the clip)
            const int r0 = (int)(t0 % L);
            const int span = (r0 + (cnt - 1) * M) / L + K;                // <= RS_XCAP by the choice of sub
            __syncthreads();                                              // the pass before this one has been read
            for (int i = tid; i < span; i += 256) {
                const int64_t j = base + i;
                xs[i] = (j >= 0 && j < n) ? (float)x[j] : 0.f;            // a predicate on the INDEX: nothing outside is loaded
            }
            __syncthreads();
            float acc[RS_PER];
            const float* tp[RS_PER];
            const float* xp[RS_PER];
#pragma unroll
            for (int r = 0; r < RS_PER; ++r) {
                const int d = min(tid + 256 * r, cnt - 1);                // (a lane past the pass recomputes its last output)
                const int u = r0 + d * M;                                 // < 2^10 + 2^10 * 2^12
                tp[r] = (LDS_TAPS ? ts : taps) + (size_t)(u % L) * K;
                xp[r] = xs + u / L;
                acc[r] = 0.f;
            }
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int r = 0; r < RS_PER; ++r) acc[r] = fmaf(tp[r][k], xp[r][k], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < RS_PER; ++r) {
                const int d = tid + 256 * r;
                if (d < cnt) y[ms + d] = (int16_t)(int)fminf(fmaxf(rintf(acc[r]), -32768.f), 32767.f);
            }
        }
    }
}

__global__ __launch_bounds__(256) void resample_var_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ in_offsets,
                                                           const int64_t* __restrict__ out_offsets,
                                                           const int32_t* __restrict__ table_ids, VarTables tables, int n_tables,
                                                           const float* __restrict__ bank, int64_t max_out,
                                                           int16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rsv_lds[];
    float* xs = rsv_lds;                               // [RS_XCAP] the pass's frames
    float* ts = rsv_lds + RS_XCAP;                     // [L * K] of an LDS-resident table
    const int b = blockIdx.y;
    const int id = table_ids[b];
    if (id < 0 || id >= n_tables) return;              // (uniform: the whole workgroup leaves)
    const int64_t lo = in_offsets[b];
    const int64_t n = in_offsets[b + 1] - lo;
    if (n < 0) return;
    const VarTable t = tables.t[id];
    const int64_t n_out = min((n * t.L + t.M - 1) / t.M, max_out);
    if ((int64_t)blockIdx.x * RS_TILE >= n_out) return;
    const int16_t* x = pcm + lo;
    int16_t* y = out + out_offsets[b];
    const float* taps = bank + t.tap_offset;
    if (t.lds)
        var_clip<true>(x, n, n_out, t.L, t.M, t.K, t.sub, taps, y, xs, ts);
    else
        var_clip<false>(x, n, n_out, t.L, t.M, t.K, t.sub, taps, y, xs, ts);
}

}  // namespace

extern "C" int ds2_resample_var(const int16_t* pcm, const int64_t* in_offsets, const int64_t* out_offsets,
                                const int32_t* table_ids, int B, const ds2_resample_table* tables_host, int n_tables,
                                const float* tap_bank, size_t bank_floats, int max_out, int16_t* out, void* stream) {
    DS2_CHECK_ARG(pcm && in_offsets && out_offsets && table_ids && tables_host && tap_bank && out);
    DS2_CHECK_ARG(B >= 1 && B <= 65535);
    DS2_CHECK_ARG(n_tables >= 1 && n_tables <= DS2_RESAMPLE_VAR_TABLES);
    DS2_CHECK_ARG(max_out >= 0);
    VarTables tables = {};
    size_t lds_taps = 0;
    for (int i = 0; i < n_tables; ++i) {
        const ds2_resample_table& s = tables_host[i];
        if (s.L < 1 || s.L > 1024 || s.M < 1 || s.M > 4096 || s.K < 1 || s.K > 1023 || (s.K & 1) != 1) {
            ds2_set_error("ds2_resample_var: table %d has L %d, M %d, K %d; L in 1..1024, M in 1..4096, K odd in 1..1023", i,
                          s.L, s.M, s.K);
            return DS2_ERR_ARG;
        }
        const size_t floats = (size_t)s.L * (size_t)s.K;
        if (s.tap_offset < 0 || (size_t)s.tap_offset > bank_floats || floats > bank_floats - (size_t)s.tap_offset) {
            ds2_set_error("ds2_resample_var: table %d (tap_offset %d, %zu floats) does not lie inside the tap bank of %zu floats",
                          i, s.tap_offset, floats, bank_floats);
            return DS2_ERR_ARG;
        }
        VarTable& t = tables.t[i];
        t.L = s.L, t.M = s.M, t.K = s.K, t.tap_offset = s.tap_offset;
        // outputs per pass: the largest count whose input span, (sub - 1) M / L + 1 + K frames at most, fits the staging buffer
        int64_t sub = (int64_t)(RS_XCAP - s.K - 1) * s.L / s.M + 1;
        t.sub = (int)(sub > RS_TILE ? RS_TILE : sub);
        t.lds = floats <= (size_t)RS_TCAP;
        if (t.lds && floats > lds_taps) lds_taps = floats;
    }
    if (max_out == 0) return DS2_OK;
    const int64_t tiles = ((int64_t)max_out + RS_TILE - 1) / RS_TILE;
    int64_t gx = RS_MAX_GROUPS / B;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    const size_t dyn = ((size_t)RS_XCAP + lds_taps) * sizeof(float);
    if (dyn > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(resample_var_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
        ds2_set_error("ds2_resample_var: %zu bytes of dynamic LDS are not available", dyn);
        return DS2_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(resample_var_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), dyn, (hipStream_t)stream, pcm, in_offsets,
                       out_offsets, table_ids, tables, n_tables, tap_bank, (int64_t)max_out, out);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
