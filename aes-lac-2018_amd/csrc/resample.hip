// Sample-rate conversion on the device (gfx950): B interleaved int16 clips of a flat buffer are mixed down to mono and
// converted by the reduced ratio L / M with a polyphase FIR, int16 out.  The reference piped its files through sox; the rule
// here is written down in include/ds2hip.h under "sample-rate conversion".
//
// A workgroup produces DS2_RESAMPLE_TILE consecutive outputs of one clip (tiles counted from the clip's own start, workgroup x
// takes tiles x, x + gridDim.x, ...), in passes of `sub` outputs whose downmixed input span (sub * M / L + K frames) fits the
// RS_XCAP floats of LDS it is staged into; frames outside the clip are zeros by a predicate on the INDEX, so nothing outside
// the clip is loaded.  Lane d of a pass owns outputs d, d + 256, ...: its tap row p = (m M) mod L and its first frame m M / L
// come from the pass's own (int64) start plus a 32-bit remainder.  The taps are read from LDS where the whole (L, K) table fits
// RS_TCAP floats (every L = 1 table: all lanes read one address, a broadcast; the 160 x 141 table of 44.1 kHz: K is odd, so
// rows p and p + 1 start an odd number of banks apart) and through the cache otherwise.  Each output is ONE chain of fmaf over
// k = 0 .. K - 1 upwards from +0, zeros of the padding included: the bits do not depend on the tile, the pass or the grid.
#include <vector>

#include "ds2_common.h"

namespace {

constexpr int RS_TILE = DS2_RESAMPLE_TILE;             // outputs of one clip per workgroup tile
constexpr int RS_XCAP = 8192;                          // downmixed frames staged per pass (32 KiB)
constexpr int RS_TCAP = 24576;                         // taps kept in LDS (96 KiB); a larger table is read through the cache
constexpr int RS_PER = RS_TILE / 256;                  // outputs per lane and pass, at most
constexpr int64_t RS_MAX_GROUPS = 4096;                // workgroups of one launch, about (a longer clip's take several tiles)
static_assert(RS_TILE % 256 == 0 && RS_PER >= 1, "tile geometry");
static_assert(RS_XCAP > 1023 + 1 && (RS_XCAP + RS_TCAP) * 4 <= 160 * 1024, "LDS budget of one CU");

template <bool LDS_TAPS>
__global__ __launch_bounds__(256) void resample_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ in_offsets,
                                                       int C, int L, int M, const float* __restrict__ taps, int K,
                                                       int16_t* __restrict__ out, const int64_t* __restrict__ out_offsets,
                                                       int sub, float inv_c) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* xs = rs_lds;                                // [RS_XCAP] the pass's frames, downmixed
    float* ts = rs_lds + RS_XCAP;                      // [L * K] with LDS_TAPS
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t lo = in_offsets[b];
    const int64_t n = max(in_offsets[b + 1] - lo, (int64_t)0) / C;       // frames
    const int64_t n_out = (n * L + M - 1) / M;
    const int64_t ntiles = (n_out + RS_TILE - 1) / RS_TILE;
    if ((int64_t)blockIdx.x >= ntiles) return;
    if (LDS_TAPS)
        for (int i = tid; i < L * K; i += 256) ts[i] = taps[i];           // (visible after the first pass's barrier)
    const int16_t* x = pcm + lo;
    int16_t* y = out + out_offsets[b];
    const int h = (K - 1) >> 1;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t m_end = min((tile + 1) * RS_TILE, n_out);
        for (int64_t ms = tile * RS_TILE; ms < m_end; ms += sub) {
            const int cnt = (int)min((int64_t)sub, m_end - ms);
            const int64_t t0 = ms * M;                                    // int64: an hour at M = 441 passes 2^31
            const int64_t base = t0 / L - h;                              // first frame of the pass (may lie before the clip)
            const int r0 = (int)(t0 % L);
            const int span = (r0 + (cnt - 1) * M) / L + K;                // <= RS_XCAP by the choice of sub
            __syncthreads();                                              // the pass before this one has been read
            for (int i = tid; i < span; i += 256) {
                const int64_t j = base + i;
                float v = 0.f;
                if (j >= 0 && j < n) {
                    const int16_t* q = x + j * C;
                    int s = 0;
                    for (int c = 0; c < C; ++c) s += q[c];
                    v = (float)s;                                         // |s| <= 2^18: exact
                }
                xs[i] = v;
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
                if (d < cnt) {
                    const float v = C > 1 ? __fmul_rn(acc[r], inv_c) : acc[r];
                    y[ms + d] = (int16_t)(int)fminf(fmaxf(rintf(v), -32768.f), 32767.f);
                }
            }
        }
    }
}

}  // namespace

extern "C" size_t ds2_resample_out_len(size_t n_frames, int L, int M) {
    if (L < 1 || M < 1) return 0;
    return (n_frames * (size_t)L + (size_t)M - 1) / (size_t)M;
}

extern "C" int ds2_resample(const int16_t* pcm, const int64_t* in_offsets, int B, int channels, int L, int M,
                            const float* taps, int K, int16_t* out, const int64_t* out_offsets, void* stream) {
    DS2_CHECK_ARG(pcm && in_offsets && taps && out && out_offsets);
    DS2_CHECK_ARG(B >= 1 && B <= 65535 && channels >= 1 && channels <= 8);
    DS2_CHECK_ARG(L >= 1 && L <= 1024 && M >= 1 && M <= 4096);
    DS2_CHECK_ARG(K >= 1 && K <= 1023 && (K & 1) == 1);
    // The clip lengths are checked before anything is written, and the longest clip sizes the grid: the B + 1 input offsets are
    // read back here (the one wait of this entry point; the launch itself is enqueued as everywhere else).
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> off((size_t)B + 1);
    DS2_HIP(hipMemcpyAsync(off.data(), in_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    DS2_HIP(hipStreamSynchronize(st));
    int64_t longest = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t len = off[b + 1] - off[b];
        if (off[b] < 0 || len < 0 || len % channels != 0) {
            ds2_set_error("ds2_resample: clip %d spans elements %lld .. %lld: not a whole number of %d-channel frames", b,
                          (long long)off[b], (long long)off[b + 1], channels);
            return DS2_ERR_ARG;
        }
        if (len / channels > longest) longest = len / channels;
    }
    DS2_CHECK_ARG(longest <= (int64_t)1 << 40);                          // (n L stays far inside int64)
    const int64_t n_out = (longest * L + M - 1) / M;
    if (n_out == 0) return DS2_OK;
    const int64_t tiles = (n_out + RS_TILE - 1) / RS_TILE;
    int64_t gx = RS_MAX_GROUPS / B;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    // outputs per pass: the largest count whose input span, (sub - 1) M / L + 1 + K frames at most, fits the staging buffer
    int64_t sub = (int64_t)(RS_XCAP - K - 1) * L / M + 1;
    if (sub > RS_TILE) sub = RS_TILE;
    const bool lds_taps = (int64_t)L * K <= RS_TCAP;
    const size_t dyn = ((size_t)RS_XCAP + (lds_taps ? (size_t)L * K : 0)) * sizeof(float);
    auto kernel = lds_taps ? resample_kernel<true> : resample_kernel<false>;
    if (dyn > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) !=
            hipSuccess) {
        ds2_set_error("ds2_resample: %zu bytes of dynamic LDS are not available (L %d, K %d)", dyn, L, K);
        return DS2_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), dyn, st, pcm, in_offsets, channels, L, M, taps, K, out,
                       out_offsets, (int)sub, 1.0f / (float)channels);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
