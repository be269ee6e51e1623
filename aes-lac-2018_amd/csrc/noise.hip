// Noise-injection augmentation on the device (gfx950): out = wav + coef * noise, per clip of a minibatch, with
// coef = level * rms(wav) / rms(noise crop).  Stands where the reference's NoiseInjection.__call__ would run
// (codes/transforms.py:254-287, between ToTensor and ToSpectrogram); that class raises on its first call, so the semantics are
// its evident intent, written down in include/ds2hip.h.
//
// Bandwidth bound: per sample 4 B of speech + 2 B of noise are read twice (energy, then mix) and 4 B are written.  Two kernels
// with the launch boundary as the only synchronisation.  Every sum has a fixed order -- a lane's samples in index order, a
// shuffle tree, the four waves in order, a clip's chunk partials in index order -- and is taken in float64 over exact products,
// so a clip's output bits depend on nothing but the clip, its draw and the size of the workspace.  No atomics.
#include "ds2_common.h"

namespace {

constexpr int NZ_CHUNK = DS2_NOISE_CHUNK;              // samples one workgroup handles per pass (include/ds2hip.h)
constexpr int64_t NZ_MAX_CHUNKS = 1 << 20;             // grid cap: 2^32 samples of one clip in one pass

struct NoiseClip {
    int64_t lo, n, nchunks;                            // the clip in the flat buffer; its number of chunks
    int64_t nlo, nlen, start;                          // its recording in the bank, and the first sample of the crop
};

__device__ inline NoiseClip noise_clip(const int64_t* __restrict__ offsets, const int64_t* __restrict__ noise_lo,
                                       const int64_t* __restrict__ noise_len, const int64_t* __restrict__ noise_start,
                                       int b) {
    NoiseClip c;
    c.lo = offsets[b];
    c.n = offsets[b + 1] - c.lo;
    c.nchunks = (c.n + NZ_CHUNK - 1) / NZ_CHUNK;
    c.nlo = noise_lo[b];
    c.nlen = noise_len[b] > 0 ? noise_len[b] : 0;
    c.start = c.nlen > 0 ? min(max(noise_start[b], (int64_t)0), c.nlen - 1) : 0;    // never outside the recording
    return c;
}

// position in the recording of clip sample i (the recording repeats when it is shorter than the clip)
__device__ inline int64_t noise_pos(const NoiseClip& c, int64_t i) { return (c.start + i) % c.nlen; }

// Energy: workgroup (x, b) sums chunks x, x + gridDim.x, ... of clip b (one chunk when the workspace was sized by
// ds2_noise_mix_ws_bytes for the longest clip) and writes ONE (Ex, En) pair.  wav is read before the mix kernel may
// overwrite it in place: no __restrict__.
__global__ __launch_bounds__(256) void noise_energy_kernel(const float* wav, const int64_t* __restrict__ offsets,
                                                           const int16_t* __restrict__ bank,
                                                           const int64_t* __restrict__ noise_lo,
                                                           const int64_t* __restrict__ noise_len,
                                                           const int64_t* __restrict__ noise_start, float noise_scale,
                                                           double* __restrict__ ws) {
    __shared__ double part[2][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const NoiseClip c = noise_clip(offsets, noise_lo, noise_len, noise_start, b);
    if ((int64_t)blockIdx.x >= c.nchunks || c.nlen == 0) return;         // past the clip's end, or no noise drawn
    const float* x = wav + c.lo;
    const int16_t* rec = bank + c.nlo;
    const int64_t step = 256 % c.nlen;
    double ex = 0.0, en = 0.0;
    for (int64_t ch = blockIdx.x; ch < c.nchunks; ch += gridDim.x) {
        const int64_t i0 = ch * NZ_CHUNK + tid, i1 = min((ch + 1) * NZ_CHUNK, c.n);
        int64_t p = i0 < i1 ? noise_pos(c, i0) : 0;
        for (int64_t i = i0; i < i1; i += 256) {
            const double xv = (double)x[i];
            const double nv = (double)__fmul_rn((float)rec[p], noise_scale);
            ex = fma(xv, xv, ex);                                         // float operands: the product is exact in double
            en = fma(nv, nv, en);
            p += step;
            if (p >= c.nlen) p -= c.nlen;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ex += __shfl_xor(ex, o, 64);
        en += __shfl_xor(en, o, 64);
    }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = ex;
        part[1][tid >> 6] = en;
    }
    __syncthreads();
    if (tid == 0) {
        double* slot = ws + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
        slot[0] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
        slot[1] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
}

// Mix: the same grid.  Every workgroup adds up its clip's partials in index order (every lane the same loads: they come from
// L2), derives coef, and writes its chunks of out.  coef == 0 (level 0, a silent crop or clip, no noise drawn) copies wav.
__global__ __launch_bounds__(256) void noise_mix_kernel(const float* wav, const int64_t* __restrict__ offsets,
                                                        const int16_t* __restrict__ bank,
                                                        const int64_t* __restrict__ noise_lo,
                                                        const int64_t* __restrict__ noise_len,
                                                        const int64_t* __restrict__ noise_start,
                                                        const float* __restrict__ level, float noise_scale,
                                                        const double* __restrict__ ws, float* out,
                                                        float* __restrict__ coef_out) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const NoiseClip c = noise_clip(offsets, noise_lo, noise_len, noise_start, b);
    if (blockIdx.x == 0 && tid == 0 && coef_out && c.n <= 0) coef_out[b] = 0.f;    // an empty clip still gets its coefficient
    if ((int64_t)blockIdx.x >= c.nchunks) return;
    float coef = 0.f;
    if (c.nlen > 0) {
        const int64_t np = min(c.nchunks, (int64_t)gridDim.x);
        const double* slot = ws + (int64_t)b * gridDim.x * 2;
        double ex = 0.0, en = 0.0;
        for (int64_t k = 0; k < np; ++k) {
            ex += slot[2 * k];
            en += slot[2 * k + 1];
        }
        if (en > 0.0) {
            const double n = (double)c.n;
            const float f = (float)((double)level[b] * sqrt(ex / n) / sqrt(en / n));
            coef = isfinite(f) ? f : 0.f;
        }
    }
    if (blockIdx.x == 0 && tid == 0 && coef_out) coef_out[b] = coef;
    const float* x = wav + c.lo;
    float* y = out + c.lo;
    if (coef == 0.f) {
        if (x != y)
            for (int64_t ch = blockIdx.x; ch < c.nchunks; ch += gridDim.x)
                for (int64_t i = ch * NZ_CHUNK + tid, i1 = min((ch + 1) * NZ_CHUNK, c.n); i < i1; i += 256) y[i] = x[i];
        return;
    }
    const int16_t* rec = bank + c.nlo;
    const int64_t step = 256 % c.nlen;
    for (int64_t ch = blockIdx.x; ch < c.nchunks; ch += gridDim.x) {
        const int64_t i0 = ch * NZ_CHUNK + tid, i1 = min((ch + 1) * NZ_CHUNK, c.n);
        int64_t p = i0 < i1 ? noise_pos(c, i0) : 0;
        for (int64_t i = i0; i < i1; i += 256) {
            const float nv = __fmul_rn((float)rec[p], noise_scale);
            y[i] = __fadd_rn(x[i], __fmul_rn(coef, nv));                  // two roundings, no fma: numpy float32 can follow
            p += step;
            if (p >= c.nlen) p -= c.nlen;
        }
    }
}

}  // namespace

extern "C" size_t ds2_noise_mix_ws_bytes(int B, size_t max_clip_len) {
    if (B < 1) B = 1;
    size_t chunks = (max_clip_len + NZ_CHUNK - 1) / NZ_CHUNK;
    if (chunks < 1) chunks = 1;
    if (chunks > (size_t)NZ_MAX_CHUNKS) chunks = (size_t)NZ_MAX_CHUNKS;
    return (size_t)B * chunks * 2 * sizeof(double);
}

extern "C" int ds2_noise_mix(const float* wav, const int64_t* offsets, int B, const int16_t* bank, const int64_t* noise_lo,
                             const int64_t* noise_len, const int64_t* noise_start, const float* level, float noise_scale,
                             float* out, float* coef, void* ws, size_t ws_bytes, void* stream) {
    DS2_CHECK_ARG(wav && offsets && bank && noise_lo && noise_len && noise_start && level && out && ws);
    DS2_CHECK_ARG(B >= 1 && B <= 65535 && noise_scale > 0.f);
    DS2_CHECK_ARG(ws_bytes >= (size_t)B * 2 * sizeof(double));           // at least one partial per clip
    // the workspace fixes the chunk grid: ws_bytes / (16 B) chunks per clip (a longer clip's workgroups take several chunks)
    size_t chunks = ws_bytes / ((size_t)B * 2 * sizeof(double));
    if (chunks > (size_t)NZ_MAX_CHUNKS) chunks = (size_t)NZ_MAX_CHUNKS;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    hipLaunchKernelGGL(noise_energy_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, offsets, bank, noise_lo, noise_len,
                       noise_start, noise_scale, (double*)ws);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(noise_mix_kernel, grid, dim3(256), 0, (hipStream_t)stream, wav, offsets, bank, noise_lo, noise_len,
                       noise_start, level, noise_scale, (const double*)ws, out, coef);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
