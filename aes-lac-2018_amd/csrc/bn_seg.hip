// Segmented sequence BatchNorm: the G per-task heads of the multi-task model (codes/model.py: MultiTaskModel) in one launch per
// stage.  x = xa + xb is the top GRU layer's output, (T,B,F) with the two directions summed in the read; task g owns the batch
// columns [b0[g], b0[g+1]), so its T*B_g rows are strided in x (row t*B + b).  Per task the arithmetic is that of bn.hip's
// sequence flavour over the task's rows alone -- what the reference's per-head BatchNorm1d sees after x[:, b0:b1] -- with fp32
// partials combined in fp64.  The normalised rows are written PACKED, task after task, as contiguous (T, B_g, F) blocks (each
// head's FC is then one plain GEMM), and the backward reads the packed gradient and writes the interleaved (T,B,F) one.
#include <limits.h>

#include "ds2_common.h"

namespace {

constexpr int NPART = 64;       // partials per (task, feature): the same split as bn.hip
constexpr int SEG_MAX = 8;

struct SegArgs {
    int G;
    int b0[SEG_MAX + 1];        // task g owns batch columns [b0[g], b0[g + 1]); b0[0] = 0, b0[G] = B
    const float* gamma[SEG_MAX];
    const float* beta[SEG_MAX];
    float* p0[SEG_MAX];         // stats: running_mean; bwd: dgamma
    float* p1[SEG_MAX];         // stats: running_var;  bwd: dbeta
};

template <int V> struct SegVec;
template <> struct SegVec<1> { typedef float T; };
template <> struct SegVec<4> { typedef f32x4 T; };

template <typename VT>
__device__ __forceinline__ VT ldv(const float* p) { return *reinterpret_cast<const VT*>(p); }
__device__ __forceinline__ float lane_of(float v, int) { return v; }
__device__ __forceinline__ float lane_of(f32x4 v, int e) { return v[e]; }

// task of packed row R (rows of task g start at T*b0[g]) / of batch column b
__device__ __forceinline__ int seg_of_packed_row(const SegArgs& sa, int T, size_t R) {
    int g = 0;
    for (int k = 1; k < sa.G; ++k)
        if ((size_t)T * sa.b0[k] <= R) g = k;
    return g;
}
__device__ __forceinline__ int seg_of_column(const SegArgs& sa, int b) {
    int g = 0;
    for (int k = 1; k < sa.G; ++k)
        if (sa.b0[k] <= b) g = k;
    return g;
}

// grid (NPART, ceil(F/V/64), G); block = 64 column groups x 4 row lanes.  MODE 0: sum x, sum x^2 over the task's rows.
// MODE 1 (backward): sum g, sum g*xhat with g read from the task's packed block.
template <int MODE, int V>
__global__ __launch_bounds__(256) void bn1d_seg_reduce_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                              const float* __restrict__ dyp,
                                                              const float* __restrict__ mean_invstd, SegArgs sa, int T,
                                                              int B, int F, double* __restrict__ part) {
    typedef typename SegVec<V>::T vt;
    const int g = blockIdx.z, p = blockIdx.x, tid = threadIdx.x;
    const int FV = F / V;
    const int cq = blockIdx.y * 64 + (tid & 63), ry = tid >> 6;
    const int b0 = sa.b0[g], bg = sa.b0[g + 1] - b0;
    const int rows = T * bg;
    vt s0{}, s1{};
    if (cq < FV) {
        const int c = V * cq;
        vt mu{}, is{};
        if (MODE == 1) {
            mu = ldv<vt>(mean_invstd + (size_t)g * 2 * F + c);
            is = ldv<vt>(mean_invstd + (size_t)g * 2 * F + F + c);
        }
        const float* dyg = MODE == 1 ? dyp + (size_t)T * b0 * F : nullptr;
        for (int r = p * 4 + ry; r < rows; r += NPART * 4) {
            const int t = r / bg;
            const size_t o = ((size_t)t * B + b0 + (r - t * bg)) * F + c;
            vt v = ldv<vt>(xa + o);
            if (xb) v += ldv<vt>(xb + o);
            if (MODE == 0) {
                s0 += v;
                s1 += v * v;
            } else {
                const vt gr = ldv<vt>(dyg + (size_t)r * F + c);
                s0 += gr;
                s1 += gr * (v - mu) * is;
            }
        }
    }
    __shared__ vt sm[4][64][2];
    sm[ry][tid & 63][0] = s0;
    sm[ry][tid & 63][1] = s1;
    __syncthreads();
    if (ry == 0 && cq < FV) {
        const int l = tid & 63;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double d0 = 0.0, d1 = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d0 += (double)lane_of(sm[k][l][0], e);
                d1 += (double)lane_of(sm[k][l][1], e);
            }
            const size_t q = (((size_t)g * F + V * cq + e) * NPART + p) * 2;
            part[q + 0] = d0;
            part[q + 1] = d1;
        }
    }
}

// grid (F, G), one wave per (feature, task): combine the NPART fp64 partials; running buffers as torch's BatchNorm1d
__global__ __launch_bounds__(64) void bn1d_seg_finalize_stats_kernel(const double* __restrict__ part, SegArgs sa, int T,
                                                                     int F, float eps, float momentum, int use_running,
                                                                     float* __restrict__ mean_invstd) {
    const int c = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    float* mi = mean_invstd + (size_t)g * 2 * F;
    float* rm = sa.p0[g];
    float* rv = sa.p1[g];
    if (use_running) {
        if (lane == 0) {
            mi[c] = rm[c];
            mi[F + c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
        }
        return;
    }
    const double count = (double)T * (sa.b0[g + 1] - sa.b0[g]);
    const size_t q = (((size_t)g * F + c) * NPART + lane) * 2;
    const double s0 = wave_sum_d(part[q + 0]);
    const double s1 = wave_sum_d(part[q + 1]);
    if (lane == 0) {
        const double mean = s0 / count;
        double var = s1 / count - mean * mean;
        if (var < 0.0) var = 0.0;
        mi[c] = (float)mean;
        mi[F + c] = (float)(1.0 / sqrt(var + (double)eps));
        if (rm) {
            const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            rm[c] = (float)((1.0 - momentum) * rm[c] + momentum * mean);
            rv[c] = (float)((1.0 - momentum) * rv[c] + momentum * unb);
        }
    }
}

// grid (F, G): dgamma = sum g*xhat, dbeta = sum g; coef (G,2,F) = the two means the input gradient needs
__global__ __launch_bounds__(64) void bn1d_seg_finalize_bwd_kernel(const double* __restrict__ part, SegArgs sa, int T,
                                                                   int F, float* __restrict__ coef) {
    const int c = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    const double count = (double)T * (sa.b0[g + 1] - sa.b0[g]);
    const size_t q = (((size_t)g * F + c) * NPART + lane) * 2;
    const double s0 = wave_sum_d(part[q + 0]);
    const double s1 = wave_sum_d(part[q + 1]);
    if (lane == 0) {
        sa.p1[g][c] = (float)s0;
        sa.p0[g][c] = (float)s1;
        coef[(size_t)g * 2 * F + c] = (float)(s0 / count);
        coef[(size_t)g * 2 * F + F + c] = (float)(s1 / count);
    }
}

// y packed: element (R, c) of the packed (T*B, F) output, R in task g's block -> row t*B + b of x
template <int V>
__global__ __launch_bounds__(256) void bn1d_seg_apply_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                             const float* __restrict__ mean_invstd, SegArgs sa, int T,
                                                             int B, int F, size_t nv, float* __restrict__ y) {
    typedef typename SegVec<V>::T vt;
    const int FV = F / V;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
        const size_t R = i / FV;
        const int c = V * (int)(i - R * FV);
        const int g = seg_of_packed_row(sa, T, R);
        const int b0 = sa.b0[g], bg = sa.b0[g + 1] - b0;
        const int r = (int)(R - (size_t)T * b0);
        const int t = r / bg;
        const size_t o = ((size_t)t * B + b0 + (r - t * bg)) * F + c;
        vt v = ldv<vt>(xa + o);
        if (xb) v += ldv<vt>(xb + o);
        const float* mi = mean_invstd + (size_t)g * 2 * F;
        const vt sc = ldv<vt>(sa.gamma[g] + c) * ldv<vt>(mi + F + c);
        *reinterpret_cast<vt*>(y + R * F + c) = (v - ldv<vt>(mi + c)) * sc + ldv<vt>(sa.beta[g] + c);
    }
}

// dx interleaved: element (S, c) of the (T*B, F) gradient, S = t*B + b, reads the packed dxf row of (t, b)
template <int V>
__global__ __launch_bounds__(256) void bn1d_seg_bwd_apply_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                                 const float* __restrict__ dxf,
                                                                 const float* __restrict__ mean_invstd,
                                                                 const float* __restrict__ coef, SegArgs sa, int T,
                                                                 int B, int F, size_t nv, float* __restrict__ dx) {
    typedef typename SegVec<V>::T vt;
    const int FV = F / V;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
        const size_t S = i / FV;
        const int c = V * (int)(i - S * FV);
        const int t = (int)(S / B), b = (int)(S - (size_t)t * B);
        const int g = seg_of_column(sa, b);
        const int b0 = sa.b0[g], bg = sa.b0[g + 1] - b0;
        const size_t P = (size_t)T * b0 + (size_t)t * bg + (b - b0);
        const size_t o = S * F + c;
        vt v = ldv<vt>(xa + o);
        if (xb) v += ldv<vt>(xb + o);
        const float* mi = mean_invstd + (size_t)g * 2 * F;
        const float* cf = coef + (size_t)g * 2 * F;
        const vt is = ldv<vt>(mi + F + c);
        const vt xh = (v - ldv<vt>(mi + c)) * is;
        *reinterpret_cast<vt*>(dx + o) =
            ldv<vt>(sa.gamma[g] + c) * is * (ldv<vt>(dxf + P * F + c) - ldv<vt>(cf + c) - xh * ldv<vt>(cf + F + c));
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int seg_ew_blocks(size_t n) {
    size_t b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

// the kernels index a task's rows (rows = T * B_g, r = R - T * b0) in int
inline bool seg_rows_fit(int T, int B) { return (long long)T * B <= INT_MAX; }

// bounds_host: G + 1 column offsets, 0 = b0[0] < b0[1] < ... < b0[G] = B
bool seg_args(int G, const int* bounds_host, int B, SegArgs* sa) {
    if (G < 1 || G > SEG_MAX || !bounds_host || bounds_host[0] != 0 || bounds_host[G] != B) return false;
    *sa = SegArgs{};
    sa->G = G;
    for (int g = 0; g <= G; ++g) {
        if (g > 0 && bounds_host[g] <= bounds_host[g - 1]) return false;
        sa->b0[g] = bounds_host[g];
    }
    return true;
}

}  // namespace

extern "C" int ds2_bn1d_seg_stats(const float* xa, const float* xb, int T, int B, int F, int G, const int* bounds_host,
                                  float eps, float momentum, int use_running, float* const* running_mean_host,
                                  float* const* running_var_host, float* mean_invstd, void* ws, void* stream) {
    DS2_CHECK_ARG(xa && mean_invstd && ws && T > 0 && B > 0 && F > 0);
    DS2_CHECK_ARG(seg_rows_fit(T, B));
    SegArgs sa;
    DS2_CHECK_ARG(seg_args(G, bounds_host, B, &sa));
    DS2_CHECK_ARG(!use_running || (running_mean_host && running_var_host));
    for (int g = 0; g < G; ++g) {
        sa.p0[g] = running_mean_host ? running_mean_host[g] : nullptr;
        sa.p1[g] = running_var_host ? running_var_host[g] : nullptr;
        DS2_CHECK_ARG(!use_running || (sa.p0[g] && sa.p1[g]));
        DS2_CHECK_ARG((sa.p0[g] == nullptr) == (sa.p1[g] == nullptr));
    }
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    if (!use_running) {
        if ((F & 3) == 0 && al16(xa) && al16(xb))
            hipLaunchKernelGGL((bn1d_seg_reduce_kernel<0, 4>), dim3(NPART, ds2_cdiv(F / 4, 64), G), dim3(256), 0, st, xa,
                               xb, nullptr, nullptr, sa, T, B, F, part);
        else
            hipLaunchKernelGGL((bn1d_seg_reduce_kernel<0, 1>), dim3(NPART, ds2_cdiv(F, 64), G), dim3(256), 0, st, xa, xb,
                               nullptr, nullptr, sa, T, B, F, part);
    }
    hipLaunchKernelGGL(bn1d_seg_finalize_stats_kernel, dim3(F, G), dim3(64), 0, st, part, sa, T, F, eps, momentum,
                       use_running, mean_invstd);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}

extern "C" int ds2_bn1d_seg_apply(const float* xa, const float* xb, const float* mean_invstd, int T, int B, int F, int G,
                                  const int* bounds_host, const float* const* gamma_host, const float* const* beta_host,
                                  float* y, void* stream) {
    DS2_CHECK_ARG(xa && mean_invstd && gamma_host && beta_host && y && T > 0 && B > 0 && F > 0);
    DS2_CHECK_ARG(seg_rows_fit(T, B));
    SegArgs sa;
    DS2_CHECK_ARG(seg_args(G, bounds_host, B, &sa));
    bool vec = (F & 3) == 0 && al16(xa) && al16(xb) && al16(y) && al16(mean_invstd);
    for (int g = 0; g < G; ++g) {
        sa.gamma[g] = gamma_host[g];
        sa.beta[g] = beta_host[g];
        DS2_CHECK_ARG(sa.gamma[g] && sa.beta[g]);
        vec = vec && al16(sa.gamma[g]) && al16(sa.beta[g]);
    }
    const size_t n = (size_t)T * B * F;
    if (vec)
        hipLaunchKernelGGL(bn1d_seg_apply_kernel<4>, dim3(seg_ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, xa,
                           xb, mean_invstd, sa, T, B, F, n / 4, y);
    else
        hipLaunchKernelGGL(bn1d_seg_apply_kernel<1>, dim3(seg_ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, xa, xb,
                           mean_invstd, sa, T, B, F, n, y);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}

extern "C" int ds2_bn1d_seg_bwd(const float* xa, const float* xb, const float* dxf, const float* mean_invstd, int T, int B,
                                int F, int G, const int* bounds_host, const float* const* gamma_host, float* dy,
                                float* const* dgamma_host, float* const* dbeta_host, void* ws, void* stream) {
    DS2_CHECK_ARG(xa && dxf && mean_invstd && gamma_host && dy && dgamma_host && dbeta_host && ws);
    DS2_CHECK_ARG(T > 0 && B > 0 && F > 0);
    DS2_CHECK_ARG(seg_rows_fit(T, B));
    SegArgs sa;
    DS2_CHECK_ARG(seg_args(G, bounds_host, B, &sa));
    bool vec = (F & 3) == 0 && al16(xa) && al16(xb) && al16(dxf) && al16(dy) && al16(mean_invstd);
    for (int g = 0; g < G; ++g) {
        sa.gamma[g] = gamma_host[g];
        sa.p0[g] = dgamma_host[g];
        sa.p1[g] = dbeta_host[g];
        DS2_CHECK_ARG(sa.gamma[g] && sa.p0[g] && sa.p1[g]);
        vec = vec && al16(sa.gamma[g]);
    }
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    float* coef = (float*)(part + (size_t)G * F * NPART * 2);
    if (vec)
        hipLaunchKernelGGL((bn1d_seg_reduce_kernel<1, 4>), dim3(NPART, ds2_cdiv(F / 4, 64), G), dim3(256), 0, st, xa, xb,
                           dxf, mean_invstd, sa, T, B, F, part);
    else
        hipLaunchKernelGGL((bn1d_seg_reduce_kernel<1, 1>), dim3(NPART, ds2_cdiv(F, 64), G), dim3(256), 0, st, xa, xb, dxf,
                           mean_invstd, sa, T, B, F, part);
    hipLaunchKernelGGL(bn1d_seg_finalize_bwd_kernel, dim3(F, G), dim3(64), 0, st, part, sa, T, F, coef);
    const size_t n = (size_t)T * B * F;
    if (vec)
        hipLaunchKernelGGL(bn1d_seg_bwd_apply_kernel<4>, dim3(seg_ew_blocks(n / 4)), dim3(256), 0, st, xa, xb, dxf,
                           mean_invstd, coef, sa, T, B, F, n / 4, dy);
    else
        hipLaunchKernelGGL(bn1d_seg_bwd_apply_kernel<1>, dim3(seg_ew_blocks(n)), dim3(256), 0, st, xa, xb, dxf,
                           mean_invstd, coef, sa, T, B, F, n, dy);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
