// CTC negative log-likelihood and its gradient w.r.t. un-normalised activations, gfx950.
//
// Three launches:
//   K0  row maximum and log1p(sum of exp of the OTHER entries) of acts (T*B rows, one wave per row).  The two parts of the
//       row's log-sum-exp stay apart so that log p = (a - max) - log1p(..) keeps its RELATIVE accuracy for the symbol a
//       trained model is sure of: max + log(sum) as one float would round a -log p of 4e-7 to 0 or 1.9e-6 at |a| ~ 20.
//   K1  grid (B, 2): block (b,0) runs the alpha recursion forward in time, block (b,1) the beta
//       recursion backward in time, concurrently, in LOG space.  Values are carried in fp64 but the
//       transcendental part of every log-sum-exp runs in fp32: with m = max(a,b,c),
//           lse3 = m + log(exp(a-m) + exp(b-m) + exp(c-m)),  the log term lies in [0, log 3],
//       so its fp32 rounding is ~1e-7 ABSOLUTE whatever |m| is; it is formed as log1p of the two smaller terms, so that it
//       is also accurate RELATIVE to itself when they are tiny (the near-zero cost of a confidently right utterance).  (Plain fp32 log space loses ~1e-3
//       on the posteriors once |alpha| ~ 2000 at T = 746; a rescaled linear-domain recursion
//       underflows fp32 when the posterior mass sits far from the row maximum, e.g. early in training
//       with blank-dominated outputs.)  A row of 2L+1 states lives in LDS (double-buffered, one
//       barrier per frame) and is streamed to HBM for K2.
//   K2  grid (T, B): posterior occupancy per symbol exp(alpha+beta-lp-ll) (LDS float atomics for
//       label states, a wave reduction for the blank states), grad = scale * (softmax - occupancy).
// Only K1 is sequential in T; its critical path is T barriers per utterance.
// The helpers, K0 and one row of K1 live in ctc_common.h: ds2_ctc_mwer_grad (ctc_mwer.hip) runs them over many label rows.
#include "ctc_common.h"

namespace {

// K1: one state per thread, one workgroup per (utterance, direction); the recursion itself is ctc_common.h's.
template <int NTHR>
__global__ __launch_bounds__(NTHR) void ctc_alphabeta_kernel(
    const float* __restrict__ acts, const float* __restrict__ rmx, const float* __restrict__ rl1p,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ label_offsets, const int32_t* __restrict__ label_lens,
    const int32_t* __restrict__ act_lens, int T, int B, int A, int smax, double* __restrict__ alpha,
    double* __restrict__ beta, double* __restrict__ ll_out, float* __restrict__ costs) {
    const int b = blockIdx.x, dirn = blockIdx.y;
    ctc_alphabeta_row<NTHR>(acts, rmx, rl1p, labels + label_offsets[b], label_lens[b], min(act_lens[b], T), b, dirn, T, B, A, smax,
                            (dirn == 0 ? alpha : beta) + (size_t)b * T * smax, ll_out + b, costs + b);
}

__global__ __launch_bounds__(128) void ctc_grad_kernel(const float* __restrict__ acts, const float* __restrict__ rmx,
                                                       const float* __restrict__ rl1p,
                                                       const int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ label_offsets,
                                                       const int32_t* __restrict__ label_lens,
                                                       const int32_t* __restrict__ act_lens, int T, int B, int A,
                                                       int smax, const double* __restrict__ alpha,
                                                       const double* __restrict__ beta,
                                                       const double* __restrict__ ll_in, float grad_scale,
                                                       int zero_batch_if_inf, float* __restrict__ grad) {
    __shared__ float occ[256];
    __shared__ int any_inf;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* grow = grad + ((size_t)t * B + b) * A;
    const int tl = min(act_lens[b], T);
    const double ll = ll_in[b];
    if (zero_batch_if_inf) {   // the training step's rule (codes/engine.py:27-30): an infinite batch loss is replaced by
                               // 0 * loss, so NO utterance of the batch contributes a gradient
        if (tid == 0) any_inf = 0;
        __syncthreads();
        for (int i = tid; i < B; i += 128)
            if (ll_in[i] == NEG_INF_D || ll_in[i] == -NEG_INF_D) any_inf = 1;
        __syncthreads();
    }
    if (t >= tl || ll == NEG_INF_D || (zero_batch_if_inf && any_inf)) {
        for (int k = tid; k < A; k += 128) grow[k] = 0.f;
        return;
    }
    for (int k = tid; k < A; k += 128) occ[k] = 0.f;
    __syncthreads();
    const int L = label_lens[b], S = 2 * L + 1;
    const int32_t* lab = labels + label_offsets[b];
    const float* arow = acts + ((size_t)t * B + b) * A;
    const float m0 = rmx[(size_t)t * B + b], p0 = rl1p[(size_t)t * B + b];
    const double* al = alpha + ((size_t)b * T + t) * smax;
    const double* be = beta + ((size_t)b * T + t) * smax;
    const double base_blank = ll + (double)((arow[0] - m0) - p0);
    float blank_sum = 0.f;
    for (int s = tid; s < S; s += 128) {
        const double ab = al[s] + be[s];
        if (ab == NEG_INF_D) continue;
        if (s & 1) {
            const int k = lab[s >> 1];
            atomicAdd(&occ[k], expf((float)(ab - ll - (double)((arow[k] - m0) - p0))));
        } else {
            blank_sum += expf((float)(ab - base_blank));
        }
    }
    blank_sum = wave_sum(blank_sum);
    if ((tid & 63) == 0) atomicAdd(&occ[0], blank_sum);
    __syncthreads();
    for (int k = tid; k < A; k += 128) grow[k] = grad_scale * (expf((arow[k] - m0) - p0) - occ[k]);
}

}  // namespace

extern "C" size_t ds2_ctc_ws_bytes(int T, int B, int A, int max_label_len) {
    (void)A;
    const size_t smax = 2 * (size_t)max_label_len + 1;
    return sizeof(double) * (2 * (size_t)B * T * smax + (size_t)B) + sizeof(float) * 2 * (size_t)T * B + 64;
}

extern "C" int ds2_ctc_loss_grad(const float* acts, const int32_t* labels, const int32_t* label_offsets,
                                 const int32_t* label_lens, const int32_t* act_lens, int T, int B, int A,
                                 int max_label_len, float grad_scale, int zero_batch_if_inf, float* costs,
                                 float* grad, void* ws, void* stream) {
    DS2_CHECK_ARG(acts && labels && label_offsets && label_lens && act_lens && costs && grad && ws);
    DS2_CHECK_ARG(T > 0 && B > 0 && A > 1 && A <= 256 && max_label_len >= 0);
    const int smax = 2 * max_label_len + 1;
    DS2_CHECK_ARG(smax <= MAX_S);
    DS2_CHECK_ARG(B <= 65535);
    hipStream_t st = (hipStream_t)stream;
    double* alpha = (double*)ws;
    double* beta = alpha + (size_t)B * T * smax;
    double* ll = beta + (size_t)B * T * smax;
    float* rmx = (float*)(ll + B);
    float* rl1p = rmx + (size_t)T * B;
    hipLaunchKernelGGL(ctc_lse_kernel, dim3(ds2_cdiv((long)T * B, 4)), dim3(256), 0, st, acts, T * B, A, rmx, rl1p);
#define DS2_CTC_AB(N_)                                                                                                  \
    hipLaunchKernelGGL(ctc_alphabeta_kernel<N_>, dim3(B, 2), dim3(N_), 0, st, acts, rmx, rl1p, labels, label_offsets,    \
                       label_lens, act_lens, T, B, A, smax, alpha, beta, ll, costs)
    if (smax <= 256) DS2_CTC_AB(256);
    else if (smax <= 512) DS2_CTC_AB(512);
    else DS2_CTC_AB(1024);
#undef DS2_CTC_AB
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(T, B), dim3(128), 0, st, acts, rmx, rl1p, labels, label_offsets, label_lens,
                       act_lens, T, B, A, smax, alpha, beta, ll, grad_scale, zero_batch_if_inf, grad);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
