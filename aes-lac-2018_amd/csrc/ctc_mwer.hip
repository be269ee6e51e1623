// Minimum-word-error-rate loss and gradient from N-best lists (ds2_ctc_mwer_grad; include/ds2hip.h "MWER" has the rules).
//
// Utterance b owns N + 1 label ROWS that share its activations: row n < N is hypothesis n of the device N-best search, row N is
// the reference.  Row r = b (N + 1) + n everywhere below.  Four launches, none replicates acts or the gradient per row:
//   K0  ctc_lse_kernel (ctc_common.h), once per (t, b): every row of an utterance shares the frame's log-sum-exp.
//   K1  grid (B (N + 1), 2): one row's alpha (y = 0) or beta (y = 1) recursion, ctc_common.h's ctc_alphabeta_row -- the code
//       ds2_ctc_loss_grad runs, fp64-carried, emissions staged through LDS, 256 / 512 / 1024 threads by state count.  A row at
//       or past hyp_count[b] is not read and gets log p = -inf; so does a row longer than max_label_len (or hyp_stride).
//   K2  grid (B): the utterance's posteriors over its finite rows, expected risk and the row weights w_n, all in fp64 from the
//       rows' log-likelihoods: w_n = -P_n (W_n - E[W]) for the hypotheses, ctc_weight for the reference, every w = 0 when the
//       reference is infeasible.
//   K3  grid (T, B): loops over the utterance's rows IN ROW ORDER and adds w_n * occupancy_n(t, k) into one LDS accumulator of A
//       entries, then writes grad_scale * ((sum of w) * softmax - accumulator) once.  The accumulator is 64-bit FIXED POINT
//       (2^-44 units, integer LDS atomics): integer addition commutes, so the result does not depend on the order in which the
//       states of a row arrive, and two launches on the same input give the same bits.  |w_n| is at most the spread of the
//       risks (<= 2048 labels), occupancies sum to 1 per row: |accumulator| < 129 * 2^11 * 2^44 < 2^63; a term is rounded by at
//       most 2^-45, 1023 states x 129 rows of them by 2^-28 in all.
// Workspace: alpha and beta (B (N + 1), T, smax) fp64, log p and w (B (N + 1)) fp64, the two log-sum-exp parts (T, B) fp32.
#include "ctc_common.h"

namespace {

constexpr int MWER_MAX_N = 128;              // DS2_MWER_MAX_NBEST: the beam search's largest beam
constexpr double MWER_FIX = 17592186044416.0;   // 2^44

struct MwerRow {
    const int32_t* lab;
    int len;
    bool used, fits;
};

// row n of utterance b: its labels and length; used = it exists (n < hyp_count[b], or the reference), fits = it can be run
__device__ __forceinline__ MwerRow mwer_row(int b, int n, int N, const int32_t* hyp, const int32_t* hyp_len,
                                            const int32_t* hyp_count, int hyp_stride, const int32_t* ref,
                                            const int32_t* ref_offsets, const int32_t* ref_lens, int max_label_len) {
    MwerRow r;
    if (n == N) {
        r.lab = ref + ref_offsets[b];
        r.len = ref_lens[b];
        r.used = true;
        r.fits = r.len >= 0 && r.len <= max_label_len;
    } else {
        r.used = n < hyp_count[b];
        r.len = r.used ? hyp_len[(size_t)b * N + n] : 0;
        r.lab = hyp + ((size_t)b * N + n) * hyp_stride;
        r.fits = r.used && r.len >= 0 && r.len <= max_label_len && r.len <= hyp_stride;
    }
    return r;
}

template <int NTHR>
__global__ __launch_bounds__(NTHR) void mwer_alphabeta_kernel(
    const float* __restrict__ acts, const float* __restrict__ rmx, const float* __restrict__ rl1p,
    const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ hyp_count, int N,
    int hyp_stride, const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_offsets,
    const int32_t* __restrict__ ref_lens, int max_label_len, const int32_t* __restrict__ act_lens, int T, int B, int A, int smax,
    double* __restrict__ alpha, double* __restrict__ beta, double* __restrict__ ll_out, float* __restrict__ ref_costs,
    float* __restrict__ hyp_costs) {
    const int r = blockIdx.x, dirn = blockIdx.y;
    const int b = r / (N + 1), n = r - b * (N + 1);
    const MwerRow row = mwer_row(b, n, N, hyp, hyp_len, hyp_count, hyp_stride, ref, ref_offsets, ref_lens, max_label_len);
    float* cost = n == N ? ref_costs + b : hyp_costs + (size_t)b * N + n;
    if (!row.fits) {                                    // unused, or too long to run: no path, whatever its labels are
        if (dirn == 0 && threadIdx.x == 0) {
            *cost = INFINITY;
            ll_out[r] = NEG_INF_D;
        }
        return;
    }
    ctc_alphabeta_row<NTHR>(acts, rmx, rl1p, row.lab, row.len, min(act_lens[b], T), b, dirn, T, B, A, smax,
                            (dirn == 0 ? alpha : beta) + (size_t)r * T * smax, ll_out + r, cost);
}

__global__ __launch_bounds__(64) void mwer_weights_kernel(
    const double* __restrict__ ll, const float* __restrict__ risk, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ hyp_count, int N, int hyp_stride, int max_label_len, float ctc_weight,
    double* __restrict__ w, float* __restrict__ posterior, float* __restrict__ exp_risk, int32_t* __restrict__ dropped) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* llb = ll + (size_t)b * (N + 1);
    const int count = min(max(hyp_count[b], 0), N);
    // lane owns rows lane and lane + 64 (N <= 128)
    double l[2], rk[2];
    int ndrop = 0;
    double mx = NEG_INF_D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = lane + 64 * i;
        l[i] = NEG_INF_D;
        rk[i] = 0.0;
        if (n < count) {
            const int len = hyp_len[(size_t)b * N + n];
            if (len < 0 || len > max_label_len || len > hyp_stride) ++ndrop;
            l[i] = llb[n];
            if (l[i] != NEG_INF_D) rk[i] = (double)risk[(size_t)b * N + n];     // the risk of a row without a path is not read
            mx = fmax(mx, l[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o, 64));
        ndrop += __shfl_xor(ndrop, o, 64);
    }
    double e[2], z = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        e[i] = l[i] != NEG_INF_D ? exp(l[i] - mx) : 0.0;
        z += e[i];
    }
    z = wave_sum_d(z);
    double ew = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        e[i] = z > 0.0 ? e[i] / z : 0.0;                // P_n; no finite row: all 0, E[W] = 0
        ew += e[i] * rk[i];
    }
    ew = wave_sum_d(ew);
    const bool ref_ok = llb[N] != NEG_INF_D;            // an infeasible reference: the utterance gives no gradient, neither term
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = lane + 64 * i;
        if (n < N) {
            posterior[(size_t)b * N + n] = (float)e[i];
            w[(size_t)b * (N + 1) + n] = (ref_ok && e[i] > 0.0) ? -e[i] * (rk[i] - ew) : 0.0;
        }
    }
    if (lane == 0) {
        w[(size_t)b * (N + 1) + N] = ref_ok ? (double)ctc_weight : 0.0;
        exp_risk[b] = (float)ew;
        dropped[b] = ndrop;
    }
}

__global__ __launch_bounds__(128) void mwer_grad_kernel(
    const float* __restrict__ acts, const float* __restrict__ rmx, const float* __restrict__ rl1p,
    const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ hyp_count, int N,
    int hyp_stride, const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_offsets,
    const int32_t* __restrict__ ref_lens, int max_label_len, const int32_t* __restrict__ act_lens, int T, int B, int A, int smax,
    const double* __restrict__ alpha, const double* __restrict__ beta, const double* __restrict__ ll_in,
    const double* __restrict__ w_in, float grad_scale, int zero_batch_if_inf, float* __restrict__ grad) {
    __shared__ unsigned long long acc[256];             // two's-complement fixed point, 2^-44 units
    __shared__ int any_inf;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* grow = grad + ((size_t)t * B + b) * A;
    const int tl = min(act_lens[b], T);
    if (zero_batch_if_inf) {                            // the training step's rule, on the REFERENCES' costs (as ctc_grad_kernel)
        if (tid == 0) any_inf = 0;
        __syncthreads();
        for (int i = tid; i < B; i += 128)
            if (ll_in[(size_t)i * (N + 1) + N] == NEG_INF_D) any_inf = 1;
        __syncthreads();
    }
    if (t >= tl || (zero_batch_if_inf && any_inf)) {
        for (int k = tid; k < A; k += 128) grow[k] = 0.f;
        return;
    }
    for (int k = tid; k < A; k += 128) acc[k] = 0ull;
    __syncthreads();
    const float* arow = acts + ((size_t)t * B + b) * A;
    const float m0 = rmx[(size_t)t * B + b], p0 = rl1p[(size_t)t * B + b];
    const double lp_blank = (double)((arow[0] - m0) - p0);
    double wsum = 0.0;
    for (int n = 0; n <= N; ++n) {
        const size_t r = (size_t)b * (N + 1) + n;
        const double wn = w_in[r], ll = ll_in[r];
        if (wn == 0.0 || ll == NEG_INF_D) continue;     // (uniform over the workgroup) rows without weight or path: not read
        wsum += wn;
        const MwerRow row = mwer_row(b, n, N, hyp, hyp_len, hyp_count, hyp_stride, ref, ref_offsets, ref_lens, max_label_len);
        const int S = 2 * row.len + 1;
        const double* al = alpha + (r * T + t) * smax;
        const double* be = beta + (r * T + t) * smax;
        const double base_blank = ll + lp_blank;
        double blank_sum = 0.0;
        for (int s = tid; s < S; s += 128) {
            const double ab = al[s] + be[s];
            if (ab == NEG_INF_D) continue;
            if (s & 1) {
                const int k = row.lab[s >> 1];
                const double o = wn * (double)expf((float)(ab - ll - (double)((arow[k] - m0) - p0)));
                atomicAdd(&acc[k], (unsigned long long)__double2ll_rn(o * MWER_FIX));
            } else {
                blank_sum += (double)expf((float)(ab - base_blank));
            }
        }
        blank_sum = wave_sum_d(blank_sum);
        if ((tid & 63) == 0) atomicAdd(&acc[0], (unsigned long long)__double2ll_rn(wn * blank_sum * MWER_FIX));
    }
    __syncthreads();
    for (int k = tid; k < A; k += 128) {
        const double occ = (double)(long long)acc[k] * (1.0 / MWER_FIX);
        grow[k] = grad_scale * (float)(wsum * (double)expf((arow[k] - m0) - p0) - occ);
    }
}

}  // namespace

extern "C" size_t ds2_ctc_mwer_ws_bytes(int T, int B, int A, int N, int max_label_len) {
    (void)A;
    if (T <= 0 || B <= 0 || N <= 0 || max_label_len < 0) return 0;
    const size_t smax = 2 * (size_t)max_label_len + 1, rows = (size_t)B * ((size_t)N + 1);
    return sizeof(double) * (2 * rows * T * smax + 2 * rows) + sizeof(float) * 2 * (size_t)T * B + 64;
}

extern "C" int ds2_ctc_mwer_grad(const float* acts, const int32_t* act_lens, int T, int B, int A, const int32_t* hyp,
                                 const int32_t* hyp_len, const int32_t* hyp_count, int N, int hyp_stride, const float* risk,
                                 const int32_t* ref, const int32_t* ref_offsets, const int32_t* ref_lens, int max_label_len,
                                 float ctc_weight, float grad_scale, int zero_batch_if_inf, float* ref_costs, float* hyp_costs,
                                 float* posterior, float* exp_risk, int32_t* dropped, float* grad, void* ws, void* stream) {
    DS2_CHECK_ARG(acts && act_lens && hyp && hyp_len && hyp_count && risk && ref && ref_offsets && ref_lens);
    DS2_CHECK_ARG(ref_costs && hyp_costs && posterior && exp_risk && dropped && grad && ws);
    DS2_CHECK_ARG(T > 0 && B > 0 && A > 1 && A <= 256 && max_label_len >= 0);
    DS2_CHECK_ARG(N >= 1 && N <= MWER_MAX_N && hyp_stride >= 0);
    const int smax = 2 * max_label_len + 1;
    DS2_CHECK_ARG(smax <= MAX_S);
    DS2_CHECK_ARG(B <= 65535);
    DS2_CHECK_ARG(ctc_weight >= 0.f && ctc_weight < INFINITY && grad_scale == grad_scale);
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)B * (N + 1);
    double* alpha = (double*)ws;
    double* beta = alpha + rows * T * smax;
    double* ll = beta + rows * T * smax;
    double* w = ll + rows;
    float* rmx = (float*)(w + rows);
    float* rl1p = rmx + (size_t)T * B;
    hipLaunchKernelGGL(ctc_lse_kernel, dim3(ds2_cdiv((long)T * B, 4)), dim3(256), 0, st, acts, T * B, A, rmx, rl1p);
#define DS2_MWER_AB(N_)                                                                                                  \
    hipLaunchKernelGGL(mwer_alphabeta_kernel<N_>, dim3((unsigned)rows, 2), dim3(N_), 0, st, acts, rmx, rl1p, hyp, hyp_len,  \
                       hyp_count, N, hyp_stride, ref, ref_offsets, ref_lens, max_label_len, act_lens, T, B, A, smax, alpha, \
                       beta, ll, ref_costs, hyp_costs)
    if (smax <= 256) DS2_MWER_AB(256);
    else if (smax <= 512) DS2_MWER_AB(512);
    else DS2_MWER_AB(1024);
#undef DS2_MWER_AB
    hipLaunchKernelGGL(mwer_weights_kernel, dim3(B), dim3(64), 0, st, ll, risk, hyp_len, hyp_count, N, hyp_stride,
                       max_label_len, ctc_weight, w, posterior, exp_risk, dropped);
    hipLaunchKernelGGL(mwer_grad_kernel, dim3(T, B), dim3(128), 0, st, acts, rmx, rl1p, hyp, hyp_len, hyp_count, N, hyp_stride,
                       ref, ref_offsets, ref_lens, max_label_len, act_lens, T, B, A, smax, alpha, beta, ll, w, grad_scale,
                       zero_batch_if_inf, grad);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
