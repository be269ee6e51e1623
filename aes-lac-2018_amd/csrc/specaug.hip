// SpecAugment on the device (gfx950): time warp, frequency masks and time masks on the (B, t_max, 161) log-spectrogram that
// ds2_spectrogram_fwd writes, one launch for a whole minibatch.  The reference has no such stage: the rules are decisions,
// written down in include/ds2hip.h ("SpecAugment").
//
// Bandwidth bound: with a warp every output cell is one store and (unless masked) one or two loads; without one, in place,
// only the masked cells are stored and nothing is loaded.  Workgroup (x, b) owns SA_ROWS consecutive frames of clip b, which
// are one contiguous run of SA_ROWS * 644 bytes of out: the lanes walk it cell by cell, so every wave store is 256 contiguous
// bytes although a row start is only 4-byte aligned.  What is the same for a whole frame (source frames i0 / i1, the weight,
// "under a time mask") is worked out once per frame by SA_ROWS lanes, what is the same for a whole bin ("under a frequency
// mask") once per bin by 161 lanes, both into LDS; the cell loop then divides by the constant 161 only.
// No atomics, no workspace, no cell written twice: a clip's bits depend on the clip and its tables alone.
#include "ds2_common.h"

namespace {

constexpr int NB = 161;
constexpr int SA_ROWS = 16;                            // frames per workgroup: 2576 cells, ten per lane
constexpr int SA_MAX_MASKS = 8;

struct SpecRows {
    int i0[SA_ROWS], i1[SA_ROWS];                      // source frames of output frame row0 + r
    float frac[SA_ROWS];                               // weight of i1 (0: the frame is a copy of i0)
    unsigned char tmasked[SA_ROWS];                    // the frame lies under a time mask
    unsigned char fmasked[NB];                         // the bin lies under a frequency mask
};

// Fills `s` for workgroup (blockIdx.x, b); returns the clip's valid frames clamped into [0, t_max] and, in *any_mask, whether
// any cell of the workgroup's frames may be masked.  Table entries are device data: every one is clamped, sums in 64 bit.
__device__ inline int spec_rows(SpecRows& s, int t_max, const int32_t* __restrict__ frames, const int32_t* __restrict__ warp,
                                const int32_t* __restrict__ fmask, int MF, const int32_t* __restrict__ tmask, int MT,
                                int* any_mask) {
    const int b = blockIdx.y, tid = threadIdx.x, row0 = blockIdx.x * SA_ROWS;
    const int T = min(max(frames[b], 0), t_max);
    int flag = 0;
    if (tid < NB) {
        for (int m = 0; m < MF; ++m) {
            const int64_t f0 = fmask[((int64_t)b * MF + m) * 2], f = fmask[((int64_t)b * MF + m) * 2 + 1];
            const int64_t lo = max(f0, (int64_t)0), hi = min(f0 + max(f, (int64_t)0), (int64_t)NB);
            flag |= (tid >= lo && tid < hi);
        }
        s.fmasked[tid] = (unsigned char)flag;
    } else if (tid >= 192 && tid < 192 + SA_ROWS) {    // (the fourth wave: the first three are busy with the bins)
        const int r = tid - 192, t = row0 + r;
        int i0 = t, i1 = t;
        float frac = 0.f;
        if (t < T) {
            for (int m = 0; m < MT; ++m) {
                const int64_t t0 = tmask[((int64_t)b * MT + m) * 2], w = tmask[((int64_t)b * MT + m) * 2 + 1];
                const int64_t lo = max(t0, (int64_t)0), hi = min(t0 + max(w, (int64_t)0), (int64_t)T);
                flag |= (t >= lo && t < hi);
            }
            if (warp) {
                const int64_t c = min(max(warp[2 * b], 0), T - 1), c2 = min(max(warp[2 * b + 1], 0), T - 1);
                int64_t num, den, base;
                if (t < c2) {
                    num = (int64_t)t * c, den = c2, base = 0;
                } else {
                    num = (int64_t)(t - c2) * (T - c), den = T - c2, base = c;
                }
                i0 = (int)min(base + num / den, (int64_t)T - 1);
                i1 = min(i0 + 1, T - 1);
                frac = __fdiv_rn((float)(num % den), (float)den);          // both below 2^24 (T <= 4096): one rounding
            }
        }
        s.i0[r] = i0, s.i1[r] = i1, s.frac[r] = frac;
        s.tmasked[r] = (unsigned char)flag;
    }
    *any_mask = __syncthreads_or(flag);
    return T;
}

// Every cell of out is written: warped, masked or zero (padding).  x is never written: __restrict__ holds (the host refuses
// an overlap).
__global__ __launch_bounds__(256) void spec_augment_kernel(const float* __restrict__ x, float* __restrict__ out, int t_max,
                                                           const int32_t* __restrict__ frames,
                                                           const int32_t* __restrict__ warp,
                                                           const int32_t* __restrict__ fmask, int MF,
                                                           const int32_t* __restrict__ tmask, int MT, float mask_value) {
    __shared__ SpecRows s;
    int any;
    const int T = spec_rows(s, t_max, frames, warp, fmask, MF, tmask, MT, &any);
    const int row0 = blockIdx.x * SA_ROWS, ncell = min(SA_ROWS, t_max - row0) * NB;
    const float* xc = x + (size_t)blockIdx.y * t_max * NB;
    float* oc = out + ((size_t)blockIdx.y * t_max + row0) * NB;
    for (int i = threadIdx.x; i < ncell; i += 256) {
        const int r = i / NB, k = i - r * NB;
        float y = 0.f;                                                     // collate padding
        if (row0 + r < T) {
            if (s.tmasked[r] | s.fmasked[k]) {
                y = mask_value;                                            // stored, whatever lies beneath
            } else {
                const float frac = s.frac[r];
                y = xc[(size_t)s.i0[r] * NB + k];
                if (frac != 0.f) y = fmaf(frac, __fsub_rn(xc[(size_t)s.i1[r] * NB + k], y), y);
            }
        }
        oc[i] = y;
    }
}

// No warp, in place: only the masked cells are stored, nothing is loaded.
__global__ __launch_bounds__(256) void spec_mask_inplace_kernel(float* __restrict__ out, int t_max,
                                                                const int32_t* __restrict__ frames,
                                                                const int32_t* __restrict__ fmask, int MF,
                                                                const int32_t* __restrict__ tmask, int MT,
                                                                float mask_value) {
    __shared__ SpecRows s;
    int any;
    const int T = spec_rows(s, t_max, frames, nullptr, fmask, MF, tmask, MT, &any);
    const int row0 = blockIdx.x * SA_ROWS;
    if (!any || row0 >= T) return;
    const int ncell = min(SA_ROWS, T - row0) * NB;                         // (nothing past the clip's frames)
    float* oc = out + ((size_t)blockIdx.y * t_max + row0) * NB;
    for (int i = threadIdx.x; i < ncell; i += 256) {
        const int r = i / NB, k = i - r * NB;
        if (s.tmasked[r] | s.fmasked[k]) oc[i] = mask_value;
    }
}

}  // namespace

extern "C" int ds2_spec_augment(const float* x, float* out, int B, int t_max, const int32_t* frames, const int32_t* warp,
                                const int32_t* fmask, int MF, const int32_t* tmask, int MT, float mask_value, void* stream) {
    DS2_CHECK_ARG(x && out && frames);
    DS2_CHECK_ARG(B >= 1 && B <= 65535 && t_max >= 1);
    DS2_CHECK_ARG(MF >= 0 && MF <= SA_MAX_MASKS && MT >= 0 && MT <= SA_MAX_MASKS);
    DS2_CHECK_ARG((fmask || MF == 0) && (tmask || MT == 0));
    if (!fmask) MF = 0;
    if (!tmask) MT = 0;
    const size_t bytes = (size_t)B * (size_t)t_max * NB * sizeof(float);
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    const dim3 grid((unsigned)ds2_cdiv(t_max, SA_ROWS), (unsigned)B);
    if (!warp && out == x) {
        if (MF == 0 && MT == 0) return DS2_OK;                             // nothing to do
        hipLaunchKernelGGL(spec_mask_inplace_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, t_max, frames, fmask, MF,
                           tmask, MT, mask_value);
    } else {
        // a warp reads frames other than the one it writes; a plain copy with masks refuses a partial overlap as well
        DS2_CHECK_ARG(xa + bytes <= oa || oa + bytes <= xa);
        hipLaunchKernelGGL(spec_augment_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, out, t_max, frames, warp, fmask,
                           MF, tmask, MT, mask_value);
    }
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
