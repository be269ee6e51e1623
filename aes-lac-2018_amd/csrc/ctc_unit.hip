// Unit posteriors: how sure is the model of every word (or character) of a decoded label row -- the CTC forward over the
// frames the decoder gave the unit (include/ds2hip.h, "unit posterior", has the definition; tests/conf_ref.py states it in
// Python).  gfx950.
//
// Two launches on the stream:
//   units   one WAVE per row.  A first sweep over the row's labels and offsets, 64 at a time, validates it; a second finds the
//           units from two ballots per 64 labels, "a unit starts here" and "a unit ends here": the lane at a unit's END numbers
//           it (the ends before it), finds its start (the last start at or below it, or the one carried in from earlier
//           labels) and writes unit_first, unit_len and, into the workspace, the unit's first frame and frame count -- (0, 0)
//           for a unit that gets no value, so the second launch looks at nothing else to decide.  The wave then fills the
//           entries past the row's count.
//   values  one WAVE per (row, listed unit).  Lane j carries label state 2 j + 1 and the blank state 2 j + 2 behind it as fp64
//           pairs in registers; lane 0 carries the leading blank, state 0, as well.  So 64 lanes hold the S = 2 L + 1 <= 129
//           states, a state's stay and its s-1 neighbour are the lane's own, and only a label's s-1 / s-2 from the lane below
//           cross lanes: lane j - 1 adds them (blank, plus its label where the two labels differ) and ONE fp64 value moves up a
//           lane per frame (two 32-bit DPP moves, wave_shr:1; no LDS, no barrier).  A frame is two additions and a product
//           for the label, one addition and a product for the blank.  The emissions p[t][label], p[t][blank] do not depend on
//           the recursion: the loads of the NEXT 8 frames are issued before the current 8 are worked on.
//           Every 4 frames the wave asks by ballot whether any state is above 2^200 or none above 2^-200; only then does it
//           take the wave maximum and rescale all states by that power of two (between two looks the largest state moves by
//           at most 2^-596 .. 2^520: fp32 inputs, at most three terms).
// Critical path of `values`: n dependent frames of one wave; all units run side by side.  No workgroup waits on another, no
// atomics, outputs leave through ordinary vector stores.
#include "ds2_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int UNIT_MAX_LABELS = DS2_UNIT_MAX_LABELS;   // one label per lane
static_assert(UNIT_MAX_LABELS == 64, "a lane carries one label of the unit");
constexpr int UNIT_WAVES = 4;                          // rows (units) per workgroup
constexpr int UNIT_NTHR = 64 * UNIT_WAVES;
constexpr int UNIT_CH = 8;                             // frames per load group
constexpr int UNIT_LOOK = 4;                           // frames between two looks at the magnitudes
constexpr int MAX_A = 256;

inline size_t ws_align(size_t n) { return (n + 15) & ~(size_t)15; }

__device__ inline unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// ---- launch 1: validate the row, list its units
__global__ __launch_bounds__(UNIT_NTHR) void unit_find_kernel(
    const int32_t* __restrict__ sizes, int B, int T, int A, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ lens, const int32_t* __restrict__ utt, int R, int stride,
    int space_id, int blank, int max_units, int2* __restrict__ span, int32_t* __restrict__ unit_first,
    int32_t* __restrict__ unit_len, double* __restrict__ unit_logp, int32_t* __restrict__ n_units,
    int32_t* __restrict__ dropped) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * UNIT_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                                     // (wave-uniform; the kernel has no barrier)
    const int len = lens[r];
    const int u = utt ? utt[r] : r;
    bool ok = len >= 0 && len <= stride && u >= 0 && u < B;
    const int lim = ok ? min(max(sizes[u], 0), T) : 0;
    const int32_t* lab = labels + (size_t)r * stride;
    const int32_t* off = offsets + (size_t)r * stride;
    const size_t row = (size_t)r * max_units;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    if (ok) {
        bool bad = false;
        for (int p = lane; p < len; p += 64) {
            const int c = lab[p], o = off[p];
            const int po = p > 0 ? off[p - 1] : -1;
            bad = bad || c < 0 || c >= A || c == blank || o <= po || o >= lim;
        }
        ok = !__any(bad);
    }

    int count = 0, ndrop = 0;
    if (ok) {
        int open_first = -1;                                // the start of a unit that has not ended yet (wave-uniform)
        for (int base = 0; base < len; base += 64) {
            const int p = base + lane;
            const bool in = p < len;
            bool start = in, end = in;                      // characters: every label starts and ends a unit
            if (space_id >= 0) {
                const bool here = in && lab[p] != space_id;
                start = here && (p == 0 || lab[p - 1] == space_id);
                end = here && (p + 1 >= len || lab[p + 1] == space_id);
            }
            const unsigned long long smask = __ballot(start), emask = __ballot(end);
            bool drop = false;
            if (end) {
                const int idx = count + __popcll(emask & lanes_below(lane));
                const unsigned long long sm = smask & (lanes_below(lane) | (1ull << lane));
                const int first = sm ? base + 63 - __clzll((long long)sm) : open_first;
                const int ulen = p - first + 1;
                drop = ulen > UNIT_MAX_LABELS;
                if (idx < max_units) {
                    unit_first[row + idx] = first;
                    unit_len[row + idx] = ulen;
                    int2 sp = make_int2(0, 0);
                    if (drop) {
                        unit_logp[row + idx] = nan;
                    } else {
                        const int f0 = off[first];
                        sp = make_int2(f0, off[p] - f0 + 1);
                    }
                    span[row + idx] = sp;
                }
            }
            ndrop += __popcll(__ballot(drop));
            count += __popcll(emask);
            if (smask) {
                const int hs = 63 - __clzll((long long)smask);
                if (!emask || hs > 63 - __clzll((long long)emask)) open_first = base + hs;
            }
        }
    }
    if (lane == 0) {
        n_units[r] = ok ? count : -1;
        dropped[r] = ndrop;
    }
    for (int k = min(count, max_units) + lane; k < max_units; k += 64) {
        unit_first[row + k] = -1;
        unit_len[row + k] = -1;
        unit_logp[row + k] = nan;
        span[row + k] = make_int2(0, 0);
    }
}

// what the lane below holds (lane 0 reads 0): one step up the wave, in registers
__device__ inline double from_lane_below(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, false);   // wave_shr:1
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ inline double wave_max(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(x, o, 64);
        if (y > x) x = y;
    }
    return x;
}

// ---- launch 2: the forward recursion of one unit per wave
__global__ __launch_bounds__(UNIT_NTHR) void unit_value_kernel(
    const float* __restrict__ probs, int T, int A, const int32_t* __restrict__ labels, const int32_t* __restrict__ utt,
    long units, int stride, int blank, int max_units, const int2* __restrict__ span, const int32_t* __restrict__ unit_first,
    const int32_t* __restrict__ unit_len, double* __restrict__ unit_logp) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * UNIT_WAVES + (threadIdx.x >> 6);
    if (w >= units) return;                                 // (wave-uniform; the kernel has no barrier)
    const int2 sp = span[w];
    const int n = sp.y;
    if (n <= 0) return;                                     // past the count, dropped, or an invalid row: launch 1 wrote it
    const int r = (int)(w / max_units);
    const int u = utt ? utt[r] : r;
    const int first = unit_first[w], L = unit_len[w];
    const bool act = lane < L;
    const int sym = act ? labels[(size_t)r * stride + first + lane] : 0;
    const int sym_next = __shfl_down(sym, 1, 64);
    const bool skip_next = lane + 1 < L && sym_next != sym; // lane + 1's label may be entered from this lane's label
    const float* pu = probs + ((size_t)u * T + sp.x) * A;

    float nl[UNIT_CH], nb[UNIT_CH];                         // the next load group: this lane's label and the blank
    auto load = [&](int t0) {
#pragma unroll
        for (int i = 0; i < UNIT_CH; ++i) {
            const bool in = act && t0 + i < n;              // nothing past the span, nothing for a lane without a label
            nl[i] = in ? pu[(size_t)(t0 + i) * A + sym] : 0.f;
            nb[i] = in ? pu[(size_t)(t0 + i) * A + blank] : 0.f;
        }
    };

    // state before the span's first frame: all mass in the leading blank (a product with 1.0 is exact)
    double a_lab = 0.0, a_blk = 0.0, a_b0 = lane == 0 ? 1.0 : 0.0;
    int e2 = 0;                                             // the power of two taken out so far
    bool dead = false;
    load(0);
    for (int t0 = 0; t0 < n && !dead; t0 += UNIT_CH) {
        float cl[UNIT_CH], cb[UNIT_CH];
#pragma unroll
        for (int i = 0; i < UNIT_CH; ++i) {
            cl[i] = nl[i];
            cb[i] = nb[i];
        }
        if (t0 + UNIT_CH < n) load(t0 + UNIT_CH);           // in flight while this group's frames are worked on
#pragma unroll
        for (int i = 0; i < UNIT_CH; ++i) {
            if (t0 + i < n) {
                const double pl = cl[i] > 0.f ? (double)cl[i] : 0.0;   // NaN and negative count as 0
                const double pb = cb[i] > 0.f ? (double)cb[i] : 0.0;
                double up = a_blk;
                if (skip_next) up = a_blk + a_lab;
                double in = from_lane_below(up);
                if (lane == 0) in = a_b0;
                const double nlab = pl * ((a_lab + in));
                a_blk = pb * (a_blk + a_lab);
                a_b0 = pb * a_b0;
                a_lab = nlab;
            }
            if ((i + 1) % UNIT_LOOK == 0) {
                const double m = fmax(fmax(a_lab, a_blk), a_b0);
                if (__any(m > 0x1p200) || !__any(m > 0x1p-200)) {
                    const double mx = wave_max(m);
                    if (mx == 0.0) {
                        dead = true;                        // every state is 0 and stays 0
                    } else if (mx < INFINITY) {
                        const int e = ilogb(mx);
                        a_lab = ldexp(a_lab, -e);
                        a_blk = ldexp(a_blk, -e);
                        a_b0 = ldexp(a_b0, -e);
                        e2 += e;
                    }
                }
            }
        }
    }
    if (lane == L - 1) unit_logp[w] = log(a_blk + a_lab) + (double)e2 * 0.693147180559945309417232121458;
}

}  // namespace

extern "C" size_t ds2_ctc_unit_posterior_ws_bytes(int R, int stride, int max_units) {
    (void)stride;
    if (R < 1 || max_units < 1) return 0;
    return ws_align((size_t)R * max_units * sizeof(int2)) + 16;
}

extern "C" int ds2_ctc_unit_posterior(const float* probs, const int32_t* sizes, int B, int T, int A, const int32_t* labels,
                                      const int32_t* offsets, const int32_t* lens, const int32_t* utt, int R, int stride,
                                      int space_id, int blank, int max_units, void* ws, size_t ws_bytes, int32_t* unit_first,
                                      int32_t* unit_len, double* unit_logp, int32_t* n_units, int32_t* dropped,
                                      void* stream) {
    if (A < 1 || A > MAX_A) {
        ds2_set_error("ds2_ctc_unit_posterior: alphabet size %d is outside 1..%d", A, MAX_A);
        return DS2_ERR_ARG;
    }
    if (blank < 0 || blank >= A) {
        ds2_set_error("ds2_ctc_unit_posterior: blank %d is outside [0, %d)", blank, A);
        return DS2_ERR_ARG;
    }
    if (space_id < -1 || space_id >= A || space_id == blank) {
        ds2_set_error("ds2_ctc_unit_posterior: space_id %d is outside -1..%d or equals blank %d", space_id, A - 1, blank);
        return DS2_ERR_ARG;
    }
    if (R < 1 || stride < 1 || max_units < 1) {
        ds2_set_error("ds2_ctc_unit_posterior: R %d, stride %d and max_units %d must be >= 1", R, stride, max_units);
        return DS2_ERR_ARG;
    }
    if (B < 1 || T < 1 || (long)B * T > (1l << 25)) {
        ds2_set_error("ds2_ctc_unit_posterior: B %d x T %d is outside 1..2^25 frames", B, T);
        return DS2_ERR_ARG;
    }
    if ((long)R * stride > (1l << 27) || (long)R * max_units > (1l << 27)) {
        ds2_set_error("ds2_ctc_unit_posterior: R %d x stride %d or x max_units %d exceeds 2^27", R, stride, max_units);
        return DS2_ERR_ARG;
    }
    if (!probs || !sizes || !labels || !offsets || !lens || !unit_first || !unit_len || !unit_logp || !n_units || !dropped) {
        ds2_set_error("ds2_ctc_unit_posterior: a NULL pointer (only utt may be NULL)");
        return DS2_ERR_ARG;
    }
    if (ws_bytes < ds2_ctc_unit_posterior_ws_bytes(R, stride, max_units) || !ws) {
        ds2_set_error("ds2_ctc_unit_posterior: workspace of %zu bytes < ds2_ctc_unit_posterior_ws_bytes = %zu", ws_bytes,
                      ds2_ctc_unit_posterior_ws_bytes(R, stride, max_units));
        return DS2_ERR_ARG;
    }
    int2* span = (int2*)(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    hipLaunchKernelGGL(unit_find_kernel, dim3(ds2_cdiv(R, UNIT_WAVES)), dim3(UNIT_NTHR), 0, (hipStream_t)stream, sizes, B, T, A,
                       labels, offsets, lens, utt, R, stride, space_id, blank, max_units, span, unit_first, unit_len,
                       unit_logp, n_units, dropped);
    DS2_CHECK_LAUNCH();
    const long units = (long)R * max_units;
    hipLaunchKernelGGL(unit_value_kernel, dim3(ds2_cdiv(units, UNIT_WAVES)), dim3(UNIT_NTHR), 0, (hipStream_t)stream, probs, T,
                       A, labels, utt, units, stride, blank, max_units, span, unit_first, unit_len, unit_logp);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
