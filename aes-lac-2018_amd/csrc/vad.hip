// Speech / non-speech segmentation of a recording of any length on the device (gfx950): ds2_vad_segment.  Not in the
// reference, which cuts its corpora with dataset scripts and sox; the rule (steps 1-8) is written down in include/ds2hip.h and
// uses integers only, so tests/vad_ref.py can hold it to exact equality.
//
// Three launches on the caller's stream, the launch boundary being the only synchronisation between workgroups:
//   vad_energy_kernel  E[j], the one pass over the samples (2 B each): a workgroup takes 64 blocks (20 KB), every lane loads
//                      aligned 16-byte chunks, the chunk sums go through LDS to the 4 lanes that add up one block
//   vad_level_kernel   S[j], bin(S[j]) and the histogram: per workgroup in LDS, merged with integer atomics
//   vad_runs_kernel    steps 3-8 in ONE workgroup of 1024 threads: threshold; raw runs, merged runs (gaps closed) and the output
//                      rows each as a count + block scan + write over contiguous per-thread ranges (the level bytes 16 per
//                      load: one dependent byte load per block was 0.3 ms of latency for an hour); a run longer than
//                      max_len is split by one wave (the argmin of a cut over its lanes), once to count its pieces and once
//                      to write them
#include "ds2_common.h"

namespace {

constexpr int VB = DS2_VAD_BLOCK;                      // samples per block
constexpr int VBINS = DS2_VAD_BINS;
constexpr int VCH = VB / 8;                            // 16-byte chunks per block: 20
constexpr int VTILE = 64;                              // blocks per workgroup pass of the energy kernel
constexpr int VTCH = VTILE * VCH;                      // chunks per tile: 1280 (+ 1 when pcm is not 16-byte aligned)
constexpr int VNT = 1024;                              // threads of the runs kernel
constexpr int VNW = VNT / 64;

typedef unsigned long long u64;

__device__ __forceinline__ unsigned vad_sq2(int a, int b) {           // two squares: at most 2^31
    return (unsigned)(a * a) + (unsigned)(b * b);
}

__device__ __forceinline__ int vad_bin(u64 s) {
    if (s < 4) return (int)s;
    const int e = 63 - __clzll((long long)s);
    return 4 * e + (int)((s >> (e - 2)) & 3);
}

// E[j] for every block.  `mis` samples lie between the 16-byte boundary below pcm and pcm itself: chunk q of the aligned
// stream holds samples 8 q - mis .. 8 q - mis + 7, so a chunk with q % 20 == 0 gives its first `mis` samples to the block
// before it.  A chunk that is not wholly inside pcm[0, n) is read sample by sample: nothing outside is touched.
__global__ __launch_bounds__(256) void vad_energy_kernel(const int16_t* __restrict__ pcm, long long n, int nb, int mis,
                                                         u64* __restrict__ E, unsigned* __restrict__ hist) {
    __shared__ u64 main_s[VTCH + 1];
    __shared__ u64 early_s[VTILE + 1];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < VBINS) hist[tid] = 0;                 // for the next launch's atomics
    const int16_t* ap = pcm - mis;                                     // 16-byte aligned
    const int ntiles = (nb + VTILE - 1) / VTILE;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long q0 = (long long)tile * VTCH;
        for (int c = tid; c < VTCH + (mis ? 1 : 0); c += 256) {
            const long long q = q0 + c, r0 = 8 * q - mis;              // first sample of the chunk
            int x[8];
            if (r0 >= n) {
#pragma unroll
                for (int t = 0; t < 8; ++t) x[t] = 0;
            } else if (r0 >= 0 && r0 + 8 <= n) {
                const int4 v = *reinterpret_cast<const int4*>(ap + 8 * q);
                x[0] = (int16_t)(v.x & 0xffff); x[1] = v.x >> 16;
                x[2] = (int16_t)(v.y & 0xffff); x[3] = v.y >> 16;
                x[4] = (int16_t)(v.z & 0xffff); x[5] = v.z >> 16;
                x[6] = (int16_t)(v.w & 0xffff); x[7] = v.w >> 16;
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const long long i = r0 + t;
                    x[t] = (i >= 0 && i < n) ? (int)pcm[i] : 0;
                }
            }
            if (c % VCH == 0 && mis) {                                 // the straddling chunk: samples t < mis are early
                u64 early = 0, rest = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const u64 sq = (u64)(unsigned)(x[t] * x[t]);
                    if (t < mis) early += sq; else rest += sq;
                }
                early_s[c / VCH] = early;
                main_s[c] = rest;
            } else {
                main_s[c] = (u64)vad_sq2(x[0], x[1]) + (u64)vad_sq2(x[2], x[3]) + (u64)vad_sq2(x[4], x[5]) +
                            (u64)vad_sq2(x[6], x[7]);
            }
        }
        __syncthreads();
        const int b = tid >> 2, part = tid & 3;
        u64 s = 0;
#pragma unroll
        for (int i = 0; i < VCH / 4; ++i) s += main_s[b * VCH + part * (VCH / 4) + i];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        const int j = tile * VTILE + b;
        if (part == 0 && j < nb) E[j] = s + (mis ? early_s[b + 1] : 0);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void vad_level_kernel(const u64* __restrict__ E, int nb, u64* __restrict__ S,
                                                        uint8_t* __restrict__ bins, unsigned* __restrict__ hist) {
    __shared__ unsigned lh[VBINS];
    const int tid = threadIdx.x;
    if (tid < VBINS) lh[tid] = 0;
    __syncthreads();
    for (int j = blockIdx.x * 256 + tid; j < nb; j += gridDim.x * 256) {
        const u64 s = (j > 0 ? E[j - 1] : 0) + E[j] + (j + 1 < nb ? E[j + 1] : 0);
        const int b = min(vad_bin(s), VBINS - 1);                      // (155 at most for sums of int16 squares)
        S[j] = s;
        bins[j] = (uint8_t)b;
        atomicAdd(&lh[b], 1u);
    }
    __syncthreads();
    if (tid < VBINS && lh[tid]) atomicAdd(&hist[tid], lh[tid]);
}

__device__ __forceinline__ int vad_byte(const uint4& v, int t) {       // byte t of 16 (t a constant after unrolling)
    const unsigned w = (t >> 2) == 0 ? v.x : (t >> 2) == 1 ? v.y : (t >> 2) == 2 ? v.z : v.w;
    return (int)((w >> (8 * (t & 3))) & 255u);
}

// exclusive prefix of v over the 1024 threads in thread order, and the total (every thread calls it)
__device__ int vad_scan(int v, int* wsum, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                                                   // wsum may still be read from the previous call
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < VNW; ++i) {
        const int s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    return base + x - v;
}

// Step 7 for one run [s, e) by one wave (s, e wave-uniform).  Returns the number of pieces; with `segs` writes piece i to
// row o + i while that row is below cap.
__device__ int vad_split(const u64* __restrict__ S, int s, int e, int max_len, int h, int32_t* segs, int o, int cap,
                         int lane) {
    int cnt = 0;
    while (e - s > max_len) {
        const int lo = s + h, hi = min(s + max_len, e - h);            // e - s >= 2 h: lo <= hi
        u64 best = ~0ull;
        int bi = 0x7fffffff;
#pragma unroll 4
        for (int c = lo + lane; c <= hi; c += 64) {                    // ascending c: a strict < keeps the smallest
            const u64 v = S[c];
            if (v < best) {
                best = v;
                bi = c;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov < best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (segs && lane == 0 && o + cnt < cap) {
            segs[2 * (o + cnt)] = s;
            segs[2 * (o + cnt) + 1] = bi;
        }
        s = bi;
        ++cnt;
    }
    if (segs && lane == 0 && o + cnt < cap) {
        segs[2 * (o + cnt)] = s;
        segs[2 * (o + cnt) + 1] = e;
    }
    return cnt + 1;
}

struct VadArgs {
    int nb, rank, margin_bins, min_bin, max_bin, min_speech, min_silence, pad, max_len, seg_cap;
};

__global__ __launch_bounds__(VNT) void vad_runs_kernel(const uint8_t* __restrict__ bins, const u64* __restrict__ S,
                                                       const unsigned* __restrict__ hist, VadArgs a, int32_t* starts,
                                                       int32_t* ends, int32_t* mstart, int32_t* mend, int32_t* cnt,
                                                       int32_t* off, int32_t* segs, int32_t* info) {
    __shared__ int wsum[VNW];
    __shared__ int thr_s[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = a.nb, cap = a.seg_cap;
    if (nb == 0) {
        for (int r = tid; r < 2 * cap; r += VNT) segs[r] = -1;
        if (tid < 8) info[tid] = 0;
        return;
    }
    // step 3: the threshold
    if (tid == 0) {
        unsigned cum = 0;
        int k = 0;
        for (; k < VBINS - 1; ++k) {
            cum += hist[k];
            if (cum > (unsigned)a.rank) break;
        }
        thr_s[0] = k;
        thr_s[1] = min(max(k + a.margin_bins, a.min_bin), a.max_bin);
    }
    __syncthreads();
    const int floor_bin = thr_s[0], thr = thr_s[1];

    // raw runs of the mask: thread t owns blocks [j0, j1), j0 a multiple of 16, and takes its level bytes 16 per load (the
    // bytes between nb and the next multiple of 16 lie inside the workspace and are skipped)
    int R;
    {
        const int chunk = ((nb + VNT - 1) / VNT + 15) & ~15;
        const int j0 = min(tid * chunk, nb), j1 = min(j0 + chunk, nb);
        const int prev = j0 > 0 && j0 < nb ? (bins[j0 - 1] >= thr) : 0;
        int c = 0, p = prev;
        for (int j = j0; j < j1; j += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(bins + j);
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j + t < j1) {
                    const int m = vad_byte(v, t) >= thr;
                    c += m & (p ^ 1);
                    p = m;
                }
        }
        int k = vad_scan(c, wsum, tid, &R);
        p = prev;
        for (int j = j0; j < j1; j += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(bins + j);
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j + t < j1) {
                    const int m = vad_byte(v, t) >= thr;
                    if (m && !p) starts[k++] = j + t;
                    if (!m && p) ends[k - 1] = j + t;                  // the run's start is behind j + t: k >= 1
                    p = m;
                }
        }
        if (tid == 0 && bins[nb - 1] >= thr) ends[R - 1] = nb;
    }
    __syncthreads();

    // step 4: raw run k opens a merged run unless the gap before it is shorter than min_silence
    int G;
    {
        const int chunk = (R + VNT - 1) / VNT;
        const int k0 = min(tid * chunk, R), k1 = min(k0 + chunk, R);
        int c = 0;
        for (int k = k0; k < k1; ++k) c += (k == 0 || starts[k] - ends[k - 1] >= a.min_silence);
        int g = vad_scan(c, wsum, tid, &G);
        for (int k = k0; k < k1; ++k)
            if (k == 0 || starts[k] - ends[k - 1] >= a.min_silence) {
                mstart[g] = starts[k];
                if (k > 0) mend[g - 1] = ends[k - 1];
                ++g;
            }
        if (tid == 0 && R > 0) mend[G - 1] = ends[R - 1];
    }
    __syncthreads();

    // steps 5-7: pieces per merged run (0 = dropped); a run longer than max_len is counted by a wave.  Wave w takes the
    // runs g = w (mod 16), so neighbouring long runs are cut side by side
    const int h = (a.max_len + 1) / 2;
    int speech = 0;
    for (int g0 = 0; g0 * VNW < G; g0 += 64) {
        const int g = (g0 + lane) * VNW + wave;
        int s = 0, e = 0, c = 0;
        if (g < G) {
            s = mstart[g];
            e = mend[g];
            if (e - s >= a.min_speech) {
                speech += e - s;
                s = max(0, s - a.pad);
                e = min(nb, e + a.pad);
                c = 1;
            }
        }
        unsigned long long longs = __ballot(c && e - s > a.max_len);
        while (longs) {
            const int src = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            const int n = vad_split(S, __shfl(s, src, 64), __shfl(e, src, 64), a.max_len, h, nullptr, 0, 0, lane);
            if (lane == src) c = n;
        }
        if (g < G) cnt[g] = c;
    }
    int n_speech;
    vad_scan(speech, wsum, tid, &n_speech);
    __syncthreads();

    // step 8: the first row of every merged run
    int n_seg;
    {
        const int chunk = (G + VNT - 1) / VNT;
        const int g0 = min(tid * chunk, G), g1 = min(g0 + chunk, G);
        int c = 0;
        for (int g = g0; g < g1; ++g) c += cnt[g];
        int o = vad_scan(c, wsum, tid, &n_seg);
        for (int g = g0; g < g1; ++g) {
            off[g] = o;
            o += cnt[g];
        }
    }
    __syncthreads();
    for (int g0 = 0; g0 * VNW < G; g0 += 64) {
        const int g = (g0 + lane) * VNW + wave;
        int s = 0, e = 0, o = 0, c = 0;
        if (g < G) {
            c = cnt[g];
            o = off[g];
            s = max(0, mstart[g] - a.pad);
            e = min(nb, mend[g] + a.pad);
            if (c == 1 && o < cap) {
                segs[2 * o] = s;
                segs[2 * o + 1] = e;
            }
        }
        unsigned long long longs = __ballot(c > 1);
        while (longs) {
            const int src = __ffsll((long long)longs) - 1;
            longs &= longs - 1;
            vad_split(S, __shfl(s, src, 64), __shfl(e, src, 64), a.max_len, h, segs, __shfl(o, src, 64), cap, lane);
        }
    }
    for (int r = 2 * min(n_seg, cap) + tid; r < 2 * cap; r += VNT) segs[r] = -1;
    if (tid < 8) {
        const int v[8] = {n_seg, floor_bin, thr, n_speech, nb, 0, 0, 0};
        info[tid] = v[tid];
    }
}

struct VadLayout {
    size_t e, s, hist, runs[6], bins, total;
};

inline size_t vad_up(size_t x) { return (x + 255) & ~(size_t)255; }

VadLayout vad_layout(size_t n) {
    const size_t nb = (n + VB - 1) / VB, rmax = nb / 2 + 1;
    VadLayout l;
    size_t at = 0;
    l.e = at, at += vad_up(nb * sizeof(u64));
    l.s = at, at += vad_up(nb * sizeof(u64));
    l.hist = at, at += vad_up(VBINS * sizeof(unsigned));
    for (int i = 0; i < 6; ++i) l.runs[i] = at, at += vad_up(rmax * sizeof(int32_t));
    l.bins = at, at += vad_up(nb);
    l.total = at;
    return l;
}

}  // namespace

extern "C" size_t ds2_vad_segment_ws_bytes(size_t n) { return vad_layout(n).total; }

extern "C" int ds2_vad_segment(const int16_t* pcm, size_t n, int rank, int margin_bins, int min_bin, int max_bin,
                               int min_speech, int min_silence, int pad, int max_len, void* ws, size_t ws_bytes,
                               int32_t* segs, int seg_cap, int32_t* info, void* stream) {
    DS2_CHECK_ARG(n < ((size_t)1 << 31));
    const int nb = (int)((n + VB - 1) / VB);
    DS2_CHECK_ARG((pcm || n == 0) && ((uintptr_t)pcm & 1) == 0);
    DS2_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0 && segs && ((uintptr_t)segs & 3) == 0 && info && ((uintptr_t)info & 3) == 0);
    DS2_CHECK_ARG(min_speech >= 2 && max_len >= 4 && pad >= 0 && pad < (1 << 29) && 2 * pad < min_silence);
    DS2_CHECK_ARG(rank >= 0 && rank <= (nb > 0 ? nb - 1 : 0));
    DS2_CHECK_ARG(margin_bins >= 0 && margin_bins < VBINS && min_bin >= 0 && min_bin < VBINS && max_bin >= 0 &&
                  max_bin < VBINS);
    DS2_CHECK_ARG(seg_cap >= 1 && seg_cap < (1 << 30));
    const VadLayout l = vad_layout(n);
    DS2_CHECK_ARG(ws_bytes >= l.total);
    // keeps s + max_len and (max_len + 1) / 2 inside int for a huge max_len; no run is longer than nb, so nothing is split
    // either way and h, which changes with it, is never used
    if (max_len > nb) max_len = nb > 4 ? nb : 4;
    char* w = (char*)ws;
    u64* E = (u64*)(w + l.e);
    u64* S = (u64*)(w + l.s);
    unsigned* hist = (unsigned*)(w + l.hist);
    int32_t* runs[6];
    for (int i = 0; i < 6; ++i) runs[i] = (int32_t*)(w + l.runs[i]);
    uint8_t* bins = (uint8_t*)(w + l.bins);
    hipStream_t st = (hipStream_t)stream;
    if (nb > 0) {
        const int mis = (int)(((uintptr_t)pcm & 15) / 2);
        const int ntiles = (nb + VTILE - 1) / VTILE;
        hipLaunchKernelGGL(vad_energy_kernel, dim3(ntiles < 1024 ? ntiles : 1024), dim3(256), 0, st, pcm, (long long)n, nb,
                           mis, E, hist);
        DS2_CHECK_LAUNCH();
        const int lv = (nb + 255) / 256;
        hipLaunchKernelGGL(vad_level_kernel, dim3(lv < 256 ? lv : 256), dim3(256), 0, st, E, nb, S, bins, hist);
        DS2_CHECK_LAUNCH();
    }
    const VadArgs a = {nb, rank, margin_bins, min_bin, max_bin, min_speech, min_silence, pad, max_len, seg_cap};
    hipLaunchKernelGGL(vad_runs_kernel, dim3(1), dim3(VNT), 0, st, bins, S, hist, a, runs[0], runs[1], runs[2], runs[3],
                       runs[4], runs[5], segs, info);
    DS2_CHECK_LAUNCH();
    return DS2_OK;
}
