// Persistent BiGRU recurrence, the 16x16 MFMA forms (round 1: whole batch per workgroup; round 2: two batch parts; round 3: two
// parts on the bf16 matrix pipe with split operands) -- the forms B >= 13 (forward) / B >= 17 (backward) and every width the
// 4x4x1 forms of gru_persist.hip do not cover run.  Split out of gru_persist.hip in round 6; the protocol description, the
// exchange workspace and the C entry points are there.
//
// Five of the six kernels are one time step written once, as parts (gru_fwd_persistent_p2b_kernel is written out: see there):
//   Role            who a thread is: MFMA lane (m, q), gate thread (unit jj, batch row nn of tile gbt), batch part, counters
//   OpF32 / OpBf16  operand policy: resident weights of a gate row, one k block's fragment from the ring, accumulate
//   fetch_mfma      the (batch tile, k chunk) pipeline: hand-off fetch -> MFMA -> red[]
//   PutScalar / PutQuad / PutOctet   hand-off store policy: value v of k index k, batch row nn, tile gbt
//   step_arrived / finish_step       arrival wait + abort; drain + barrier + arrival add
//   BwdSaved / bwd_cell              the backward step's saved-activation loads and gate maths
// and two bodies, fwd_recurrence and bwd_recurrence, that a form struct (FwdWhole .. BwdP2b) parameterises.  The forward gate
// maths and both directions' saved-activation stores stand in their one body: behind a struct-returning helper the forward
// maths kept its arithmetic but the compiler placed its waits differently in more of the forward kernels.  What a form
// struct names is what those kernels really differ in; every such difference is a measured decision or says that it is not.
// profiles/gru16_refactor.md holds the comparison of the compiled kernels with the six written-out ones they replace.
#include "gru_persist_common.h"
#include "split_bf16.h"

namespace {

typedef __bf16 gbf16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------- role
// UNITS hidden units per workgroup (8 = PJU: the whole-batch forms; 16: the two-part forms, 512 threads = 16 units x 32 rows);
// PARTS: blockIdx.z is a batch part.
template <int UNITS, bool PARTS>
struct Role {
    static constexpr int LOG_UNITS = UNITS == 8 ? 3 : 4;
    int tid, lane, wave, dir, part, nslice, j0, m, q;
    int jj, nn, gbt, gb, gj;                            // gate role: unit jj, batch row 16 gbt + nn of this part
    bool gate_ok;
    unsigned int* shards;

    // false: this part has no batch rows and the workgroup has left the kernel
    __device__ __forceinline__ bool init(int nbt, int B, int H, SyncWs* sync) {
        tid = threadIdx.x, lane = tid & 63;
        // readfirstlane makes everything derived from the wave id provably wave-uniform: uniform branches and SGPR
        // buffer descriptors instead of per-load waterfall loops (cdna_hip_programming.md T20)
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        dir = blockIdx.y, part = PARTS ? blockIdx.z : 0, nslice = gridDim.x;
        j0 = blockIdx.x * UNITS;
        m = lane & 15, q = lane >> 4;
        const int bper = PARTS ? (B + 1) / 2 : B, b0 = part * bper, nb = min(bper, B - b0);
        if (PARTS && nb <= 0) {
            if (tid == 0) leave_kernel(sync);
            return false;
        }
        jj = tid & (UNITS - 1), nn = (tid >> LOG_UNITS) & 15, gbt = tid >> (LOG_UNITS + 4);
        const int lb = gbt * 16 + nn;
        gb = b0 + lb, gj = j0 + jj;
        gate_ok = (gbt < nbt) && (lb < nb) && (gj < H);
        shards = &sync->arrive[dir][part][0][0];
        return true;
    }
    // The weight row of MFMA row m.  The two address forms are as the kernels were written, never measured against each other:
    // the 8-unit forms address unit j0 + (m & 7) as it is (rows 8 .. 15 of their tile repeat or pad), the 16-unit forms
    // clamp a unit >= H to row 0; neither reads a row whose `ok` is false.
    __device__ __forceinline__ int weight_unit(int H, bool& ok) const {
        const int u = j0 + (UNITS == 8 ? (m & 7) : m);
        ok = u < H;
        return UNITS == 8 ? u : (ok ? u : 0);
    }
};

// The exchange ring of one (direction, batch part): two slots of nbt * nkb k blocks of Op::BLOCK_BYTES
struct Ring {
    char* base;
    int slot_bytes, nkb;
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t read_slot(int slot) const {
        return __builtin_amdgcn_make_buffer_rsrc(base + (size_t)slot * slot_bytes, 0, slot_bytes, 0x00020000);
    }
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t both_slots() const {
        return __builtin_amdgcn_make_buffer_rsrc(base, 0, 2 * slot_bytes, 0x00020000);
    }
};
template <class Op, int NBT, class R>
__device__ __forceinline__ Ring ring_of(float* ring, const R& ro, int K, bool parts) {
    Ring rg;
    rg.nkb = K / Op::KB;
    rg.slot_bytes = NBT * rg.nkb * Op::BLOCK_BYTES;
    rg.base = reinterpret_cast<char*>(ring) + (size_t)(ro.dir * (parts ? 2 : 1) + ro.part) * 2 * rg.slot_bytes;
    return rg;
}

// ---------------------------------------------------------------------------------------------------------- operand policies
// fp32 operands on v_mfma_f32_16x16x4_f32: k blocks of 16, four MFMAs per block.
// The ring of a (direction, part) is laid out [slot 2][batch tile][k block][k quad 4][16 batch rows][4 k]: the
// MFMA B fragment of lane l is bytes 16 l .. 16 l + 15 of ONE contiguous kilobyte, so a wave-load is eight
// whole 128-B lines read in lane order (the (b, k) layout of hout gives 10-16 scattered 64-B pieces per
// load and ran the CU's inbound path at ~27 GB/s; a [16 batch][16 k] block is contiguous per wave but
// each 16-lane quarter still gathers four 64-B pieces and measured ~1 us/step slower)
struct OpF32 {
    static constexpr int KB = 16, BLOCK_BYTES = 1024;
    typedef f32x4 W;
    typedef f32x4 X;
    static __device__ __forceinline__ W load_w(const float* row, int kb, int q, bool ok) {
        return ok ? *reinterpret_cast<const f32x4*>(row + kb * 16 + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // rows of padding batch entries hold whatever an earlier launch left: their products land in
    // output columns >= B, which no gate thread reads
    // k blocks past the end: an offset beyond the descriptor's range reads as zero, with no branch
    static __device__ __forceinline__ X fetch(__amdgpu_buffer_rsrc_t rs, int bt, int nkb, int kb, int lane) {
        return LOAD_HANDOFF(rs, (kb < nkb) ? ((bt * nkb + kb) * 256 + lane * 4) * 4 : OOB_OFFSET);
    }
    template <int NG, int KBW>
    static __device__ __forceinline__ void mma(const W (&w)[NG][KBW], int i, const X& x, f32x4 (&acc)[NG]) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[g][i][e], x[e], acc[g], 0, 0, 0);
    }
};

// The two-part forms on the bf16 matrix pipe (B >= 17, H % 32 == 0).  From B = 17 half of a recurrence step is
// matrix-pipe time (16 units x 16 batch rows x 3 H k per workgroup on v_mfma_f32_16x16x4_f32: 84 / 76 instructions of 32
// cycles per wave and batch tile).  Here every fp32 operand is split without error into three bf16 terms (split_bf16.h) and
// the products run on v_mfma_f32_16x16x32_bf16 -- six exact partial products per 32 k, 16 cycles each: 0.43 x the pipe time
// for the same fp32 result (the accumulator is fp32 as before).  The weights are split once per launch into registers
// (three planes of 8 bf16 per lane and 32-k block: 1.5 x the registers of the fp32 copy); the NEW state is split by the
// gate thread that produces it and written to the exchange ring as three bf16 planes, eight units per 16-byte write-through
// store (two neighbours' values are packed by one split, the four dwords of an octet gathered with DPP) -- 1.5 x the
// hand-off bytes, no conversion on the consumers' side.
// Ring layout of a (direction, part): [slot 2][batch tile][k block of 32][plane 3][k octet 4][16 batch rows][8 k] bf16: a
// wave-load of one plane of one block is 1 KB contiguous, lane l = (batch row l & 15, octet l >> 4).
struct OpBf16 {
    static constexpr int KB = 32, BLOCK_BYTES = 3 * 1024;
    struct W { gbf16x8 p[3]; };                         // row m, k = 32 kb + 8 q .. + 7, three planes
    typedef W X;
    static __device__ __forceinline__ W load_w(const float* row, int kb, int q, bool ok) {
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            lo = *reinterpret_cast<const f32x4*>(row + kb * 32 + q * 8);
            hi = *reinterpret_cast<const f32x4*>(row + kb * 32 + q * 8 + 4);
        }
        unsigned int pl[3][4];
        split3(lo[0], lo[1], pl[0][0], pl[1][0], pl[2][0]);
        split3(lo[2], lo[3], pl[0][1], pl[1][1], pl[2][1]);
        split3(hi[0], hi[1], pl[0][2], pl[1][2], pl[2][2]);
        split3(hi[2], hi[3], pl[0][3], pl[1][3], pl[2][3]);
        W w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u32x4 v = {pl[c][0], pl[c][1], pl[c][2], pl[c][3]};
            w.p[c] = __builtin_bit_cast(gbf16x8, v);
        }
        return w;
    }
    static __device__ __forceinline__ X fetch(__amdgpu_buffer_rsrc_t rs, int bt, int nkb, int kb, int lane) {
        X x;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            x.p[c] = __builtin_bit_cast(
                gbf16x8, LOAD_HANDOFF(rs, (kb < nkb) ? ((bt * nkb + kb) * 3 + c) * 1024 + lane * 16 : OOB_OFFSET));
        return x;
    }
    template <int NG, int KBW>
    static __device__ __forceinline__ void mma(const W (&w)[NG][KBW], int i, const X& x, f32x4 (&acc)[NG]) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 a = acc[g];
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[1], x.p[1], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[0], x.p[2], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[2], x.p[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[0], x.p[1], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[1], x.p[0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[g][i].p[0], x.p[0], a, 0, 0, 0);
            acc[g] = a;
        }
    }
};

// ---------------------------------------------------------------------------------------------------------- fetch -> MFMA -> red[]
// Stages = (batch tile, chunk of CH k blocks); NG gate tiles share each fetched fragment.  The fragments of stage st + 1
// are in flight while the MFMAs of stage st issue (fully unrolled so the two fragment buffers stay in registers).
// SKIP_TAIL: see below.
template <class Op, int NG, int NBT, int KBW, int CH, bool SKIP_TAIL>
__device__ __forceinline__ void fetch_mfma(const typename Op::W (&w)[NG][KBW], __amdgpu_buffer_rsrc_t rs, int nkb, int wave,
                                           int lane, int m, int q, float (&red)[NWP][NG][NBT][16][17]) {
    constexpr int NCH = (KBW + CH - 1) / CH, NST = NBT * NCH;
    static_assert(!SKIP_TAIL || NCH == 1, "the tail test looks at a stage's last k block");
    typename Op::X bf[2][CH];
    auto fetch = [&](int st, typename Op::X (&dst)[CH]) {
        const int bt = st / NCH, i0 = (st % NCH) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int kb = wave + NWP * (i0 + c);                  // wave-uniform
            if (i0 + c < KBW)                                      // compile-time
                dst[c] = Op::fetch(rs, bt, nkb, kb, lane);
            else
                dst[c] = typename Op::X{};
        }
    };
    fetch(0, bf[0]);
    f32x4 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < NST; ++st) {
        if (st + 1 < NST) fetch(st + 1, bf[(st + 1) & 1]);
        // all loads out before the MFMAs (the scheduler would otherwise sink them in between, 2 in flight)
        __builtin_amdgcn_sched_barrier(0);
        const int bt = st / NCH, i0 = (st % NCH) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = i0 + c;
            if (i >= KBW) break;                                   // compile-time
            // the forward step is MFMA-issue bound: a wave whose last k block lies past H (H = 800: 50 blocks
            // over 8 waves, six of them own 6 not 7) skips its all-zero MFMAs (wave-uniform branch).  The backward
            // kernels never had the test; nobody has measured it there.
            if (SKIP_TAIL && i == KBW - 1 && wave + NWP * i >= nkb) break;
            Op::mma(w, i, bf[st & 1][c], acc);
        }
        if ((st % NCH) == NCH - 1) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave][g][bt][4 * q + r][m] = acc[g][r];
                acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- hand-off stores
// A policy gathers a value from the neighbouring gate threads (EVERY lane calls gather: DPP needs the whole row active)
// and the lanes it names storers put the payload at k index k, batch row nn, tile gbt of slot s & 1.

// one 4-byte write-through store per gate thread
struct PutScalar {
    typedef float Payload;
    static __device__ __forceinline__ Payload gather(float v) { return v; }
    static __device__ __forceinline__ bool storer(int jj) { return true; }
    static __device__ __forceinline__ void put(const Ring& rg, int s, int nbt, int gbt, int nn, int k, Payload v) {
        float* slot = reinterpret_cast<float*>(rg.base) + ((size_t)(s & 1) * nbt + gbt) * (size_t)rg.nkb * 256 + nn * 4;
        store_sc1(&slot[(size_t)(k >> 4) * 256 + ((k & 15) >> 2) * 64 + (k & 3)], v);
    }
};
// Four neighbouring gate threads (units 4u .. 4u+3 of one batch row: adjacent lanes, 16 contiguous bytes of the ring) hand
// their values to the first of them, which issues ONE 16-byte write-through store: a quarter of the fabric writes
// (a 4-byte sc1 store costs about six times a 16-byte one per byte).  H % 16 == 0: a quad never straddles H.
struct PutQuad {
    typedef f32x4 Payload;
    static __device__ __forceinline__ Payload gather(float v) {
        f32x4 hq;
        hq[0] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x00, 0xF, 0xF, true));
        hq[1] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x55, 0xF, 0xF, true));
        hq[2] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xAA, 0xF, 0xF, true));
        hq[3] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xFF, 0xF, 0xF, true));
        return hq;
    }
    static __device__ __forceinline__ bool storer(int jj) { return (jj & 3) == 0; }
    static __device__ __forceinline__ void put(const Ring& rg, int s, int nbt, int gbt, int nn, int k, Payload v) {
        store_sc1_b128(rg.both_slots(),
                       (s & 1) * rg.slot_bytes + ((gbt * rg.nkb + (k >> 4)) * 256 + ((k & 15) >> 2) * 64 + nn * 4) * 4,
                       __builtin_bit_cast(u32x4, v));
    }
};
// the octet gather of one plane: lanes 8 o + {0, 2, 4, 6} hold the packed pairs; lane 8 o receives all four
__device__ __forceinline__ u32x4 gather_octet(unsigned int pair) {
    const int p = (int)pair;
    const int x1 = __builtin_amdgcn_update_dpp(0, p, 0xAA, 0xF, 0xF, true);      // quad lane 2's pair
    const int x2 = __builtin_amdgcn_update_dpp(0, p, 0x104, 0xF, 0xF, true);     // row_shl:4 -> lane + 4's pair
    const int x3 = __builtin_amdgcn_update_dpp(0, x1, 0x104, 0xF, 0xF, true);    // lane + 6's pair
    u32x4 v;
    v[0] = pair;
    v[1] = (unsigned int)x1;
    v[2] = (unsigned int)x2;
    v[3] = (unsigned int)x3;
    return v;
}
// split this thread's value together with its odd neighbour's (lanes 2 i, 2 i + 1 hold units 2 i, 2 i + 1 of one batch row)
// and gather the octet: planes[q] is valid in lanes with (unit & 7) == 0
__device__ __forceinline__ void split_gather_octet(float v, u32x4 (&planes)[3]) {
    const float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // lane ^ 1
    unsigned int p1, p2, p3;
    split3(v, nb, p1, p2, p3);
    planes[0] = gather_octet(p1);
    planes[1] = gather_octet(p2);
    planes[2] = gather_octet(p3);
}
// Three bf16 planes, eight units per 16-byte store.  H % 32 == 0: an octet of units is an octet of k.
struct PutOctet {
    struct Payload { u32x4 p[3]; };
    static __device__ __forceinline__ Payload gather(float v) {
        Payload pl;
        split_gather_octet(v, pl.p);
        return pl;
    }
    static __device__ __forceinline__ bool storer(int jj) { return (jj & 7) == 0; }
    static __device__ __forceinline__ void put(const Ring& rg, int s, int nbt, int gbt, int nn, int k, const Payload& v) {
        const __amdgpu_buffer_rsrc_t rs_w = rg.both_slots();
        const int base = (s & 1) * rg.slot_bytes + (gbt * rg.nkb + (k >> 5)) * 3 * 1024 + ((k & 31) >> 3) * 256 + nn * 16;
#pragma unroll
        for (int c = 0; c < 3; ++c) store_sc1_b128(rs_w, base + c * 1024, v.p[c]);
    }
};

// ---------------------------------------------------------------------------------------------------------- step frame
// false: a spin timed out somewhere (the sticky error flag is set) and the workgroup leaves
__device__ __forceinline__ bool step_arrived(int dbg, int wave, int lane, unsigned int* shards, int s, int nslice, SyncWs* sync,
                                             int& abort_flag) {
    if (!DS2_DBG(dbg, 1) && wave == 0 && !wait_arrivals(shards, s, nslice, lane, &sync->error) && lane == 0) abort_flag = 1;
    __syncthreads();
    return !abort_flag;
}
__device__ __forceinline__ void finish_step(int dbg, int tid, unsigned int* shards) {
    if (!DS2_DBG(dbg, 4)) wait_vmcnt0();   // every storing wave drains its hand-off store
    __syncthreads();
    if (tid == 0)
        __hip_atomic_fetch_add(shards + (blockIdx.x % NSHARD) * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------- gate maths
// saved activations of step t (written by the forward pass, an earlier launch): plain loads
struct BwdSaved {
    float dh, r, z, n, gn, hpv;
    template <class R>
    __device__ __forceinline__ void load(const R& ro, const float* G, const float* ghn, const float* hout, const float* d_out,
                                         int t, int T, int B, int H) {
        dh = r = z = n = gn = hpv = 0.f;
        if (ro.gate_ok) {
            const bool has_prev = ro.dir == 0 ? (t > 0) : (t < T - 1);
            const size_t row = ((size_t)t * B + ro.gb) * 2 + ro.dir, gbase = row * 3 * H + ro.gj;
            dh = d_out[((size_t)t * B + ro.gb) * H + ro.gj];
            r = G[gbase];
            z = G[gbase + H];
            n = G[gbase + 2 * H];
            gn = ghn[row * H + ro.gj];
            if (has_prev) hpv = hout[(((size_t)ro.dir * T + (ro.dir == 0 ? t - 1 : t + 1)) * B + ro.gb) * H + ro.gj];
        }
    }
};
// No contraction: these values are defined without a fused multiply-add, and whether the compiler fuses 1 - n * n depends
// on how its vectoriser pairs the neighbouring products: behind most helper shapes (reference outputs, arguments by
// value) the same statements compile to a v_pk_fma_f32, i.e. other bits.
struct BwdCell { float dr_pre, dz_pre, dn_pre, dghn, dhz; };
__device__ __forceinline__ BwdCell bwd_cell(float dh, const BwdSaved& a) {
#pragma clang fp contract(off)
    BwdCell c;
    c.dn_pre = dh * (1.f - a.z) * (1.f - a.n * a.n);
    c.dz_pre = dh * (a.hpv - a.n) * a.z * (1.f - a.z);
    c.dr_pre = c.dn_pre * a.gn * a.r * (1.f - a.r);
    c.dghn = c.dn_pre * a.r;
    c.dhz = dh * a.z;                                   // dh * z carried to the next (earlier) step
    return c;
}

// ---------------------------------------------------------------------------------------------------------- the forms
// What the five kernels built from the parts differ in.  LATE_LOAD (backward): the saved activations of step s + 1 are
// loaded at the END of step s, behind the saved-activation stores, instead of at the top of step s + 1 in front of its
// hand-off loads (round 4, as in the 4x4x1 kernels: a wave's vector-memory operations complete in issue order).  Backward
// p2 has the scheme and its two neighbours do not; no measurement of it on any of them is recorded.
// chunk<NBT, KBW>(): k blocks per fetch stage (fetch_mfma).  The chunk sizes are as the kernels were written; no
// measurement that chose between them is recorded.

// Forward, whole batch per workgroup: 8 units, two gate tiles -- tile 0 rows = [r units | z units], tile 1 rows =
// [n units | unused].  NBT = batch tiles of 16 (1; 2 and 4 only in the tuning library).
struct FwdWhole {
    typedef OpF32 Op;
    typedef PutScalar Put;
    static constexpr int UNITS = PJU, NG = 2;
    static constexpr bool PARTS = false;
    template <int NBT, int KBW> static constexpr int chunk() { return KBW; }
};
// Forward, 16x16x4 form with TWO batch parts (blockIdx.z): a workgroup owns 16 units and half the batch, so
// its gate rows fill three whole tiles (r16, z16, n16; the 8-unit form above pads its second tile by half) and it loads
// half the hidden state per step.  For B >= 24: per wave and batch tile 3 x KBW x 4 MFMAs instead of 2 x 2 x KBW x 4 for
// the two tiles a whole batch of 32 needs.  NBT = batch tiles of 16 per part (1 or 2).
struct FwdP2 {
    typedef OpF32 Op;
    typedef PutQuad Put;
    static constexpr int UNITS = 16, NG = 3;
    static constexpr bool PARTS = true;
    template <int NBT, int KBW> static constexpr int chunk() { return KBW; }
};
// Backward, whole batch per workgroup: rows m < 8 of the one tile are columns j0 + m of W_hh = rows of w_hh_t; K = 3 H:
// dGH of the previous step = [dr_pre | dz_pre | d(gh_n)] comes from the ring.
// ONE_GATE: see BwdP2b.
struct BwdWhole {
    typedef OpF32 Op;
    typedef PutScalar Put;
    static constexpr int UNITS = PJU;
    static constexpr bool PARTS = false, LATE_LOAD = false, ONE_GATE = false;
    template <int NBT, int KBW> static constexpr int chunk() { return (NBT > 1 && KBW > 10) ? 7 : KBW; }
};
// Backward, 16x16x4 form with TWO batch parts (blockIdx.z), the twin of FwdP2: a workgroup owns 16 units -- 16 rows of
// w_hh_t, a whole MFMA tile (the 8-unit form above pads half of every tile) -- and half the batch, so per step it pulls
// HALF of d(gh) (150 KB at B = 32 instead of 300) and issues NBT x 150 / 8 x 4 MFMAs per wave.  For B >= 17: the 4x4x1
// forms' cost grows with every batch quad (B = 32: 7.0 us per step, B = 64: 12.3), this form's with every tile of 16 rows
// per part.  The hand-off loads of k chunk c + 1 are in flight under the MFMAs of chunk c.
struct BwdP2 {
    typedef OpF32 Op;
    typedef PutQuad Put;
    static constexpr int UNITS = 16;
    static constexpr bool PARTS = true, LATE_LOAD = true, ONE_GATE = false;
    template <int NBT, int KBW> static constexpr int chunk() { return KBW > 10 ? 7 : KBW; }
};
// Backward twin of gru_fwd_persistent_p2b_kernel: rows of w_hh_t split into registers once.  The hand-off fragments of a
// batch tile are fetched in chunks of 2 k blocks (the weights take 12 registers per block, a chunk of fragments 12 per
// block too).
// ONE_GATE: the three gates' values are gathered and stored one gate at a time (12 registers of payload, not 36).
struct BwdP2b {
    typedef OpBf16 Op;
    typedef PutOctet Put;
    static constexpr int UNITS = 16;
    static constexpr bool PARTS = true, LATE_LOAD = false, ONE_GATE = true;
    template <int NBT, int KBW> static constexpr int chunk() { return KBW > 2 ? 2 : KBW; }
};

// ---------------------------------------------------------------------------------------------------------- forward
template <class F, int NBT, int KBW>
__device__ __forceinline__ void fwd_recurrence(float* __restrict__ G, float* __restrict__ ghn, float* __restrict__ hout,
                                               const float* __restrict__ w_hh, SyncWs* __restrict__ sync,
                                               float* __restrict__ ring, int T, int B, int H, int dbg) {
    typedef typename F::Op Op;
    typedef typename F::Put Put;
    constexpr int NG = F::NG;
    __shared__ float red[NWP][NG][NBT][16][17];
    __shared__ int abort_flag;

    Role<F::UNITS, F::PARTS> ro;
    if (!ro.init(NBT, B, H, sync)) return;
    const Ring rg = ring_of<Op, NBT>(ring, ro, H, F::PARTS);
    if (ro.tid == 0) abort_flag = 0;

    typename Op::W w[NG][KBW];                          // resident weights: tile g, k block wave + NWP i
    {
        bool unit_ok;
        const int unit = ro.weight_unit(H, unit_ok);
        const int hi = ro.m >> 3;                       // (whole-batch layout: upper half of tile 0 = gate z, of tile 1 unused)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int gate = NG == 3 ? g : (g == 0 ? hi : 2);
            const bool row_ok = unit_ok && (NG == 3 || g == 0 || hi == 0);
            const float* row = w_hh + ((size_t)ro.dir * 3 * H + (size_t)gate * H + unit) * H;
#pragma unroll
            for (int i = 0; i < KBW; ++i) {
                const int kb = ro.wave + NWP * i;
                w[g][i] = Op::load_w(row, kb, ro.q, kb < rg.nkb && row_ok);
            }
        }
    }
    float hp = 0.f;                                     // this thread's h_{t-1}, carried in a register
    __syncthreads();

    float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f;
    auto load_gi = [&](int t) {                         // independent of h
        if (ro.gate_ok) {
            const size_t gb3 = (((size_t)t * B + ro.gb) * 2 + ro.dir) * 3 * H + ro.gj;
            gi_r = G[gb3];
            gi_z = G[gb3 + H];
            gi_n = G[gb3 + 2 * H];
        }
    };
    for (int s = 0; s < T; ++s) {
        const int t = ro.dir == 0 ? s : T - 1 - s;
        const size_t row = ((size_t)t * B + ro.gb) * 2 + ro.dir, gbase = row * 3 * H + ro.gj;
        gi_r = gi_z = gi_n = 0.f;
        load_gi(t);                                     // issued before the wait
        if (s > 0) {
            if (!step_arrived(dbg, ro.wave, ro.lane, ro.shards, s, ro.nslice, sync, abort_flag)) return;
            if (!DS2_DBG(dbg, 2))
                fetch_mfma<Op, NG, NBT, KBW, F::template chunk<NBT, KBW>(), true>(w, rg.read_slot((s - 1) & 1), rg.nkb,
                                                                                          ro.wave, ro.lane, ro.m, ro.q, red);
        }
        __syncthreads();
        float sv_r = 0.f, sv_z = 0.f, sv_n = 0.f, sv_g = 0.f, sv_h = 0.f;
        if (ro.gate_ok) {
            float gh_r = 0.f, gh_z = 0.f, gh_n = 0.f;
            if (s > 0) {
#pragma unroll
                for (int wv = 0; wv < NWP; ++wv) {
                    gh_r += red[wv][0][ro.gbt][ro.jj][ro.nn];
                    gh_z += NG == 3 ? red[wv][1][ro.gbt][ro.jj][ro.nn] : red[wv][0][ro.gbt][8 + ro.jj][ro.nn];
                    gh_n += red[wv][NG - 1][ro.gbt][ro.jj][ro.nn];
                }
            }
            const float r = fast_sigmoid(gi_r + gh_r);
            const float z = fast_sigmoid(gi_z + gh_z);
            const float n = fast_tanh(gi_n + r * gh_n);
            const float h = (1.f - z) * n + z * hp;
            hp = h;
            sv_h = h;
            sv_r = r;
            sv_z = z;
            sv_n = n;
            sv_g = gh_n;
        }
        // handed to every other workgroup through the ring; hout keeps the plain copy for later launches
        const typename Put::Payload ph = Put::gather(sv_h);
        if (ro.gate_ok && Put::storer(ro.jj)) Put::put(rg, s, NBT, ro.gbt, ro.nn, ro.gj, ph);
        finish_step(dbg, ro.tid, ro.shards);
        if (ro.gate_ok) {   // saved activations are only read by later launches: keep them off the hand-off's critical path
            hout[(((size_t)ro.dir * T + t) * B + ro.gb) * H + ro.gj] = sv_h;
            G[gbase] = sv_r;
            G[gbase + H] = sv_z;
            G[gbase + 2 * H] = sv_n;
            ghn[row * H + ro.gj] = sv_g;
        }
    }
    if (ro.tid == 0) leave_kernel(sync);
}

// ---------------------------------------------------------------------------------------------------------- backward
template <class F, int NBT, int KBW>
__device__ __forceinline__ void bwd_recurrence(float* __restrict__ G, float* __restrict__ ghn, const float* __restrict__ hout,
                                               const float* __restrict__ d_out, const float* __restrict__ w_hh_t,
                                               SyncWs* __restrict__ sync, float* __restrict__ ring, int T, int B, int H,
                                               int dbg) {
    typedef typename F::Op Op;
    typedef typename F::Put Put;
    __shared__ float red[NWP][1][NBT][16][17];
    __shared__ int abort_flag;

    Role<F::UNITS, F::PARTS> ro;
    if (!ro.init(NBT, B, H, sync)) return;
    const int K = 3 * H;
    const Ring rg = ring_of<Op, NBT>(ring, ro, K, F::PARTS);
    if (ro.tid == 0) abort_flag = 0;

    typename Op::W w[1][KBW];                           // row m: column (j0 + m) of W_hh = row of w_hh_t
    {
        bool unit_ok;
        const int unit = ro.weight_unit(H, unit_ok);
        const bool row_ok = unit_ok && ro.m < F::UNITS;
        const float* row = w_hh_t + ((size_t)ro.dir * H + unit) * K;
#pragma unroll
        for (int i = 0; i < KBW; ++i) {
            const int kb = ro.wave + NWP * i;
            w[0][i] = Op::load_w(row, kb, ro.q, row_ok && kb < rg.nkb);
        }
    }
    float dhz = 0.f;                                    // dh * z carried to the next (earlier) step
    __syncthreads();

    BwdSaved a;
    if (F::LATE_LOAD) a.load(ro, G, ghn, hout, d_out, ro.dir == 0 ? T - 1 : 0, T, B, H);
    for (int s = 0; s < T; ++s) {
        const int t = ro.dir == 0 ? T - 1 - s : s;
        const size_t row = ((size_t)t * B + ro.gb) * 2 + ro.dir, gbase = row * 3 * H + ro.gj;
        if (!F::LATE_LOAD) a.load(ro, G, ghn, hout, d_out, t, T, B, H);   // issued before the wait
        if (s > 0) {
            if (!step_arrived(dbg, ro.wave, ro.lane, ro.shards, s, ro.nslice, sync, abort_flag)) return;
            if (!DS2_DBG(dbg, 2))
                fetch_mfma<Op, 1, NBT, KBW, F::template chunk<NBT, KBW>(), false>(w, rg.read_slot((s - 1) & 1), rg.nkb,
                                                                                       ro.wave, ro.lane, ro.m, ro.q, red);
        }
        __syncthreads();
        BwdCell c = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (ro.gate_ok) {
            float dh = a.dh;
            if (s > 0) {
                float sum = 0.f;
#pragma unroll
                for (int wv = 0; wv < NWP; ++wv) sum += red[wv][0][ro.gbt][ro.jj][ro.nn];
                dh += sum + dhz;
            }
            c = bwd_cell(dh, a);
            dhz = c.dhz;
        }
        {   // hand-off copies into the ring (write-through); k index of unit j in gate g is g * H + j
            const bool storer = ro.gate_ok && Put::storer(ro.jj);
            auto put = [&](const typename Put::Payload& p, int g) {
                Put::put(rg, s, NBT, ro.gbt, ro.nn, g * H + ro.gj, p);
            };
            if (F::ONE_GATE) {
                const typename Put::Payload p0 = Put::gather(c.dr_pre);
                if (storer) put(p0, 0);
                const typename Put::Payload p1 = Put::gather(c.dz_pre);
                if (storer) put(p1, 1);
                const typename Put::Payload p2 = Put::gather(c.dghn);
                if (storer) put(p2, 2);
            } else {
                const typename Put::Payload p0 = Put::gather(c.dr_pre), p1 = Put::gather(c.dz_pre), p2 = Put::gather(c.dghn);
                if (storer) {
                    put(p0, 0);
                    put(p1, 1);
                    put(p2, 2);
                }
            }
        }
        finish_step(dbg, ro.tid, ro.shards);
        if (ro.gate_ok) {   // d(gi), d(gh_n) for the GEMMs that follow this launch: plain stores, off the critical path
            G[gbase] = c.dr_pre;
            G[gbase + H] = c.dz_pre;
            G[gbase + 2 * H] = c.dn_pre;
            ghn[row * H + ro.gj] = c.dghn;
        }
        if (F::LATE_LOAD && s + 1 < T) a.load(ro, G, ghn, hout, d_out, ro.dir == 0 ? T - 2 - s : s + 1, T, B, H);
    }
    if (ro.tid == 0) leave_kernel(sync);
}

// ---------------------------------------------------------------------------------------------------------- the six kernels
// (the names are the ones tools/gru_pmc.sh and the tables under profiles/ match on)
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_fwd_persistent_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                                                      float* __restrict__ hout, const float* __restrict__ w_hh,
                                                                      SyncWs* __restrict__ sync, float* __restrict__ ring,
                                                                      int T, int B, int H, int dbg) {
    fwd_recurrence<FwdWhole, NBT, KBW>(G, ghn, hout, w_hh, sync, ring, T, B, H, dbg);
}
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_fwd_persistent_p2_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                                                         float* __restrict__ hout, const float* __restrict__ w_hh,
                                                                         SyncWs* __restrict__ sync, float* __restrict__ ring,
                                                                         int T, int B, int H, int dbg) {
    fwd_recurrence<FwdP2, NBT, KBW>(G, ghn, hout, w_hh, sync, ring, T, B, H, dbg);
}
// Forward, two parts on the bf16 pipe: NOT built from the parts above but written out.  Built from them (Role, OpBf16,
// fetch_mfma with a one-buffer mode, PutOctet, the forward body with a late-load switch) this kernel computes the same bits
// from the same opcode counts, but its step measured 0.02 - 0.03 us (0.5 - 1 %) slower at B = 16 .. 64, H = 800, in six
// alternations out of six (profiles/gru16_refactor.md): the compiler then schedules the tail of the cross-wave reduction
// behind one LDS wait, and no arrangement of the shared parts gives the schedule of the text below for all six
// instantiations.  It fetches a whole batch tile and then issues it, with no second buffer (not measured against a
// double-buffered form).
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_fwd_persistent_p2b_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                                                          float* __restrict__ hout,
                                                                          const float* __restrict__ w_hh,
                                                                          SyncWs* __restrict__ sync,
                                                                          float* __restrict__ ring, int T, int B, int H,
                                                                          int dbg) {
    __shared__ float red[NWP][3][NBT][16][17];
    __shared__ int abort_flag;
    constexpr int UNITS = 16;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dir = blockIdx.y, part = blockIdx.z, nslice = gridDim.x;
    const int j0 = blockIdx.x * UNITS;
    const int m = lane & 15, q = lane >> 4;
    const int nkb = H >> 5;                             // k blocks of 32
    const int bper = (B + 1) / 2, b0 = part * bper, nb = min(bper, B - b0);
    if (nb <= 0) {
        if (tid == 0) leave_kernel(sync);
        return;
    }
    const int slot_bytes = NBT * nkb * 3 * 1024;
    char* my_ring = reinterpret_cast<char*>(ring) + (size_t)(dir * 2 + part) * 2 * slot_bytes;
    if (tid == 0) abort_flag = 0;

    gbf16x8 wq[3][KBW][3];                              // [gate][k block][plane]: row m = unit j0 + m, k = 32 kb + 8 q ..
    {
        const bool unit_ok = (j0 + m) < H;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float* row = w_hh + ((size_t)dir * 3 * H + (size_t)g * H + (unit_ok ? j0 + m : 0)) * H;
#pragma unroll
            for (int i = 0; i < KBW; ++i) {
                const int kb = wave + NWP * i;
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
                if (kb < nkb && unit_ok) {
                    lo = *reinterpret_cast<const f32x4*>(row + kb * 32 + q * 8);
                    hi = *reinterpret_cast<const f32x4*>(row + kb * 32 + q * 8 + 4);
                }
                unsigned int pl[3][4];
                split3(lo[0], lo[1], pl[0][0], pl[1][0], pl[2][0]);
                split3(lo[2], lo[3], pl[0][1], pl[1][1], pl[2][1]);
                split3(hi[0], hi[1], pl[0][2], pl[1][2], pl[2][2]);
                split3(hi[2], hi[3], pl[0][3], pl[1][3], pl[2][3]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const u32x4 v = {pl[c][0], pl[c][1], pl[c][2], pl[c][3]};
                    wq[g][i][c] = __builtin_bit_cast(gbf16x8, v);
                }
            }
        }
    }
    // gate role: unit jj, local batch row 16 gbt + nn  (512 threads = 16 units x 32 rows)
    const int jj = tid & 15, nn = (tid >> 4) & 15, gbt = tid >> 8;
    const int lb = gbt * 16 + nn, gb = b0 + lb, gj = j0 + jj;
    const bool gate_ok = (gbt < NBT) && (lb < nb) && (gj < H);
    float hp = 0.f;
    unsigned int* shards = &sync->arrive[dir][part][0][0];
    unsigned int* ctr = shards + (blockIdx.x % NSHARD) * 32;
    __syncthreads();

    // Round 4 (as in the 4x4x1 kernels): the gate pre-activations of step s + 1 are loaded at the END of step s, behind the
    // saved-activation stores, instead of at the top of step s + 1 in front of its hand-off loads (a wave's vector-memory
    // operations complete in issue order)
    float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f;
    auto load_gi = [&](int t) {
        if (gate_ok) {
            const size_t gb3 = (((size_t)t * B + gb) * 2 + dir) * 3 * H + gj;
            gi_r = G[gb3];
            gi_z = G[gb3 + H];
            gi_n = G[gb3 + 2 * H];
        }
    };
    load_gi(dir == 0 ? 0 : T - 1);
    for (int s = 0; s < T; ++s) {
        const int t = dir == 0 ? s : T - 1 - s;
        float sv_r = 0.f, sv_z = 0.f, sv_n = 0.f, sv_g = 0.f, sv_h = 0.f;
        const size_t gbase = (((size_t)t * B + gb) * 2 + dir) * 3 * H + gj;
        if (s > 0) {
            if (!DS2_DBG(dbg, 1) && wave == 0 && !wait_arrivals(shards, s, nslice, lane, &sync->error) && lane == 0)
                abort_flag = 1;
            __syncthreads();
            if (abort_flag) return;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                my_ring + (size_t)((s - 1) & 1) * slot_bytes, 0, slot_bytes, 0x00020000);
            if (!DS2_DBG(dbg, 2)) {
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) {
                    gbf16x8 bf[KBW][3];
#pragma unroll
                    for (int i = 0; i < KBW; ++i) {
                        const int kb = wave + NWP * i;                 // wave-uniform
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            bf[i][c] = __builtin_bit_cast(
                                gbf16x8, LOAD_HANDOFF(rsrc, (kb < nkb) ? ((bt * nkb + kb) * 3 + c) * 1024 + lane * 16 : OOB_OFFSET));
                    }
                    __builtin_amdgcn_sched_barrier(0);                 // all loads out before the MFMAs
                    f32x4 acc[3];
#pragma unroll
                    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < KBW; ++i) {
                        if (i == KBW - 1 && wave + NWP * i >= nkb) break;   // all-zero padded k block
#pragma unroll
                        for (int g = 0; g < 3; ++g) {
                            f32x4 a = acc[g];
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][1], bf[i][1], a, 0, 0, 0);
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][0], bf[i][2], a, 0, 0, 0);
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][2], bf[i][0], a, 0, 0, 0);
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][0], bf[i][1], a, 0, 0, 0);
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][1], bf[i][0], a, 0, 0, 0);
                            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[g][i][0], bf[i][0], a, 0, 0, 0);
                            acc[g] = a;
                        }
                    }
#pragma unroll
                    for (int g = 0; g < 3; ++g)
#pragma unroll
                        for (int r = 0; r < 4; ++r) red[wave][g][bt][4 * q + r][m] = acc[g][r];
                }
            }
        }
        __syncthreads();
        if (gate_ok) {
            float gh_r = 0.f, gh_z = 0.f, gh_n = 0.f;
            if (s > 0) {
#pragma unroll
                for (int w = 0; w < NWP; ++w) {
                    gh_r += red[w][0][gbt][jj][nn];
                    gh_z += red[w][1][gbt][jj][nn];
                    gh_n += red[w][2][gbt][jj][nn];
                }
            }
            const float r = fast_sigmoid(gi_r + gh_r);
            const float z = fast_sigmoid(gi_z + gh_z);
            const float n = fast_tanh(gi_n + r * gh_n);
            const float h = (1.f - z) * n + z * hp;
            hp = h;
            sv_h = h;
            sv_r = r;
            sv_z = z;
            sv_n = n;
            sv_g = gh_n;
        }
        {
            u32x4 planes[3];
            split_gather_octet(sv_h, planes);                          // (every lane: DPP needs the whole row active)
            if (gate_ok && (jj & 7) == 0) {
                const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(my_ring, 0, 2 * slot_bytes, 0x00020000);
                const int base = (s & 1) * slot_bytes + (gbt * nkb + (gj >> 5)) * 3 * 1024 + ((gj & 31) >> 3) * 256 + nn * 16;
#pragma unroll
                for (int c = 0; c < 3; ++c) store_sc1_b128(rs_w, base + c * 1024, planes[c]);
            }
        }
        if (!DS2_DBG(dbg, 4)) wait_vmcnt0();
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gate_ok) {
            hout[(((size_t)dir * T + t) * B + gb) * H + gj] = sv_h;
            G[gbase] = sv_r;
            G[gbase + H] = sv_z;
            G[gbase + 2 * H] = sv_n;
            ghn[(((size_t)t * B + gb) * 2 + dir) * H + gj] = sv_g;
        }
        if (s + 1 < T) load_gi(dir == 0 ? s + 1 : T - 2 - s);
    }
    if (tid == 0) leave_kernel(sync);
}
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_bwd_persistent_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                             const float* __restrict__ hout, const float* __restrict__ d_out,
                                             const float* __restrict__ w_hh_t, SyncWs* __restrict__ sync, float* __restrict__ ring,
                                             int T, int B, int H, int dbg) {
    bwd_recurrence<BwdWhole, NBT, KBW>(G, ghn, hout, d_out, w_hh_t, sync, ring, T, B, H, dbg);
}
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_bwd_persistent_p2_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                             const float* __restrict__ hout, const float* __restrict__ d_out,
                                             const float* __restrict__ w_hh_t, SyncWs* __restrict__ sync, float* __restrict__ ring,
                                             int T, int B, int H, int dbg) {
    bwd_recurrence<BwdP2, NBT, KBW>(G, ghn, hout, d_out, w_hh_t, sync, ring, T, B, H, dbg);
}
template <int NBT, int KBW>
__global__ __launch_bounds__(NWP * 64) void gru_bwd_persistent_p2b_kernel(float* __restrict__ G, float* __restrict__ ghn,
                                             const float* __restrict__ hout, const float* __restrict__ d_out,
                                             const float* __restrict__ w_hh_t, SyncWs* __restrict__ sync, float* __restrict__ ring,
                                             int T, int B, int H, int dbg) {
    bwd_recurrence<BwdP2b, NBT, KBW>(G, ghn, hout, d_out, w_hh_t, sync, ring, T, B, H, dbg);
}

}  // namespace

bool ds2_p16_launch_fwd(int form, int nbt, float* G, float* ghn, float* hout, const float* w_hh, void* sync_, float* ring, int T,
                        int B, int H, int dbg, hipStream_t st) {
    SyncWs* sync = (SyncWs*)sync_;
    const dim3 whole(ds2_cdiv(H, PJU), 2), halves(ds2_cdiv(H, 16), 2, 2);
    const int kbw = ds2_cdiv(H / 16, NWP), kbw_bf16 = ds2_cdiv(H / 32, NWP);
    auto go = [&](auto kernel, dim3 grid) { return launch_persistent(kernel, grid, 0, st, G, ghn, hout, w_hh, sync, ring, T, B, H, dbg); };
    if (form == 0)
        return with_kbw<1, 2, 4>(nbt, [&](auto N) {
            return with_kbw<1, 2, 4, 7>(kbw, [&](auto K) { return go(&gru_fwd_persistent_kernel<N, K>, whole); });
        });
    if (form == 1)
        return with_kbw<1, 2>(nbt, [&](auto N) {
            return with_kbw<1, 2, 4, 7>(kbw, [&](auto K) { return go(&gru_fwd_persistent_p2_kernel<N, K>, halves); });
        });
    return with_kbw<1, 2>(nbt, [&](auto N) {
        return with_kbw<1, 2, 4>(kbw_bf16, [&](auto K) { return go(&gru_fwd_persistent_p2b_kernel<N, K>, halves); });
    });
}

bool ds2_p16_launch_bwd(int form, int nbt, float* G, float* ghn, const float* hout, const float* d_out, const float* w_hh_t,
                        void* sync_, float* ring, int T, int B, int H, int dbg, hipStream_t st) {
    SyncWs* sync = (SyncWs*)sync_;
    const dim3 whole(ds2_cdiv(H, PJU), 2), halves(ds2_cdiv(H, 16), 2, 2);
    const int kbw = ds2_cdiv(3 * H / 16, NWP), kbw_bf16 = ds2_cdiv(3 * H / 32, NWP);
    auto go = [&](auto kernel, dim3 grid) {
        return launch_persistent(kernel, grid, 0, st, G, ghn, hout, d_out, w_hh_t, sync, ring, T, B, H, dbg);
    };
    if (form == 0)
        return with_kbw<1, 2, 4>(nbt, [&](auto N) {
            return with_kbw<1, 2, 4, 8, 19>(kbw, [&](auto K) { return go(&gru_bwd_persistent_kernel<N, K>, whole); });
        });
    if (form == 1)
        return with_kbw<1, 2>(nbt, [&](auto N) {
            return with_kbw<1, 2, 4, 8, 19>(kbw, [&](auto K) { return go(&gru_bwd_persistent_p2_kernel<N, K>, halves); });
        });
    return with_kbw<1, 2>(nbt, [&](auto N) {
        return with_kbw<1, 2, 5, 10>(kbw_bf16, [&](auto K) { return go(&gru_bwd_persistent_p2b_kernel<N, K>, halves); });
    });
}
