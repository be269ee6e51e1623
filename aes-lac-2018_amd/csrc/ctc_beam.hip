// Batched CTC prefix beam search on the device, with optional n-gram LM shallow fusion (ds2_ctc_beam_search_batch), and the
// same search with the output rows decoupled from the utterances, each row with its own LM weights (ds2_ctc_beam_search_rows:
// many (alpha, beta) pairs over one batch in one launch; DESIGN.md "LM weight tuning"), and the batch search with phrase
// boosting (ds2_ctc_beam_search_bias: a context graph over the boosted phrases adds w * V(prefix) to a prefix's rank;
// include/ds2hip.h and DESIGN.md "Phrase boosting"), and the batch search, boosted or not, that returns the N best entries
// of the final beam instead of one (ds2_ctc_beam_search_nbest; include/ds2hip.h and DESIGN.md "N-best lists").
// Not in the reference (its test.py offers greedy / none); the host search ds2_ctc_beam_search (decode_host.hip) is the
// no-LM yardstick and tests/beam_ref.py the pure-Python statement of the contract.  DESIGN.md "Device CTC beam search".
//
// One workgroup (256 threads) per utterance, no inter-workgroup communication.  Per frame:
//   1. the frame's A log-probs -> LDS (fp64, converted exactly as the host search does; the next row is prefetched);
//   2. merge lookup: beam j searches the beam for its parent prefix (hash + length); if the parent is slot i, j pulls the
//      extension (i, last(j)) into its own stay and that candidate is dropped from the new ones;
//   3. the W*A candidates (stay of i = index i*A+blank, extension of i by c = index i*A+c) are scored in fp64 and written
//      as order-preserving 64-bit keys into LDS (0 = no candidate);
//   4. exact top-W selection: an 8-pass radix select finds the W-th largest key; ties at that key go to the lower
//      candidate index, and the new beam is laid out in candidate-index order (two block scans), so the result does not
//      depend on thread count or timing;
//   5. every new beam entry is rebuilt from its parent slot by one thread; each selected extension appends a node
//      (parent node, symbol, frame) to the utterance's node array in the workspace.
// After the last frame the end-of-utterance LM terms are added, the best entry is picked (ties -> lower slot) and its
// node chain is followed back.  Merging compares 64-bit prefix hashes and lengths: two distinct prefixes of one beam
// with equal hash and length (probability ~ W^2 / 2^64 per frame) would be merged wrongly.
//
// Host half (from ds2_ctc_beam_ws_bytes down): each extern "C" entry makes its own checks, fills a BeamCall by field name
// and calls BeamCall::run(), which makes the checks all entries share and picks one of the five instantiations
// <ROWS, BIAS, NBEST> in one place; beam_launch<...> sets that kernel's LDS attribute and launches it.
#include "ds2_common.h"
#include "ds2_hash.h"

#pragma clang fp contract(off)     // the scores are compared with the host search's: no fused multiply-adds

namespace {

constexpr int BEAM_THREADS = 256;
constexpr int MAX_W = 128;
constexpr int MAX_A = 128;
constexpr int MAX_ORDER = 8;
constexpr int MAX_CTX = MAX_ORDER - 1;
constexpr double NEG_INF = -1e300;
constexpr uint64_t HASH_SEED = DS2_HASH_SEED;

struct BeamNode {      // one appended label on some lineage
    int parent, sym, frame;
};

struct LmArgs {
    const uint64_t* ngram;   // (ngram_cap, 2): key, (float ln p | float ln backoff << 32)
    const uint64_t* words;   // (word_cap, 2): key, word id
    int ngram_cap, word_cap, order, unit;   // unit: 0 = no LM, 1 = char, 2 = word
    int bos, eos, unk, space;
    double alpha, beta, oov;
};

__device__ inline double log_add(double x, double y) {
    if (x <= NEG_INF) return y;
    if (y <= NEG_INF) return x;
    const double m = x > y ? x : y;
    return m + log1p(exp(-fabs(x - y)));
}

// order-preserving map of a double onto uint64 (larger score -> larger key); every non-NaN score maps above 0
__device__ inline uint64_t score_key(double s) {
    const uint64_t u = (uint64_t)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// open-addressing probe; returns the entry's payload word or false
__device__ inline bool table_find(const uint64_t* tab, int cap, uint64_t key, uint64_t* val) {
    const uint32_t mask = (uint32_t)cap - 1;
    uint32_t i = (uint32_t)key & mask;
    for (int n = 0; n < cap; ++n) {
        const uint64_t k = tab[2 * (size_t)i];
        if (k == key) {
            *val = tab[2 * (size_t)i + 1];
            return true;
        }
        if (k == 0) return false;
        i = (i + 1) & mask;
    }
    return false;
}

__device__ inline float lo_f(uint64_t v) { return __uint_as_float((uint32_t)v); }
__device__ inline float hi_f(uint64_t v) { return __uint_as_float((uint32_t)(v >> 32)); }

// ln P(w | ctx[0..n)) by ARPA backoff (codes/lm.py NGramLM.log_prob_ids); *tok = the id w enters the history as
__device__ double lm_log_prob(const LmArgs& lm, const int* ctx, int n, int w, int* tok) {
    double acc = 0.0;
    if (w >= 0) {
        for (int k = n; k >= 0; --k) {
            uint64_t h = HASH_SEED;
#pragma unroll
            for (int q = 0; q < MAX_CTX; ++q)      // constant indices keep ctx[] in registers
                if (q >= n - k && q < n) h = ds2_hash_step(h, ctx[q]);
            uint64_t v;
            if (table_find(lm.ngram, lm.ngram_cap, ds2_hash_key(ds2_hash_step(h, w)), &v)) {
                *tok = w;
                return acc + (double)lo_f(v);
            }
            if (k > 0 && table_find(lm.ngram, lm.ngram_cap, ds2_hash_key(h), &v)) acc += (double)hi_f(v);
        }
    }
    *tok = lm.unk;
    return lm.oov;
}

// append tok to the history ctx[0..n), keeping the last cap = order-1 tokens; returns the new length
__device__ inline int ctx_push(int* ctx, int n, int cap, int tok) {
    if (cap == 0) return 0;
    const bool full = n == cap;
#pragma unroll
    for (int q = 0; q < MAX_CTX; ++q) {
        if (full && q + 1 < n) ctx[q] = ctx[q + 1];
        if (q == (full ? n - 1 : n)) ctx[q] = tok;
    }
    return full ? n : n + 1;
}

// the word spelled by a partial-word hash -> word id, or -1 (OOV)
__device__ inline int word_lookup(const LmArgs& lm, uint64_t whash) {
    uint64_t v;
    return table_find(lm.words, lm.word_cap, ds2_hash_key(whash), &v) ? (int)(uint32_t)v : -1;
}

// LM part of appending c: returns alpha * ln p + beta (or 0) and updates ctx / n / whash / wlen in place
__device__ double lm_delta(const LmArgs& lm, int c, int* ctx, int* n, uint64_t* whash, int* wlen) {
    const int cap = lm.order - 1;
    int tok;
    if (lm.unit == 1) {
        const double lp = lm_log_prob(lm, ctx, *n, c, &tok);
        *n = ctx_push(ctx, *n, cap, tok);
        return lm.alpha * lp + lm.beta;
    }
    if (c != lm.space) {
        *whash = ds2_hash_step(*whash, c);
        *wlen += 1;
        return 0.0;
    }
    if (*wlen == 0) return 0.0;
    const double lp = lm_log_prob(lm, ctx, *n, word_lookup(lm, *whash), &tok);
    *n = ctx_push(ctx, *n, cap, tok);
    *whash = HASH_SEED;
    *wlen = 0;
    return lm.alpha * lp + lm.beta;
}

// phrase boosting: the context graph's tables (include/ds2hip.h "phrase boosting")
struct BiasArgs {
    const int32_t* trans;    // (states, A): next state | gain << 16; the blank column is never read
    const int32_t* fin;      // (states): F(path(s)) - depth(s)
    int states;
    double weight;           // nats per matched label
};

// one step of the scan automaton: appending c in state *state; a next state outside [0, states) is taken as the root
__device__ inline void bias_step(const BiasArgs& bias, int A, int c, int* state, int* count) {
    const int32_t v = bias.trans[(size_t)*state * A + c];
    const int next = v & 0xFFFF;
    *state = next < bias.states ? next : 0;
    *count += v >> 16;
}

struct BeamLds {
    double lp[MAX_A];
    double pb[MAX_W], pnb[MAX_W], tot[MAX_W], acc[MAX_W];   // acc = alpha * LM + beta * N so far
    uint64_t hash[MAX_W], phash[MAX_W], whash[MAX_W];
    int len[MAX_W], last[MAX_W], node[MAX_W], wlen[MAX_W], pslot[MAX_W], nctx[MAX_W];
    int ctx[MAX_W][MAX_CTX];
    int sel[MAX_W], sel_node[MAX_W];   // selected candidate per new slot; its node id if it is an extension
    unsigned hist[256];
    int wave_tot[BEAM_THREADS / 64];
    uint64_t digit;
    int need;
};

// block-wide exclusive scan of one int per thread (all 256 threads call it)
__device__ inline int block_exscan(int v, int* total, BeamLds& s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s.wave_tot[wave] = x;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BEAM_THREADS / 64; ++w) {
        const int t = s.wave_tot[w];
        if (w < wave) base += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return base + x - v;
}

// stay candidate of slot i (with the merge pull from its parent slot): host search semantics
__device__ inline void stay_scores(const BeamLds& s, int i, int blank, double* npb, double* npnb) {
    const int last = s.last[i];
    *npb = log_add(NEG_INF, s.tot[i] + s.lp[blank]);
    double q = last >= 0 ? log_add(NEG_INF, s.pnb[i] + s.lp[last]) : NEG_INF;
    const int p = s.pslot[i];
    if (p >= 0 && s.lp[last] > NEG_INF) {
        const double from = (last == s.last[p]) ? s.pb[p] : s.tot[p];
        if (from > NEG_INF) q = log_add(q, from + s.lp[last]);
    }
    *npnb = q;
}

// The end of ds2_ctc_beam_search_nbest, called by all 256 threads after the last frame with s.pb[i] = the end-adjusted score
// of slot i < nb (and bcount[i] = count + final[state] where bcount is given).  A function of its own, not inlined, so
// that the frame loop of the NBEST instantiations is compiled as that of the 1-best ones.
// Ranking by counting: thread i < nb compares its score with all others in LDS; s.sel (free after the last frame) maps
// rank -> slot, -1 where fewer than nbest entries are valid.  The valid entries' ranks are 0 .. valid-1, each once, so rows
// [0, count) have a slot and the rest have none.
__device__ __noinline__ void nbest_end(BeamLds& s, const int* bcount, int nb, int nbest, int b, int T, const BeamNode* nodes,
                                       int32_t* out_labels, int32_t* out_offsets, int32_t* out_len, float* out_score,
                                       float* out_ctc, int32_t* out_bias, int32_t* out_count) {
    const int tid = threadIdx.x;
    if (tid < nbest) s.sel[tid] = -1;
    __syncthreads();
    int rank = -1;
    if (tid < nb) {
        const double v = s.pb[tid];
        if (v > NEG_INF) {          // what the single pick can choose; false for a NaN
            rank = 0;
            for (int j = 0; j < nb; ++j) {
                const double o = s.pb[j];
                rank += (o > v) || (o == v && j < tid);
            }
            if (rank < nbest) s.sel[rank] = tid;
        }
    }
    __syncthreads();
    if (tid < nbest) {
        const size_t row = (size_t)b * nbest + tid;
        const int slot = s.sel[tid];
        if (slot < 0) {
            out_len[row] = 0;
            out_score[row] = (float)NEG_INF;
            out_ctc[row] = (float)NEG_INF;
            if (bcount) out_bias[row] = 0;
        }
        if (slot >= 0 ? (tid + 1 == nbest || s.sel[tid + 1] < 0) : tid == 0) out_count[b] = slot >= 0 ? tid + 1 : 0;
    }
    if (rank >= 0 && rank < nbest) {      // up to 128 chains at once (two waves), each followed by the thread that owns the slot
        const size_t row = (size_t)b * nbest + rank;
        const int len = s.len[tid];
        int nd = s.node[tid];
        for (int q = len - 1; q >= 0; --q) {
            const BeamNode e = nodes[nd];
            out_labels[row * T + q] = e.sym;
            out_offsets[row * T + q] = e.frame;
            nd = e.parent;
        }
        out_len[row] = len;
        out_score[row] = (float)s.pb[tid];
        out_ctc[row] = (float)s.tot[tid];
        if (bcount) out_bias[row] = bcount[tid];
    }
    for (int r = 0; r < nbest; ++r) {     // zeros past every row's length, by the whole workgroup
        const size_t row = (size_t)b * nbest + r;
        const int slot = s.sel[r];
        for (int q = (slot >= 0 ? s.len[slot] : 0) + tid; q < T; q += BEAM_THREADS) {
            out_labels[row * T + q] = 0;
            out_offsets[row * T + q] = 0;
        }
    }
}

// ROWS = false: workgroup b decodes utterance b with the weights in lm_in (ds2_ctc_beam_search_batch).
// ROWS = true: workgroup r decodes utterance utt[r] with alpha_r[r] / beta_r[r] into output row r and node array r
// (ds2_ctc_beam_search_rows); everything after these first lines is the same code for both.
// BIAS = true (ds2_ctc_beam_search_bias): every beam entry also carries the context graph's (state, count) of its prefix,
// both functions of the prefix alone, and w * (double)count joins its rank after log p + acc; at the end of the utterance
// count + final[state] takes the place of count.  With BIAS = false none of this is compiled in.
// NBEST = true (ds2_ctc_beam_search_nbest): the same frames; after the last one the valid entries of the final beam are
// ranked by counting (higher end-adjusted score first, an exact tie to the lower slot) and the entry of rank n < nbest
// follows its own node chain back into output row b * nbest + n.  With NBEST = false nbest and out_count are not read and
// the end is the single pick below.
template <bool ROWS, bool BIAS, bool NBEST = false>
__global__ void __launch_bounds__(BEAM_THREADS)
ctc_beam_kernel(const float* __restrict__ probs, const int32_t* __restrict__ sizes, int B, int T, int A, int blank, int W,
                int log_input, LmArgs lm_in, const int32_t* __restrict__ utt, const float* __restrict__ alpha_r,
                const float* __restrict__ beta_r, BeamNode* __restrict__ nodes_all, int32_t* __restrict__ out_labels,
                int32_t* __restrict__ out_offsets, int32_t* __restrict__ out_len, float* __restrict__ out_score,
                float* __restrict__ out_ctc, BiasArgs bias, int32_t* __restrict__ out_bias, int nbest,
                int32_t* __restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];   // W * A candidate keys
    __shared__ BeamLds s;
    __shared__ int bstate[BIAS ? MAX_W : 1], bcount[BIAS ? MAX_W : 1];   // the context graph's state and V of each slot
    const int b = blockIdx.x, tid = threadIdx.x;      // b: the output row (and the node array); u: the utterance it decodes
    int u = b;
    LmArgs lm = lm_in;
    if (ROWS) {
        u = utt[b];
        if (u < 0 || u >= B) {      // no utterance: the empty labelling at -inf, nothing of probs or sizes is read
            if (tid == 0) {
                out_len[b] = 0;
                out_score[b] = (float)NEG_INF;
                out_ctc[b] = (float)NEG_INF;
            }
            for (int q = tid; q < T; q += BEAM_THREADS) {
                out_labels[(size_t)b * T + q] = 0;
                out_offsets[(size_t)b * T + q] = 0;
            }
            return;
        }
        if (lm.unit) {              // float -> double once, as the batch entry converts its two scalars
            lm.alpha = (double)alpha_r[b];
            lm.beta = (double)beta_r[b];
        }
    }
    const int n = min(max(sizes[u], 0), T);
    const float* pr = probs + (size_t)u * T * A;
    BeamNode* nodes = nodes_all + (size_t)b * (1 + (size_t)T * W);
    const int NC = W * A;
    const int chunk = (NC + BEAM_THREADS - 1) / BEAM_THREADS;   // contiguous candidate range per thread (scans)
    const int ctx_cap = lm.unit ? lm.order - 1 : 0;

    if (tid == 0) {
        s.pb[0] = 0.0;
        s.pnb[0] = NEG_INF;
        s.tot[0] = 0.0;
        s.acc[0] = 0.0;
        s.hash[0] = HASH_SEED;
        s.phash[0] = 0;
        s.whash[0] = HASH_SEED;
        s.len[0] = 0;
        s.last[0] = -1;
        s.node[0] = 0;
        s.wlen[0] = 0;
        s.nctx[0] = ctx_push(s.ctx[0], 0, ctx_cap, lm.bos);
        if (BIAS) {
            bstate[0] = 0;
            bcount[0] = 0;
        }
        nodes[0] = BeamNode{-1, -1, 0};
    }
    int nb = 1, node_count = 1;
    float next_v = (tid < A && n > 0) ? pr[tid] : 0.f;
    __syncthreads();

    for (int t = 0; t < n; ++t) {
        // 1. frame log-probs
        if (tid < A) {
            const double v = next_v;
            s.lp[tid] = log_input ? v : (v > 0.0 ? log(v) : NEG_INF);
            if (t + 1 < n) next_v = pr[(size_t)(t + 1) * A + tid];
        }
        // 2. merge lookup: one wave per beam entry j, lanes scan the slots
        {
            const int lane = tid & 63;
            for (int j = tid >> 6; j < nb; j += BEAM_THREADS / 64) {
                int found = -1;
                if (s.len[j] > 0) {
                    for (int base = 0; base < nb && found < 0; base += 64) {
                        const int i = base + lane;
                        const bool hit = i < nb && s.len[i] == s.len[j] - 1 && s.hash[i] == s.phash[j];
                        const uint64_t m = __ballot(hit);
                        if (m) found = base + __ffsll((unsigned long long)m) - 1;
                    }
                }
                if (lane == 0) s.pslot[j] = found;
            }
        }
        __syncthreads();
        // 3. candidate keys
        for (int k = tid; k < NC; k += BEAM_THREADS) {
            const int i = k / A, c = k - i * A;
            uint64_t key = 0;
            if (i < nb) {
                if (c == blank) {
                    double npb, npnb;
                    stay_scores(s, i, blank, &npb, &npnb);
                    double v = log_add(npb, npnb) + s.acc[i];
                    if (BIAS) v = v + bias.weight * (double)bcount[i];
                    key = score_key(v);
                } else if (s.lp[c] > NEG_INF) {
                    const double from = (c == s.last[i]) ? s.pb[i] : s.tot[i];
                    if (from > NEG_INF) {
                        double acc = s.acc[i];
                        if (lm.unit) {
                            int ctx[MAX_CTX];
                            int nctx = s.nctx[i], wl = s.wlen[i];
                            uint64_t wh = s.whash[i];
                #pragma unroll
                            for (int q = 0; q < MAX_CTX; ++q) ctx[q] = s.ctx[i][q];
                            acc = acc + lm_delta(lm, c, ctx, &nctx, &wh, &wl);
                        }
                        double v = log_add(NEG_INF, from + s.lp[c]) + acc;
                        if (BIAS) {
                            int st = bstate[i], cnt = bcount[i];
                            bias_step(bias, A, c, &st, &cnt);
                            v = v + bias.weight * (double)cnt;
                        }
                        key = score_key(v);
                    }
                }
            }
            keys[k] = key;
        }
        __syncthreads();
        for (int j = tid; j < nb; j += BEAM_THREADS)         // extensions merged into a stay are no candidates
            if (s.pslot[j] >= 0) keys[s.pslot[j] * A + s.last[j]] = 0;
        __syncthreads();

        // 4. radix select of the keep-th largest key, keep = min(W, number of candidates)
        uint64_t prefix = 0, mask = 0;
        for (int shift = 56; shift >= 0; shift -= 8) {
            s.hist[tid] = 0;
            __syncthreads();
            for (int k = tid; k < nb * A; k += BEAM_THREADS) {
                const uint64_t key = keys[k];
                if (key != 0 && (key & mask) == prefix) atomicAdd(&s.hist[(key >> shift) & 255], 1u);
            }
            __syncthreads();
            if (tid < 64) {        // wave 0: bins in descending digit order, lane l owns digits 255-4l .. 252-4l
                unsigned c4[4], sum = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c4[q] = s.hist[255 - 4 * tid - q];
                    sum += c4[q];
                }
                unsigned incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned y = __shfl_up(incl, o, 64);
                    if (tid >= o) incl += y;
                }
                const int need = (shift == 56) ? min(W, (int)__shfl(incl, 63, 64)) : s.need;
                const uint64_t m = __ballot(incl >= (unsigned)need);
                const int l = __ffsll((unsigned long long)m) - 1;
                if (tid == l) {
                    unsigned before = incl - sum;
                    int q = 0;
                    while (before + c4[q] < (unsigned)need) before += c4[q++];
                    s.need = need - (int)before;
                    s.digit = (uint64_t)(255 - 4 * l - q);
                }
            }
            __syncthreads();
            prefix |= s.digit << shift;
            mask |= 0xFFull << shift;
            __syncthreads();
        }
        const uint64_t tau = prefix;    // the keep-th largest key
        const int need_eq = s.need;     // how many keys equal to tau are kept: the ones with the lowest indices
        // 5. new slots in candidate-index order: thread tid owns candidates [k0, k1)
        const int k0 = tid * chunk, k1 = min(k0 + chunk, nb * A);
        int eq = 0;
        for (int k = k0; k < k1; ++k) eq += keys[k] == tau;
        int unused;
        const int eq_base = block_exscan(eq, &unused, s);
        int nsel = 0, next = 0;
        for (int k = k0, e = eq_base; k < k1; ++k) {
            const uint64_t key = keys[k];
            if (key > tau || (key == tau && e++ < need_eq)) {
                nsel += 1;
                next += (k % A) != blank;
            }
        }
        int all;
        const int packed = block_exscan(nsel | (next << 16), &all, s);   // counts <= W*A < 2^16
        for (int k = k0, e = eq_base, slot = packed & 0xFFFF, nid = node_count + (packed >> 16); k < k1; ++k) {
            const uint64_t key = keys[k];
            if (key > tau || (key == tau && e++ < need_eq)) {
                s.sel[slot] = k;
                s.sel_node[slot++] = (k % A) != blank ? nid++ : -1;
            }
        }
        __syncthreads();
        const int keep = all & 0xFFFF, new_nodes = all >> 16;
        // rebuild the beam: thread k owns new slot k
        double r_pb = 0, r_pnb = 0, r_acc = 0;
        uint64_t r_hash = 0, r_phash = 0, r_whash = 0;
        int r_len = 0, r_last = 0, r_node = 0, r_wlen = 0, r_nctx = 0;
        int r_ctx[MAX_CTX];
        int r_bstate = 0, r_bcount = 0;
        if (tid < keep) {
            const int k = s.sel[tid], i = k / A, c = k - i * A;
            if (BIAS) {
                r_bstate = bstate[i];
                r_bcount = bcount[i];
            }
            r_acc = s.acc[i];
            r_hash = s.hash[i];
            r_phash = s.phash[i];
            r_whash = s.whash[i];
            r_len = s.len[i];
            r_last = s.last[i];
            r_node = s.node[i];
            r_wlen = s.wlen[i];
            r_nctx = s.nctx[i];
#pragma unroll
            for (int q = 0; q < MAX_CTX; ++q) r_ctx[q] = s.ctx[i][q];
            if (c == blank) {
                stay_scores(s, i, blank, &r_pb, &r_pnb);
            } else {
                const double from = (c == s.last[i]) ? s.pb[i] : s.tot[i];
                r_pb = NEG_INF;
                r_pnb = log_add(NEG_INF, from + s.lp[c]);
                if (lm.unit) r_acc = r_acc + lm_delta(lm, c, r_ctx, &r_nctx, &r_whash, &r_wlen);
                if (BIAS) bias_step(bias, A, c, &r_bstate, &r_bcount);
                r_phash = r_hash;
                r_hash = ds2_hash_step(r_hash, c);
                r_len += 1;
                r_last = c;
                r_node = s.sel_node[tid];      // extensions are numbered in candidate-index order
                nodes[r_node] = BeamNode{s.node[i], c, t};
            }
        }
        __syncthreads();
        if (tid < keep) {
            s.pb[tid] = r_pb;
            s.pnb[tid] = r_pnb;
            s.tot[tid] = log_add(r_pb, r_pnb);
            s.acc[tid] = r_acc;
            s.hash[tid] = r_hash;
            s.phash[tid] = r_phash;
            s.whash[tid] = r_whash;
            s.len[tid] = r_len;
            s.last[tid] = r_last;
            s.node[tid] = r_node;
            s.wlen[tid] = r_wlen;
            s.nctx[tid] = r_nctx;
#pragma unroll
            for (int q = 0; q < MAX_CTX; ++q) s.ctx[tid][q] = r_ctx[q];
            if (BIAS) {
                bstate[tid] = r_bstate;
                bcount[tid] = r_bcount;
            }
        }
        nb = keep;
        node_count += new_nodes;
        __syncthreads();
    }

    // end of utterance: LM end terms, best entry (ties -> lower slot), traceback
    if (tid < nb) {
        double e = s.acc[tid];
        if (lm.unit) {
            int ctx[MAX_CTX];
            int nctx = s.nctx[tid], wl = s.wlen[tid];
            uint64_t wh = s.whash[tid];
#pragma unroll
            for (int q = 0; q < MAX_CTX; ++q) ctx[q] = s.ctx[tid][q];
            if (lm.unit == 2 && wl > 0) e = e + lm_delta(lm, lm.space, ctx, &nctx, &wh, &wl);
            int tok;
            e = e + lm.alpha * lm_log_prob(lm, ctx, nctx, lm.eos, &tok);
        }
        if (BIAS) {      // F = count + final[state]: what the prefix keeps once nothing can complete a pending phrase
            bcount[tid] += bias.fin[bstate[tid]];
            e = e + bias.weight * (double)bcount[tid];
        }
        s.pb[tid] = s.tot[tid] + e;     // reuse: end-adjusted score
    }
    __syncthreads();
    if (NBEST) {
        nbest_end(s, BIAS ? bcount : nullptr, nb, nbest, b, T, nodes, out_labels, out_offsets, out_len, out_score, out_ctc,
                  out_bias, out_count);
        return;
    }
    if (tid == 0) {
        int best = -1;
        double best_v = NEG_INF;
        for (int i = 0; i < nb; ++i)
            if (s.pb[i] > best_v) {
                best_v = s.pb[i];
                best = i;
            }
        int len = 0;
        if (best >= 0) {
            len = s.len[best];
            int nd = s.node[best];
            for (int q = len - 1; q >= 0; --q) {
                const BeamNode e = nodes[nd];
                out_labels[(size_t)b * T + q] = e.sym;
                out_offsets[(size_t)b * T + q] = e.frame;
                nd = e.parent;
            }
        }
        out_len[b] = len;
        out_score[b] = best >= 0 ? (float)best_v : (float)NEG_INF;
        out_ctc[b] = best >= 0 ? (float)s.tot[best] : (float)NEG_INF;
        if (BIAS) out_bias[b] = best >= 0 ? bcount[best] : 0;
        s.need = len;
    }
    __syncthreads();
    for (int q = s.need + tid; q < T; q += BEAM_THREADS) {
        out_labels[(size_t)b * T + q] = 0;
        out_offsets[(size_t)b * T + q] = 0;
    }
}

}  // namespace

extern "C" size_t ds2_ctc_beam_ws_bytes(int B, int T, int W) {
    if (B < 0 || T < 0 || W < 1) return 0;
    return (size_t)B * (1 + (size_t)T * W) * sizeof(BeamNode);
}

namespace {

#define BEAM_CHECK_ARG(cond)                                          \
    do {                                                              \
        if (!(cond)) {                                                \
            ds2_set_error("%s: bad argument: %s", fn, #cond);         \
            return DS2_ERR_ARG;                                       \
        }                                                             \
    } while (0)

// the 13 LM values every entry receives, in the ABI's order and under its names (the refusal messages quote them): an
// entry hands them over as one braced list
struct BeamLm {
    const void* ngram_table;
    int ngram_cap;
    const void* word_table;
    int word_cap, order, unit, bos_id, eos_id, unk_id, space_id;
    float alpha, beta, oov_logp;      // _rows has no scalar weights: it gives 0, 0
};

// One search as its entry point received it (host only): the entry makes its own checks, fills what it has by name --
// the rest stays zero -- and calls run().
struct BeamCall {
    const char* fn;                   // the entry's name, for messages
    const float* probs;
    const int32_t* sizes;
    int B, R, T, A, blank, beam_width, log_input;   // R workgroups: B but for _rows
    BeamLm lm;                        // as given, unchecked
    const int32_t* utt;               // _rows only: the utterance and the LM weights of each row
    const float *alpha_r, *beta_r;
    void* ws;
    size_t ws_bytes;
    int32_t *out_labels, *out_offsets, *out_len;
    float *out_score, *out_ctc_logp;
    BiasArgs bias;                    // phrase boosting if bias.trans, set with out_bias by check_bias
    int32_t* out_bias;
    int nbest;                        // > 0: the outputs have nbest rows per utterance (batch form only)
    int32_t* out_count;
    void* stream;

    int run() const;                  // the checks all entries share, then the launch
};

// the context-graph arguments of _bias and _nbest -> c.bias and c.out_bias, or false with the error set (DS2_ERR_ARG);
// null_text is the entry's wording
bool check_bias(BeamCall& c, const char* null_text, const int32_t* bias_trans, const int32_t* bias_final, int bias_states,
                float bias_weight, int32_t* out_bias) {
    if (bias_states < 1 || bias_states > DS2_BIAS_MAX_STATES) {
        ds2_set_error("%s: %d context-graph states are outside 1..%d", c.fn, bias_states, DS2_BIAS_MAX_STATES);
        return false;
    }
    if (!(bias_weight - bias_weight == 0.f)) {
        ds2_set_error("%s: the weight %g is not finite", c.fn, (double)bias_weight);
        return false;
    }
    if (!bias_trans || !bias_final || !out_bias) {
        ds2_set_error("%s: %s", c.fn, null_text);
        return false;
    }
    c.bias = BiasArgs{bias_trans, bias_final, bias_states, (double)bias_weight};
    c.out_bias = out_bias;
    return true;
}

// one instantiation: the kernel whose LDS attribute is raised is by construction the kernel that is launched
template <bool ROWS, bool BIAS, bool NBEST>
int beam_launch(const BeamCall& c, const LmArgs& lm) {
    const auto kern = &ctc_beam_kernel<ROWS, BIAS, NBEST>;
    const size_t dyn = (size_t)c.beam_width * c.A * sizeof(uint64_t);
    const size_t fixed = sizeof(BeamLds) + (BIAS ? 2 * MAX_W * sizeof(int) : 0);
    if (dyn + fixed > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
        ds2_set_error("%s: %zu bytes of LDS are not available", c.fn, dyn + fixed);
        return DS2_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(c.R), dim3(BEAM_THREADS), dyn, (hipStream_t)c.stream, c.probs, c.sizes, c.B, c.T, c.A,
                       c.blank, c.beam_width, c.log_input, lm, c.utt, c.alpha_r, c.beta_r, (BeamNode*)c.ws, c.out_labels,
                       c.out_offsets, c.out_len, c.out_score, c.out_ctc_logp, BIAS ? c.bias : BiasArgs{},
                       BIAS ? c.out_bias : nullptr, NBEST ? c.nbest : 0, NBEST ? c.out_count : nullptr);
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) {
        ds2_set_error("%s: launch failed: %s", c.fn, hipGetErrorString(e_));
        return DS2_ERR_LAUNCH;
    }
    return DS2_OK;
}

int BeamCall::run() const {
    const auto& [ngram_table, ngram_cap, word_table, word_cap, order, unit, bos_id, eos_id, unk_id, space_id, alpha, beta,
                 oov_logp] = lm;
    if (beam_width < 1 || beam_width > MAX_W) {
        ds2_set_error("%s: beam_width %d is outside 1..%d", fn, beam_width, MAX_W);
        return DS2_ERR_ARG;
    }
    if (A < 1 || A > MAX_A) {
        ds2_set_error("%s: alphabet size %d is outside 1..%d", fn, A, MAX_A);
        return DS2_ERR_ARG;
    }
    BEAM_CHECK_ARG(B >= 0 && R >= 0 && T >= 0 && blank >= 0 && blank < A && unit >= 0 && unit <= 2);
    BEAM_CHECK_ARG(sizes && out_labels && out_offsets && out_len && out_score && out_ctc_logp && (probs || T == 0 || B == 0));
    if (unit) {
        if (order < 1 || order > MAX_ORDER) {
            ds2_set_error("%s: LM order %d is outside 1..%d", fn, order, MAX_ORDER);
            return DS2_ERR_ARG;
        }
        BEAM_CHECK_ARG(ngram_table && ngram_cap >= 2 && (ngram_cap & (ngram_cap - 1)) == 0);
        BEAM_CHECK_ARG(unit == 1 || (word_table && word_cap >= 2 && (word_cap & (word_cap - 1)) == 0 && space_id < A));
    }
    if (ws_bytes < ds2_ctc_beam_ws_bytes(R, T, beam_width) || (!ws && R > 0)) {
        ds2_set_error("%s: workspace of %zu bytes < ds2_ctc_beam_ws_bytes = %zu", fn, ws_bytes,
                      ds2_ctc_beam_ws_bytes(R, T, beam_width));
        return DS2_ERR_ARG;
    }
    if (R == 0) return DS2_OK;
    LmArgs dev{};
    dev.ngram = (const uint64_t*)ngram_table;
    dev.words = (const uint64_t*)word_table;
    dev.ngram_cap = ngram_cap;
    dev.word_cap = word_cap;
    dev.order = unit ? order : 1;
    dev.unit = unit;
    dev.bos = bos_id;
    dev.eos = eos_id;
    dev.unk = unk_id;
    dev.space = unit == 2 ? space_id : -1;
    dev.alpha = unit ? (double)alpha : 0.0;
    dev.beta = unit ? (double)beta : 0.0;
    dev.oov = (double)oov_logp;
    // the five instantiations <ROWS, BIAS, NBEST>: boosting and N-best exist in the batch form only
    if (nbest) return bias.trans ? beam_launch<false, true, true>(*this, dev) : beam_launch<false, false, true>(*this, dev);
    if (bias.trans) return beam_launch<false, true, false>(*this, dev);
    return utt ? beam_launch<true, false, false>(*this, dev) : beam_launch<false, false, false>(*this, dev);
}

// what every entry receives under the same names; R = B until _rows says otherwise
#define BEAM_CALL(c, name)                                                                                          \
    BeamCall c{};                                                                                                   \
    c.fn = name; c.probs = probs; c.sizes = sizes; c.B = c.R = B; c.T = T; c.A = A; c.blank = blank;                \
    c.beam_width = beam_width; c.log_input = log_input; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;        \
    c.out_labels = out_labels; c.out_offsets = out_offsets; c.out_len = out_len; c.out_score = out_score;           \
    c.out_ctc_logp = out_ctc_logp

}  // namespace

extern "C" int ds2_ctc_beam_search_batch(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                                         int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                                         const void* word_table, int word_cap, int order, int unit, int bos_id,
                                         int eos_id, int unk_id, int space_id, float alpha, float beta, float oov_logp,
                                         void* ws, size_t ws_bytes, int32_t* out_labels, int32_t* out_offsets,
                                         int32_t* out_len, float* out_score, float* out_ctc_logp, void* stream) {
    BEAM_CALL(c, "ds2_ctc_beam_search_batch");
    c.lm = {ngram_table, ngram_cap, word_table, word_cap, order, unit, bos_id, eos_id, unk_id, space_id, alpha, beta, oov_logp};
    return c.run();
}

extern "C" int ds2_ctc_beam_search_rows(const float* probs, const int32_t* sizes, const int32_t* utt, const float* alpha,
                                        const float* beta, int B, int R, int T, int A, int blank, int beam_width,
                                        int log_input, const void* ngram_table, int ngram_cap, const void* word_table,
                                        int word_cap, int order, int unit, int bos_id, int eos_id, int unk_id, int space_id,
                                        float oov_logp, void* ws, size_t ws_bytes, int32_t* out_labels,
                                        int32_t* out_offsets, int32_t* out_len, float* out_score, float* out_ctc_logp,
                                        void* stream) {
    if (R < 0) {
        ds2_set_error("ds2_ctc_beam_search_rows: %d rows", R);
        return DS2_ERR_ARG;
    }
    if (R == 0) return DS2_OK;       // no rows: nothing to check, nothing is launched
    if (!utt || (unit && (!alpha || !beta))) {
        ds2_set_error("ds2_ctc_beam_search_rows: utt%s must not be NULL", unit ? ", alpha and beta" : "");
        return DS2_ERR_ARG;
    }
    BEAM_CALL(c, "ds2_ctc_beam_search_rows");
    c.R = R;
    c.utt = utt;
    c.alpha_r = alpha;
    c.beta_r = beta;
    c.lm = {ngram_table, ngram_cap, word_table, word_cap, order, unit, bos_id, eos_id, unk_id, space_id, 0.f, 0.f, oov_logp};
    return c.run();
}

extern "C" int ds2_ctc_beam_search_bias(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                                        int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                                        const void* word_table, int word_cap, int order, int unit, int bos_id, int eos_id,
                                        int unk_id, int space_id, float alpha, float beta, float oov_logp,
                                        const int32_t* bias_trans, const int32_t* bias_final, int bias_states,
                                        float bias_weight, void* ws, size_t ws_bytes, int32_t* out_labels,
                                        int32_t* out_offsets, int32_t* out_len, float* out_score, float* out_ctc_logp,
                                        int32_t* out_bias, void* stream) {
    BEAM_CALL(c, "ds2_ctc_beam_search_bias");
    if (!check_bias(c, "bias_trans, bias_final and out_bias must not be NULL", bias_trans, bias_final, bias_states,
                    bias_weight, out_bias))
        return DS2_ERR_ARG;
    c.lm = {ngram_table, ngram_cap, word_table, word_cap, order, unit, bos_id, eos_id, unk_id, space_id, alpha, beta, oov_logp};
    return c.run();
}

extern "C" int ds2_ctc_beam_search_nbest(const float* probs, const int32_t* sizes, int B, int T, int A, int blank,
                                         int beam_width, int log_input, const void* ngram_table, int ngram_cap,
                                         const void* word_table, int word_cap, int order, int unit, int bos_id, int eos_id,
                                         int unk_id, int space_id, float alpha, float beta, float oov_logp,
                                         const int32_t* bias_trans, const int32_t* bias_final, int bias_states,
                                         float bias_weight, int nbest, void* ws, size_t ws_bytes, int32_t* out_labels,
                                         int32_t* out_offsets, int32_t* out_len, float* out_score, float* out_ctc_logp,
                                         int32_t* out_bias, int32_t* out_count, void* stream) {
    BEAM_CALL(c, "ds2_ctc_beam_search_nbest");
    if (nbest < 1 || nbest > beam_width) {
        ds2_set_error("%s: nbest %d is outside 1..beam_width = %d", c.fn, nbest, beam_width);
        return DS2_ERR_ARG;
    }
    if (!out_count) {
        ds2_set_error("%s: out_count must not be NULL", c.fn);
        return DS2_ERR_ARG;
    }
    c.nbest = nbest;
    c.out_count = out_count;
    // without bias_trans there is no boosting: the other bias arguments and out_bias are ignored
    if (bias_trans && !check_bias(c, "with bias_trans, bias_final and out_bias must not be NULL", bias_trans, bias_final,
                                  bias_states, bias_weight, out_bias))
        return DS2_ERR_ARG;
    c.lm = {ngram_table, ngram_cap, word_table, word_cap, order, unit, bos_id, eos_id, unk_id, space_id, alpha, beta, oov_logp};
    return c.run();
}
