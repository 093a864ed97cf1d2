// Device primitives shared by the dynamic decode (kernels_sampling.hip) and beam search (kernels_beam.hip): the {value, id}
// arg-best with its tie rule, the workgroup max / sum through an LDS array, the optional-last-tokens mask -- by those two and the
// close of a verify pass (kernels_verify.hip): the stop-word rule, the merge of a row's partials -- and by the dynamic
// decode and the sampled tail of a verify pass: the counter-based uniform number, a vocabulary slice in
// registers (load, soft-max statistics, the radix select of its k best), the merge of the slices' candidate sets and the top-k
// layer's draw.
#pragma once
#include "ftcf_common.h"

namespace ftcf {

struct VI {
    float v;
    int   i;
};
__device__ __forceinline__ bool better(float v, int i, float bv, int bi)
{
    return (v > bv) || (v == bv && i < bi);
}
__device__ __forceinline__ VI wave_best(VI x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(x.v, o, 64);
        const int   oi = __shfl_xor(x.i, o, 64);
        if (better(ov, oi, x.v, x.i)) {
            x.v = ov;
            x.i = oi;
        }
    }
    return x;
}
// block arg-best; result valid in all threads.  red: 2*nw words of LDS.
__device__ __forceinline__ VI block_best(VI x, float* redv, int* redi)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    x = wave_best(x);
    if (lane == 0) {
        redv[wid] = x.v;
        redi[wid] = x.i;
    }
    __syncthreads();
    VI r{redv[0], redi[0]};
    for (int w = 1; w < nw; w++) {
        if (better(redv[w], redi[w], r.v, r.i)) {
            r.v = redv[w];
            r.i = redi[w];
        }
    }
    __syncthreads();
    return r;
}

// workgroup max / sum of one float per thread through red[nw] (nw waves); result valid in all threads.  The sum adds the waves'
// partials in ascending order.  `red` is still being read when these return: a caller that writes it again puts a barrier first.
__device__ __forceinline__ float block_max(float v, float* red, const int nw)
{
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = v;
    }
    __syncthreads();
    v = red[0];
    for (int w = 1; w < nw; w++) {
        v = fmaxf(v, red[w]);
    }
    return v;
}
__device__ __forceinline__ float block_sum_ordered(float v, float* red, const int nw)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = v;
    }
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < nw; w++) {
        tot += red[w];
    }
    return tot;
}

// N partials {best, max, sum of exponentials} of a row (a workgroup's waves') -> the workgroup's: v / i / m / s hold partial w's
// entry at [w * stride].  Returns the best; row_max / tot: the maximum and the sum rescaled to it, added with w ascending.
template<int N>
__device__ __forceinline__ VI merge_waves(const float* v, const int* i, const float* m, const float* s, const int stride, float& row_max,
                                          float& tot)
{
    VI r{v[0], i[0]};
    row_max = m[0];
#pragma unroll
    for (int w = 1; w < N; w++) {
        if (better(v[w * stride], i[w * stride], r.v, r.i)) {
            r.v = v[w * stride];
            r.i = i[w * stride];
        }
        row_max = fmaxf(row_max, m[w * stride]);
    }
    tot = 0.f;
#pragma unroll
    for (int w = 0; w < N; w++) {
        tot += s[w * stride] * __expf(m[w * stride] - row_max);
    }
    return r;
}

// The stop-word rule (stop_criteria_kernels.cu:24-83): does word `id` of the list {words[stop_len], offs[stop_len]} end at position
// `step`?  token_at(pos) yields the token at a position; it is called for pos = step, step - 1, ... in DESCENDING order up to the
// first mismatch, so a caller may carry state from one position to the one before it (the beam step's parent chain).
template<class TokenAt>
__device__ __forceinline__ bool stop_word_ends_at(const int* words, const int* offs, const int id, const int step, TokenAt&& token_at)
{
    if (offs[id] < 0) {
        return false;
    }
    const int item_end = offs[id], item_start = id > 0 ? offs[id - 1] : 0;
    const int item_size = item_end - item_start;
    if (step + 1 < item_size) {
        return false;
    }
    for (int t = item_size - 1; t >= 0; t--) {
        if (token_at(step - (item_size - 1) + t) != words[item_start + t]) {
            return false;
        }
    }
    return true;
}

// K15 select_optional_last_tokens (select_optional_last_tokens.cu:22-85): every logit of the row `l` whose token is not in
// tokens[count] becomes -inf.  bits: (V + 31) / 32 words of LDS.  Ends with a workgroup barrier.
__device__ __forceinline__ void mask_optional_tokens(float* l, const int V, const int* tokens, const int count, uint32_t* bits)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int words = (V + 31) / 32;
    for (int i = tid; i < words; i += nt) {
        bits[i] = 0u;
    }
    __syncthreads();
    for (int j = tid; j < count; j += nt) {
        const int t = tokens[j];
        if (t >= 0 && t < V) {
            atomicOr(&bits[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
    for (int i = tid; i < V; i += nt) {
        if (!((bits[i >> 5] >> (i & 31)) & 1u)) {
            l[i] = -INFINITY;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
// identical to oracle/ftcf_oracle.c orc_uniform: (0,1].  The reference draws from curand XORWOW
// (sampling_topk_kernels.cu:32-65,283): only the distribution is reproducible, greedy is unaffected.  Like the reference's
// curand_init(seed, 0, 0) per row, the stream depends on the row's SEED and draw count only, never on where the row sits
// in a batch (`row` is 0 at every call site): a request samples the same tokens alone, in any batch, in any batcher slot.
__device__ __forceinline__ float ftcf_uniform(uint64_t seed, uint64_t row, uint64_t draw)
{
    const uint64_t z = splitmix64(seed ^ splitmix64(row * 0x632be59bd9b4e019ULL + draw));
    const uint32_t r = (uint32_t)(z >> 40);
    return (float)(r + 1u) * (1.0f / 16777216.0f);
}

// A logit as a slice reads it under a temperature (scale = 1.0f / (temperature + 1e-6f), k_decode_prep's factor; 1: none, and the
// product is the logit's own bits).  The product is rounded where it stands -- never contracted into a later subtraction -- so
// that it is the value k_decode_prep would have stored.
__device__ __forceinline__ float scaled_logit(const float v, const float scale)
{
#pragma clang fp contract(off)
    return v * scale;
}

// v1 > v2 <=> fkey(v1) > fkey(v2), v1 == v2 <=> fkey(v1) == fkey(v2) (no NaNs among logits): -0.0 has the key of +0.0 -- the two
// are ONE value for `better`, the oracle and the reference's comparison, and the index decides between them
__device__ __forceinline__ unsigned fkey(const float v)
{
    unsigned u = __float_as_uint(v);
    u          = (u == 0x80000000u) ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// exclusive prefix sum of one int per thread over the 256-thread block; `tot` = block total.  red: 4 ints of LDS.
__device__ __forceinline__ int block_excl_scan(const int v, int* red, int& tot)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int       inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) {
            inc += t;
        }
    }
    if (lane == 63) {
        red[wid] = inc;
    }
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wid; w++) {
        base += red[w];
    }
    tot = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return base + inc - v;
}

// a candidate {value, id} of a slice: plain stores, or write-through ones when the reader is a workgroup of the SAME launch
template<bool WT>
__device__ __forceinline__ void put_cand(float* ov, int* oi, const int pos, const float v, const int id)
{
    if constexpr (WT) {
        typedef __attribute__((address_space(1))) unsigned gu32;
        __hip_atomic_store((gu32*)(ov + pos), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((gu32*)(oi + pos), (unsigned)id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    else {
        ov[pos] = v;
        oi[pos] = id;
    }
}
// The `ke` (>= 2) best of the n elements of a slice as a SET -> ov / oi [0, ke): the block's threads hold element
// threadIdx.x + 256 j in vals[j] (j < ne); l: the slice in memory (only read when more elements equal the threshold than there
// are places; mask_end: element end_local reads as -FLT_MAX there, as it does in vals; scale: slice_load's).  See k_topk_stage1.
template<int MAXE, bool WT>
__device__ __forceinline__ void slice_select(const float (&vals)[MAXE], const int ne, const int n, const int ke, const float* l,
                                             const int i0, float* ov, int* oi, int (*hist8)[257], int* hist, int* s_sel, int* redi,
                                             const bool mask_end, const int end_local, const float scale = 1.f)
{
    // ---- radix select: key of the ke-th largest element ----
    unsigned prefix = 0u, mask = 0u;
    int      need = ke;
    for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            hist8[q][threadIdx.x] = 0;
        }
        __syncthreads();
        // (eight private copies of the histogram, picked by lane: the sign / exponent bytes of a row's logits fall into a
        // handful of bins)
#pragma unroll
        for (int j = 0; j < MAXE; j++) {
            const unsigned key = fkey(vals[j]);
            if (j < ne && (key & mask) == prefix) {
                atomicAdd(&hist8[threadIdx.x & 7][(key >> shift) & 255u], 1);
            }
        }
        __syncthreads();
        {
            int t = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                t += hist8[q][threadIdx.x];
            }
            hist[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x < 64) {  // bins 4 * lane .. 4 * lane + 3; suffix sums from the top bin down
            const int lane = threadIdx.x;
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int mine = h0 + h1 + h2 + h3;
            int       above = mine;  // inclusive suffix over lanes >= lane
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(above, o, 64);
                if (lane + o < 64) {
                    above += t;
                }
            }
            above -= mine;  // elements in bins of higher lanes
            // the lane whose bins contain the need-th element (counted from the top)
            if (above < need && above + mine >= need) {
                int acc = above;
                int bin = 4 * lane + 3;
                const int hh[4] = {h0, h1, h2, h3};
#pragma unroll
                for (int q = 3; q >= 0; q--) {
                    if (acc + hh[q] >= need) {
                        bin = 4 * lane + q;
                        break;
                    }
                    acc += hh[q];
                }
                s_sel[0] = bin;
                s_sel[1] = need - acc;
            }
        }
        __syncthreads();
        prefix |= (unsigned)s_sel[0] << shift;
        mask |= 255u << shift;
        need = s_sel[1];
        __syncthreads();
    }
    // prefix = key of the ke-th largest; `need` of the elements equal to it belong to the set, (ke - need) are greater
    if (threadIdx.x == 0) {
        s_sel[2] = 0;
    }
    __syncthreads();
    int ties = 0;
#pragma unroll
    for (int j = 0; j < MAXE; j++) {
        if (j < ne) {
            const unsigned key = fkey(vals[j]);
            if (key > prefix) {
                const int pos = atomicAdd(&s_sel[2], 1);
                put_cand<WT>(ov, oi, pos, vals[j], i0 + (int)threadIdx.x + 256 * j);
            }
            else if (key == prefix) {
                ties++;
            }
        }
    }
    int       tot  = 0;
    int       rank = block_excl_scan(ties, redi, tot);
    const int tie0 = ke - need;
    if (tot == need) {  // every element equal to the threshold belongs to the set (the usual case: exactly one)
#pragma unroll
        for (int j = 0; j < MAXE; j++) {
            if (j < ne && fkey(vals[j]) == prefix) {
                put_cand<WT>(ov, oi, tie0 + rank, vals[j], i0 + (int)threadIdx.x + 256 * j);
                rank++;
            }
        }
        return;
    }
    // more equal elements than places: the ones with the lowest indices (the tie rule of `better`) -- index order needs a
    // contiguous chunk per thread
    const int per = (n + 255) / 256;
    const int c0 = threadIdx.x * per, c1 = min(n, c0 + per);
    ties = 0;
    auto elem = [&](const int i) { return (mask_end && i == end_local) ? -FLT_MAX : scaled_logit(l[i], scale); };
    for (int i = c0; i < c1; i++) {
        ties += fkey(elem(i)) == prefix ? 1 : 0;
    }
    rank = block_excl_scan(ties, redi, tot);
    for (int i = c0; i < c1 && rank < need; i++) {
        if (fkey(elem(i)) == prefix) {
            put_cand<WT>(ov, oi, tie0 + rank, elem(i), i0 + i);
            rank++;
        }
    }
}

// The load pass of a slice of n logits at `l`: the block's threads keep element threadIdx.x + 256 j in vals[j] (j < ne) -- in REGISTERS
// from here on (all loads in flight at once; the arg max, the soft-max statistics, the four select passes and the emission read
// them there -- an earlier form staged the slice in LDS and every pass serialised on its LDS read -> atomic dependency).
// end_local >= 0: that element reads as -FLT_MAX (min_length, sampling_penalty_kernels.cu:485-520: end_id cannot be chosen yet).
// scale: every element is read as scaled_logit(., scale); the memory is left alone.
// Returns the thread's arg-best (local index) and, in lmax, the maximum of its elements.
template<int MAXE>
__device__ __forceinline__ VI slice_load(float (&vals)[MAXE], const float* l, const int ne, const int end_local, float& lmax,
                                         const float scale = 1.f)
{
#pragma unroll
    for (int j = 0; j < MAXE; j++) {
        vals[j] = (j < ne) ? scaled_logit(l[threadIdx.x + 256 * j], scale) : -INFINITY;
    }
    VI best{-INFINITY, 0x7fffffff};
    lmax = -FLT_MAX;
#pragma unroll
    for (int j = 0; j < MAXE; j++) {
        if (j < ne) {
            const int i = threadIdx.x + 256 * j;
            if (i == end_local) {
                vals[j] = -FLT_MAX;
            }
            const float v = vals[j];
            lmax          = fmaxf(lmax, v);
            if (best.i == 0x7fffffff || better(v, i, best.v, best.i)) {
                best.v = v;
                best.i = i;
            }
        }
    }
    return best;
}
// soft-max statistics of the slice (addBiasSoftMax, sampling_topp_kernels.cu:1296-1345, slice by slice): m = its maximum, the
// return value = sum of exp(v - m), both in all threads.  redv: 4 floats of LDS, free again on return.
template<int MAXE>
__device__ __forceinline__ float slice_stats(const float (&vals)[MAXE], const int ne, const float lmax, float* redv, float& m)
{
    m = block_max(lmax, redv, 4);
    __syncthreads();
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < MAXE; j++) {
        if (j < ne) {
            se += __expf(vals[j] - m);
        }
    }
    se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) {
        redv[threadIdx.x >> 6] = se;
    }
    __syncthreads();
    const float sum = (redv[0] + redv[1]) + (redv[2] + redv[3]);
    __syncthreads();
    return sum;
}

// bitonic sort of n2 (a power of two) {value, id} pairs in LDS, best first (value desc, id asc)
__device__ __forceinline__ void bitonic_sort_best_first(float* v, int* id, const int n2)
{
    for (int sz = 2; sz <= n2; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
                const int  lo = ((t / st) * 2) * st + (t % st), hi = lo + st;
                const bool desc = ((lo & sz) == 0);  // this block of the network sorts best-first
                const bool hi_better = better(v[hi], id[hi], v[lo], id[lo]);
                if (hi_better == desc) {
                    const float tv = v[lo];
                    const int   ti = id[lo];
                    v[lo]  = v[hi];
                    id[lo] = id[hi];
                    v[hi]  = tv;
                    id[hi] = ti;
                }
            }
        }
    }
    __syncthreads();
}

// The kc best of the n2 candidates sv / si (LDS) -> sv / si [0, kc) sorted best first: radix select of the kc-th best (as stage 1,
// over the LDS copy), the winners compacted into the k2 = 2^ceil(log2 kc) slots tv / ti, THOSE sorted (k = 50: 21 network stages
// instead of 45 over 512 pairs)
// (h8: eight private copies of the histogram, picked by lane -- for unions of thousands of candidates, whose sign / exponent bytes
//  fall into a handful of bins and would serialise on one LDS word; NULL: the single histogram)
__device__ __forceinline__ void union_topk(float* sv, int* si, const int n2, const int kc, const int k2, float* tv, int* ti, int* hist,
                                           int* s_sel, int* redi, int (*h8)[257] = nullptr)
{
    __syncthreads();
    unsigned prefix = 0u, mask = 0u;
    int      need = kc;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        if (h8) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                h8[q][threadIdx.x] = 0;
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < n2; c += 256) {
            const unsigned key = fkey(sv[c]);
            if ((key & mask) == prefix) {
                atomicAdd(h8 ? &h8[threadIdx.x & 7][(key >> shift) & 255u] : &hist[(key >> shift) & 255u], 1);
            }
        }
        __syncthreads();
        if (h8) {
            int t = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                t += h8[q][threadIdx.x];
            }
            hist[threadIdx.x] = t;
            __syncthreads();
        }
        if (threadIdx.x < 64) {
            const int lane = threadIdx.x;
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int mine = h0 + h1 + h2 + h3;
            int       above = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(above, o, 64);
                if (lane + o < 64) {
                    above += t;
                }
            }
            above -= mine;
            if (above < need && above + mine >= need) {
                int       acc = above, bin = 4 * lane + 3;
                const int hh[4] = {h0, h1, h2, h3};
#pragma unroll
                for (int q = 3; q >= 0; q--) {
                    if (acc + hh[q] >= need) {
                        bin = 4 * lane + q;
                        break;
                    }
                    acc += hh[q];
                }
                s_sel[0] = bin;
                s_sel[1] = need - acc;
            }
        }
        __syncthreads();
        prefix |= (unsigned)s_sel[0] << shift;
        mask |= 255u << shift;
        need = s_sel[1];
        __syncthreads();
    }
    // `need` of the entries equal to the threshold belong to the set: the ones with the smallest ids (the rule of `better`)
    if (threadIdx.x == 0) {
        s_sel[2] = 0;
    }
    for (int c = threadIdx.x; c < k2; c += 256) {
        tv[c] = -INFINITY;
        ti[c] = 0x7fffffff;
    }
    __syncthreads();
    // (the k-th best itself always equals the threshold: the usual case is exactly `need` such entries, all taken)
    int nties = 0;
    for (int c = threadIdx.x; c < n2; c += 256) {
        nties += fkey(sv[c]) == prefix ? 1 : 0;
    }
    int       tie_total = 0;
    (void)block_excl_scan(nties, redi, tie_total);
    const bool all_ties = tie_total == need;
    for (int c = threadIdx.x; c < n2; c += 256) {
        const unsigned key = fkey(sv[c]);
        bool           take = key > prefix || (all_ties && key == prefix);
        if (!all_ties && key == prefix) {
            int rank = 0;  // entries with the same value and a smaller id: real duplicates at the threshold, rare
            for (int d = 0; d < n2; d++) {
                rank += (fkey(sv[d]) == prefix && (si[d] < si[c] || (si[d] == si[c] && d < c))) ? 1 : 0;
            }
            take = rank < need;
        }
        if (take) {
            const int pos = atomicAdd(&s_sel[2], 1);
            tv[pos]       = sv[c];
            ti[pos]       = si[c];
        }
    }
    bitonic_sort_best_first(tv, ti, k2);
    for (int c = threadIdx.x; c < kc; c += 256) {
        sv[c] = tv[c];
        si[c] = ti[c];
    }
    __syncthreads();
}

// one candidate per slice (k = 1): the best of the nsl (<= 256) in sv / si -> sv[0] / si[0]
__device__ __forceinline__ void best_of_slices(float* sv, int* si, const int nsl, float* redv, int* redi)
{
    __syncthreads();
    VI best{-INFINITY, 0x7fffffff};
    if ((int)threadIdx.x < nsl) {
        best.v = sv[threadIdx.x];
        best.i = si[threadIdx.x];
    }
    const VI r = block_best(best, redv, redi);
    if (threadIdx.x == 0) {
        sv[0] = r.v;
        si[0] = r.i;
    }
    __syncthreads();
}

// The top-k layer's draw by ONE thread (sampling_topk_kernels.cu:210-311): sv[0, k) are the row's k best values, best first; they
// become their probabilities, uniform number `draw` of the stream of `seed` is taken (no counter is touched: the n-th token of a
// request consumes draw n, whoever asks) and the walk's place is returned.  soft_max: the probabilities are the row's soft-max
// (the form of return_cum_log_probs) from stat(2 q), stat(2 q + 1) = {max, sum of exponentials} of slice q < NSL, not read
// otherwise; p_topk: the p of the top-k layer.
template<int NSL, class Stat>
__device__ __forceinline__ int topk_draw_at(const bool soft_max, const uint64_t seed, const uint64_t draw, const float p_topk, const int k,
                                            float* sv, Stat stat)
{
    const float smax = sv[0];
    float       ssum = 0.f;
    float       row_max = 0.f, row_den = 1.f;
    if (soft_max) {  // addBiasSoftMax of the row (sampling_topp_kernels.cu:1296-1345) from the slice statistics
        float sm[NSL], ss[NSL];
        row_max = -FLT_MAX;
        for (int q = 0; q < NSL; q++) {
            sm[q]   = stat(2 * q);
            ss[q]   = stat(2 * q + 1);
            row_max = fmaxf(row_max, sm[q]);
        }
        float tot = 0.f;
        for (int q = 0; q < NSL; q++) {
            tot += ss[q] * __expf(sm[q] - row_max);
        }
        row_den = tot + 1e-6f;
    }
    for (int i = 0; i < k; i++) {
        float u = sv[i];
        if (!soft_max) {
            u = __expf(u - smax);  // :271-275
        }
        else {
            u = __expf(u - row_max) / row_den;  // the probability the reference's in-place softmax leaves there
        }
        sv[i] = u;
        ssum += u;
    }
    const float u01 = ftcf_uniform(seed, 0, draw);
    float       rnd  = u01 * p_topk * ssum;  // :283
    int         pick = k - 1;
    for (int i = 0; i < k; i++) {
        rnd -= sv[i];
        if (rnd <= 0.0f || i == k - 1) {
            pick = i;
            break;
        }
    }
    return pick;
}

}  // namespace ftcf
