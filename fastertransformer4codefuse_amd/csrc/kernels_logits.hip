// Per-request logit processors of the continuous batcher (include/ftcf.h ftcf_logit_process): one stage over fp32 logits [B, V],
// in place, between the LM head and the dynamic decode.  Counterparts in the reference: kernels/ban_bad_words.cu:22-86 (bad
// words), the additive presence / frequency form of kernels/sampling_penalty_kernels.cu, DynamicDecodeLayer's min_length; the
// logit bias and the allowed-token mask have none.
//
// Order per processed row: penalties over the GENERATED tokens, bias, min_new_tokens, bad words, mask, then the guard.
//
// k_logit_process: a workgroup owns ONE (row, slice of `slice` consecutive logits); nobody else writes them, so the result
// does not depend on the grid.  It first turns every sparse option into LDS state of its slice --
//   s_cnt[i]   occurrences of token lo + i among the row's generated tokens (integer LDS atomics: order does not matter),
//   s_bias[i]  the bias of token lo + i, valid where s_biased has its bit (ids are distinct: plain stores),
//   s_ban      one bit per logit the end-token hold-back or a bad word bans --
// and then makes one elementwise pass: v -= presence + frequency * c where c > 0, v += bias (in fp64, rounded once), v = -inf
// where banned or not allowed.  A logit nothing applies to is not written at all.  The logits were written by the LM head a
// moment ago (L2), and a row starts at b * V floats -- 16-byte aligned only when V % 4 == 0 -- so the pass reads plain dwords, a
// wave 256 contiguous bytes.  The whole history is read by every workgroup of the row (a few thousand tokens against a slice's
// 8 KB of logits).
//
// k_logit_guard: one workgroup per row, behind it on the stream: a processed row without a single finite logit gets
// logit[end_id] = 0 -- the request ends, and the sampling kernels never see a row whose soft-max is NaN.  It leaves at the
// first 2048-logit chunk that holds a finite value: only a heavily masked row is read to its end.
#include "ftcf_common.h"
#include "kernels.h"

namespace ftcf {

constexpr int LOGIT_THREADS = 256;

struct LogitRow {
    float      presence, frequency;
    int        n_bias, min_new, hist_len, gen_start;
    const int* words;  // the row's [2][bad_len] word list or NULL
    bool       penalised, masked, any;
};
// what row b asks for; `any` false: the row keeps its bits (uniform over the workgroup)
__device__ __forceinline__ LogitRow logit_row(const LogitProcessParams& p, const int b)
{
    LogitRow r{};
    if ((p.finished && p.finished[b]) || (p.row_on && !p.row_on[b])) {
        return r;
    }
    r.presence  = p.presence ? p.presence[b] : 0.f;
    r.frequency = p.frequency ? p.frequency[b] : 0.f;
    r.n_bias    = (p.n_bias && p.bias_ids && p.bias_values) ? min(max(p.n_bias[b], 0), min(p.bias_stride, LOGIT_BIAS_MAX)) : 0;
    r.min_new   = p.min_new ? p.min_new[b] : 0;
    r.hist_len  = p.hist ? max(p.hist_len[b] + p.hist_len_add, 0) : 0;
    r.gen_start = p.hist ? min(max(p.gen_start[b], 0), r.hist_len) : 0;
    r.words     = p.bad_words ? p.bad_words + (size_t)b * 2 * p.bad_len : nullptr;
    if (r.words && r.words[p.bad_len] < 0) {  // (a word needs the offset before it: the valid words are a prefix of the list)
        r.words = nullptr;
    }
    r.penalised = r.presence != 0.f || r.frequency != 0.f;
    r.masked    = p.mask && (!p.mask_on || p.mask_on[b]);
    r.any       = r.penalised || r.n_bias > 0 || r.min_new > 0 || r.words || r.masked;
    return r;
}

__global__ __launch_bounds__(LOGIT_THREADS) void k_logit_process(const LogitProcessParams p)
{
    __shared__ int      s_cnt[LOGIT_SLICE_MAX];
    __shared__ float    s_bias[LOGIT_SLICE_MAX];
    __shared__ unsigned s_biased[LOGIT_SLICE_MAX / 32], s_ban[LOGIT_SLICE_MAX / 32];
    const int      b = blockIdx.y, tid = threadIdx.x;
    const LogitRow r = logit_row(p, b);
    if (!r.any) {
        return;
    }
    const int lo = blockIdx.x * p.slice, n = min(p.slice, p.V - lo);
    for (int i = tid; i < LOGIT_SLICE_MAX / 32; i += LOGIT_THREADS) {
        s_biased[i] = 0u;
        s_ban[i]    = 0u;
    }
    if (r.penalised) {
        for (int i = tid; i < n; i += LOGIT_THREADS) {
            s_cnt[i] = 0;
        }
    }
    __syncthreads();
    const int* hist = p.hist + (long long)b * p.stride_b;
    if (r.penalised) {
        for (int t = r.gen_start + tid; t < r.hist_len; t += LOGIT_THREADS) {
            const int d = hist[(long long)t * p.stride_t] - lo;
            if ((unsigned)d < (unsigned)n) {
                atomicAdd(&s_cnt[d], 1);
            }
        }
    }
    for (int j = tid; j < r.n_bias; j += LOGIT_THREADS) {
        const int d = p.bias_ids[(size_t)b * p.bias_stride + j] - lo;
        if ((unsigned)d < (unsigned)n) {
            s_bias[d] = p.bias_values[(size_t)b * p.bias_stride + j];
            atomicOr(&s_biased[d >> 5], 1u << (d & 31));
        }
    }
    if (tid == 0 && r.hist_len - r.gen_start < r.min_new) {
        const int d = p.end_id - lo;
        if ((unsigned)d < (unsigned)n) {
            atomicOr(&s_ban[d >> 5], 1u << (d & 31));
        }
    }
    if (r.words) {
        // ban_bad_words.cu:42-85 (without its `0 < banned_token`: id 0 can be banned): word j = ids [start, end); its last token
        // is banned when the n - 1 before it are the history's last n - 1 (prompt and generated tokens alike)
        for (int j = tid; j < p.bad_len; j += LOGIT_THREADS) {
            const int end = r.words[p.bad_len + j], start = j > 0 ? r.words[p.bad_len + j - 1] : 0;
            if (start < 0 || end <= start || end > p.bad_len) {
                continue;
            }
            const int d = r.words[end - 1] - lo, m = end - start - 1;
            if ((unsigned)d >= (unsigned)n || m > r.hist_len) {
                continue;
            }
            bool hit = true;
            for (int k = 0; k < m && hit; k++) {
                hit = hist[(long long)(r.hist_len - m + k) * p.stride_t] == r.words[start + k];
            }
            if (hit) {
                atomicOr(&s_ban[d >> 5], 1u << (d & 31));
            }
        }
    }
    __syncthreads();
    float*          row  = p.logits + (size_t)b * p.V + lo;
    const unsigned* mask = r.masked ? p.mask + (size_t)b * ((p.V + 31) / 32) : nullptr;
    for (int i = tid; i < n; i += LOGIT_THREADS) {
        const float in = row[i];
        float       v  = in;
        const int   c  = r.penalised ? s_cnt[i] : 0;
        const bool  biased = (s_biased[i >> 5] >> (i & 31)) & 1u;
        if (c > 0 || biased) {
            // the few logits a penalty or a bias reaches: summed in fp64 (the products and sums of these fp32 operands are exact
            // there up to 2^-53) and rounded ONCE, so the result is within half an fp32 ulp of the exact value
            double d = (double)in;
            if (c > 0) {
                d -= (double)r.presence + (double)r.frequency * (double)c;
            }
            if (biased) {
                d += (double)s_bias[i];
            }
            v = (float)d;
        }
        bool ban = (s_ban[i >> 5] >> (i & 31)) & 1u;
        if (mask) {
            const int t = lo + i;
            ban |= !((mask[t >> 5] >> (t & 31)) & 1u);
        }
        if (ban) {
            v = -INFINITY;
        }
        if (__float_as_uint(v) != __float_as_uint(in)) {
            row[i] = v;
        }
    }
}

__global__ __launch_bounds__(LOGIT_THREADS) void k_logit_guard(const LogitProcessParams p)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!logit_row(p, b).any) {
        return;
    }
    float* row = p.logits + (size_t)b * p.V;
    for (int base = 0; base < p.V; base += LOGIT_THREADS * 8) {
        int finite = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int i = base + k * LOGIT_THREADS + tid;
            if (i < p.V) {
                finite |= isfinite(row[i]) ? 1 : 0;
            }
        }
        if (__syncthreads_or(finite)) {
            return;
        }
    }
    if (tid == 0) {
        row[p.end_id] = 0.f;
    }
}

void launch_logit_process(const LogitProcessParams& p, hipStream_t s)
{
    LogitProcessParams q = p;
    if (q.slice <= 0) {
        q.slice = LOGIT_SLICE_DEFAULT;
    }
    FTCF_CHECK_ARG(q.logits && q.B >= 1 && q.B <= 65535 && q.V >= 1 && q.end_id >= 0 && q.end_id < q.V, "logit process: bad geometry");
    FTCF_CHECK_ARG(q.slice >= 32 && q.slice <= LOGIT_SLICE_MAX && q.slice % 32 == 0, "logit process: slice must be a multiple of 32 in [32, 4096]");
    FTCF_CHECK_ARG(!q.hist || (q.hist_len && q.gen_start), "logit process: a history needs hist_len and gen_start");
    FTCF_CHECK_ARG(!q.bad_words || (q.bad_len >= 1 && q.bad_len <= LOGIT_BAD_WORDS_MAX), "logit process: bad_words_len must be in [1, 256]");
    FTCF_CHECK_ARG(q.bias_stride >= 0, "logit process: negative bias_stride");
    hipLaunchKernelGGL(k_logit_process, dim3((q.V + q.slice - 1) / q.slice, q.B), dim3(LOGIT_THREADS), 0, s, q);
    hipLaunchKernelGGL(k_logit_guard, dim3(q.B), dim3(LOGIT_THREADS), 0, s, q);
    FTCF_HIP_CHECK(hipGetLastError());
}

}  // namespace ftcf
