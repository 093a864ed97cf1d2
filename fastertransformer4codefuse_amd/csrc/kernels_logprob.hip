// Fused LM head -> log-probability of a target token per row (prompt scoring).
//
// Counterpart of ParallelGpt's context log-probs (models/multi_gpu_gpt/ParallelGpt.cc:403-470: a cuBLAS LM-head GEMM that
// writes [S, B, V] fp32 logits, then kernels/logprob_kernels.cu:36-100 reads them back).  Here the logits never reach memory:
// one MFMA launch computes them tile by tile and reduces every tile at once to per-row soft-max statistics, a second small
// launch merges a row's tiles in fixed order.
//
// k_lm_head_logprob_tiles: a workgroup (4 waves) owns a LP_BM x LP_BN tile of logits l[r, j] = sum_k A[r, k] W[j, k] (fp16
// products, fp32 accumulation on mfma_f32_16x16x32_f16).  Both operands go through LDS in LP_KC-wide k chunks, the next chunk
// requested into registers before the current one is consumed.  Wave (wr, wc) holds rows wr*32 .. +32 x columns wc*64 .. +64:
// 2 x 4 accumulator tiles, the row of accumulator element q on lane (c, g) being g*4 + q, its column c.  The epilogue takes a
// row's max and sum of exp over the wave's 64 columns with a butterfly over the 16 lanes that share g, the two column halves
// are combined through LDS (always half 0 then half 1), and the tile publishes {max, sum} per row; the workgroup whose columns
// hold a row's target writes that logit too.  Columns >= n are -inf (left out of both reductions).
//
// Dispatch order: the m-blocks of one n-block are consecutive on ONE XCD (blocks b and b + 8 share an XCD): they run side by
// side and read the weight tile from that XCD's L2 after the first has brought it in, so the 1 GB head comes from HBM about
// once whatever m is.
//
// k_lm_head_logprob_merge: one wave per row, lane i folds n-blocks i, i + 64, ... in order, a fixed butterfly combines the lanes:
// the result does not depend on which tile finished first, and two runs are bit-identical.
#include "ftcf_common.h"
#include "kernels.h"

#include <algorithm>
#include <map>
#include <mutex>

namespace ftcf {

constexpr int LP_BM = 64, LP_BN = 128, LP_KC = 128, LP_LDT = LP_KC + 8;  // (row stride: 16 lanes of a phase on 64 banks)
constexpr int LP_THREADS = 256;
constexpr int LP_AP = LP_BM * LP_KC / 8 / LP_THREADS;  // 16-byte pieces of the A chunk per thread (4)
constexpr int LP_WP = LP_BN * LP_KC / 8 / LP_THREADS;  // ... of the W chunk (8)

__device__ __forceinline__ void lp_combine(float& m, float& s, const float m2, const float s2)
{
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) {
        return;  // (both empty)
    }
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
}

__global__ __launch_bounds__(LP_THREADS) void k_lm_head_logprob_tiles(const f16* __restrict__ A, const f16* __restrict__ W,
                                                                    const int* __restrict__ targets, float2* __restrict__ part,
                                                                    float* __restrict__ tgt_logit, int m, int n, int k, int MB,
                                                                    int NB)
{
    __shared__ __attribute__((aligned(16))) f16 as[LP_BM * LP_LDT];
    __shared__ __attribute__((aligned(16))) f16 ws[LP_BN * LP_LDT];
    __shared__ float xm[LP_BM], xs[LP_BM];
    // tile of this workgroup: consecutive slots of one XCD walk the m-blocks of one n-block
    int nb, mb;
    if (MB == 1) {
        nb = blockIdx.x;
        mb = 0;
    }
    else {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        nb = (slot / MB) * 8 + xcd;
        mb = slot % MB;
    }
    if (nb >= NB) {
        return;  // (padding of the XCD-ordered grid; before any barrier)
    }
    const int m0 = mb * LP_BM, n0 = nb * LP_BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int wr = wid >> 1, wc = wid & 1;
    const int nkc = (k + LP_KC - 1) / LP_KC;  // (a last partial chunk reads zeros past k)

    u32x4 ar[LP_AP], wreg[LP_WP];
    auto  fetch = [&](const int kc) {
#pragma unroll
        for (int u = 0; u < LP_AP; u++) {
            const int idx = threadIdx.x + u * LP_THREADS;
            int       row = m0 + idx / (LP_KC / 8);
            row           = row < m ? row : m - 1;
            const int ko  = kc * LP_KC + (idx % (LP_KC / 8)) * 8;
            ar[u]         = ko < k ? *reinterpret_cast<const u32x4*>(A + (size_t)row * k + ko) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < LP_WP; u++) {
            const int idx = threadIdx.x + u * LP_THREADS;
            int       row = n0 + idx / (LP_KC / 8);
            row           = row < n ? row : n - 1;
            const int ko  = kc * LP_KC + (idx % (LP_KC / 8)) * 8;
            wreg[u]       = ko < k ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + (size_t)row * k + ko))
                                   : u32x4{0u, 0u, 0u, 0u};
        }
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    fetch(0);
    for (int kc = 0; kc < nkc; kc++) {
#pragma unroll
        for (int u = 0; u < LP_AP; u++) {
            const int idx = threadIdx.x + u * LP_THREADS;
            *reinterpret_cast<u32x4*>(&as[(idx / (LP_KC / 8)) * LP_LDT + (idx % (LP_KC / 8)) * 8]) = ar[u];
        }
#pragma unroll
        for (int u = 0; u < LP_WP; u++) {
            const int idx = threadIdx.x + u * LP_THREADS;
            *reinterpret_cast<u32x4*>(&ws[(idx / (LP_KC / 8)) * LP_LDT + (idx % (LP_KC / 8)) * 8]) = wreg[u];
        }
        __syncthreads();
        if (kc + 1 < nkc) {
            fetch(kc + 1);  // (in flight under this chunk's MFMAs)
        }
#pragma unroll
        for (int ks = 0; ks < LP_KC / 32; ks++) {
            f16x8 af[2], bf[4];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                af[i] = *reinterpret_cast<const f16x8*>(&as[(wr * 32 + i * 16 + c) * LP_LDT + ks * 32 + g * 8]);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bf[j] = *reinterpret_cast<const f16x8*>(&ws[(wc * 64 + j * 16 + c) * LP_LDT + ks * 32 + g * 8]);
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();  // (the next chunk overwrites the tiles)
    }

    // ---- epilogue: per row, {max, sum exp} over this wave's 64 columns, then over the tile's 128 ----
    float rmax[2][4], rsum[2][4];
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = m0 + wr * 32 + i * 16 + g * 4 + q;
            const int t   = row < m ? targets[row] : -1;
            float     mx  = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int col = n0 + wc * 64 + j * 16 + c;
                if (col >= n) {
                    acc[i][j][q] = -INFINITY;
                }
                else if (col == t) {
                    tgt_logit[row] = acc[i][j][q];  // (exactly one tile and lane own a target column)
                }
                mx = fmaxf(mx, acc[i][j][q]);
            }
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, o, 16));
            }
            float s = 0.f;
            if (mx != -INFINITY) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    s += __expf(acc[i][j][q] - mx);
                }
            }
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) {
                s += __shfl_xor(s, o, 16);
            }
            rmax[i][q] = mx;
            rsum[i][q] = s;
        }
    }
    if (wc == 1 && c == 0) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                xm[wr * 32 + i * 16 + g * 4 + q] = rmax[i][q];
                xs[wr * 32 + i * 16 + g * 4 + q] = rsum[i][q];
            }
        }
    }
    __syncthreads();
    if (wc == 0 && c == 0) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r   = wr * 32 + i * 16 + g * 4 + q;
                const int row = m0 + r;
                float     mx = rmax[i][q], s = rsum[i][q];
                lp_combine(mx, s, xm[r], xs[r]);
                if (row < m) {
                    part[(size_t)nb * m + row] = float2{mx, s};
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_lm_head_logprob_merge(const float2* __restrict__ part, const float* __restrict__ tgt_logit,
                                                              const int* __restrict__ targets, float* __restrict__ log_probs,
                                                              float* __restrict__ row_lse, int m, int n, int NB)
{
    const int lane = threadIdx.x & 63;
    const int row  = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) {
        return;
    }
    float mx = -INFINITY, s = 0.f;
    for (int b = lane; b < NB; b += 64) {
        const float2 v = part[(size_t)b * m + row];
        lp_combine(mx, s, v.x, v.y);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(mx, o), s2 = __shfl_xor(s, o);
        lp_combine(mx, s, m2, s2);
    }
    if (lane == 0) {
        const float lse = mx + logf(s);
        const int   t   = targets[row];
        log_probs[row]  = (t >= 0 && t < n) ? tgt_logit[row] - lse : 0.f;
        if (row_lse) {
            row_lse[row] = lse;
        }
    }
}

size_t lm_head_log_probs_workspace_bytes(int m, int n)
{
    const size_t NB = (size_t)(n + LP_BN - 1) / LP_BN;
    return NB * m * sizeof(float2) + (size_t)m * sizeof(float);
}

void launch_lm_head_log_probs(const f16* A, const f16* W_nk, const int* targets, float* log_probs, float* row_lse, int m, int n,
                              int k, void* ws, hipStream_t s)
{
    FTCF_CHECK_ARG(m >= 1 && n >= 1 && k >= 8 && k % 8 == 0, "LM-head log-probs need m, n >= 1 and k % 8 == 0");
    FTCF_CHECK_ARG(ws != nullptr, "LM-head log-probs: no workspace");
    const int MB = (m + LP_BM - 1) / LP_BM, NB = (n + LP_BN - 1) / LP_BN;
    float2*   part = reinterpret_cast<float2*>(ws);
    float*    tgt  = reinterpret_cast<float*>(part + (size_t)NB * m);
    const int grid = MB == 1 ? NB : ((NB + 7) / 8) * 8 * MB;
    hipLaunchKernelGGL(k_lm_head_logprob_tiles, dim3(grid), dim3(LP_THREADS), 0, s, A, W_nk, targets, part, tgt, m, n, k, MB, NB);
    FTCF_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_lm_head_logprob_merge, dim3((m + 3) / 4), dim3(256), 0, s, part, tgt, targets, log_probs, row_lse, m, n, NB);
    FTCF_HIP_CHECK(hipGetLastError());
}

// ---- the engine's prompt scoring around launch_lm_head_log_probs ----
// hidden row (b, t) predicts token t + 1: target ids[b, t + 1] inside the prompt, none (-1) past it
__global__ void k_context_targets(int* targets, const int* ids, const int* lengths, int B, int S)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * S) {
        const int b = i / S, t = i % S;
        targets[i]  = t + 1 < lengths[b] ? ids[(size_t)b * S + t + 1] : -1;
    }
}
// out[b, t] = log P(ids[b, t] | ids[b, < t]) = lp[b, t - 1]; out[b, 0] = 0
__global__ void k_context_shift(float* out, const float* lp, int B, int S)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * S) {
        out[i] = (i % S) == 0 ? 0.f : lp[i - 1];
    }
}
// [T, B] time-major -> [B, T]
__global__ void k_transpose_log_probs(float* out, const float* in, int T, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * T) {
        const int b = i / T, t = i % T;
        out[i]      = in[(size_t)t * B + b];
    }
}

void launch_context_log_probs(float* out, const f16* hidden_nrm, const f16* W_nk, const int* ids, const int* lengths, int* targets,
                              float* lp, int B, int S, int V, int H, hipStream_t s)
{
    const int M = B * S;
    hipLaunchKernelGGL(k_context_targets, dim3((M + 255) / 256), dim3(256), 0, s, targets, ids, lengths, B, S);
    FTCF_HIP_CHECK(hipGetLastError());
    launch_lm_head_log_probs(hidden_nrm, W_nk, targets, lp, nullptr, M, V, H, lm_head_log_probs_workspace(M, V, s), s);
    hipLaunchKernelGGL(k_context_shift, dim3((M + 255) / 256), dim3(256), 0, s, out, lp, B, S);
    FTCF_HIP_CHECK(hipGetLastError());
}

void launch_transpose_log_probs(float* out, const float* in, int T, int B, hipStream_t s)
{
    hipLaunchKernelGGL(k_transpose_log_probs, dim3((B * T + 255) / 256), dim3(256), 0, s, out, in, T, B);
    FTCF_HIP_CHECK(hipGetLastError());
}

// top_logprobs: the pairs of a row that had finished before the step
__global__ void k_fill_top_logprobs(int* ids, float* values, size_t pairs)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (size_t)gridDim.x * blockDim.x) {
        ids[i]    = -1;
        values[i] = 0.f;
    }
}
// [T, B, N] time-major -> [B, T, N]
__global__ void k_transpose_top_logprobs(int* out_ids, float* out_values, const int* ids, const float* values, int T, int B, int N)
{
    const size_t total = (size_t)B * T * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int    j   = (int)(i % N);
        const size_t bt  = i / N;
        const int    b   = (int)(bt / T), t = (int)(bt % T);
        const size_t src = ((size_t)t * B + b) * N + j;
        out_ids[i]    = ids[src];
        out_values[i] = values[src];
    }
}

void launch_fill_top_logprobs(int* ids, float* values, size_t pairs, hipStream_t s)
{
    if (pairs == 0) {
        return;
    }
    const int grid = (int)std::min<size_t>((pairs + 255) / 256, 2048);
    hipLaunchKernelGGL(k_fill_top_logprobs, dim3(grid), dim3(256), 0, s, ids, values, pairs);
    FTCF_HIP_CHECK(hipGetLastError());
}

void launch_transpose_top_logprobs(int* out_ids, float* out_values, const int* ids, const float* values, int T, int B, int N,
                                   hipStream_t s)
{
    const size_t total = (size_t)B * T * N;
    const int    grid  = (int)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(k_transpose_top_logprobs, dim3(grid), dim3(256), 0, s, out_ids, out_values, ids, values, T, B, N);
    FTCF_HIP_CHECK(hipGetLastError());
}

// one grow-only workspace per (device, stream) that has called, kept for the life of the process (as abi_gemm_workspace)
void* lm_head_log_probs_workspace(int m, int n, hipStream_t s)
{
    static std::mutex                                                   mu;
    static std::map<std::pair<int, hipStream_t>, std::pair<void*, size_t>> ws;
    int                                                                 dev = 0;
    FTCF_HIP_CHECK(hipGetDevice(&dev));
    const size_t                need = lm_head_log_probs_workspace_bytes(m, n);
    std::lock_guard<std::mutex> lock(mu);
    auto&                       e = ws[{dev, s}];
    if (e.second < need) {
        if (e.first) {
            FTCF_HIP_CHECK(hipStreamSynchronize(s));  // (the stream's earlier launches may still read the old buffer)
            FTCF_HIP_CHECK(hipFree(e.first));
            e.first = nullptr;
        }
        FTCF_HIP_CHECK(hipMalloc(&e.first, need));
        e.second = need;
    }
    return e.first;
}

}  // namespace ftcf
