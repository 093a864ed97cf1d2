// Device primitives shared by the dynamic decode (kernels_sampling.hip) and beam search (kernels_beam.hip): the {value, id}
// arg-best with its tie rule, the workgroup max / sum through an LDS array, the optional-last-tokens mask.
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

}  // namespace ftcf
