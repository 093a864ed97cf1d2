// Speculative greedy decoding: the kernels of a verify pass over R = drafts + 1 rows of ONE sequence.
//
//  * k_verify_attention : decode attention for R <= 16 consecutive new tokens of one sequence.  launch_mmha treats its rows as
//      different sequences and would stream the same `len` cached keys R times; here a (head, key-split) workgroup reads its
//      K / V rows ONCE into registers and scores them against all R rotated queries (staged once in LDS, held in registers by
//      every lane).  The R new keys are a causal R x R tail served from LDS by the last split's workgroup (row i never reads
//      row j's key from the cache: another workgroup may not have written it yet).  Arithmetic and rounding points are
//      mmha_partial's (attn_device.hip.h): half q / k / v + bias, NeoX rotary with the fp32 angle, packed dot2 scores in fp32,
//      exp against the split's row maximum, fp32 P.V, the split partials merged in split order by the workgroup that draws
//      the head's last ticket (the ORDER is fixed whoever merges: two launches give the same bits), one normalisation with
//      the reference's + 1e-6, the context rounded once.
//  * k_ngram_draft      : prompt-lookup drafting, one workgroup.
//  * k_verify_embed     : the pass's input rows.
//  * k_verify_slices / k_verify_close : the acceptance rule of every greedy request, bare or with stop words, log-probabilities
//      or a callback.
//  * k_verify_topk_slices / k_verify_pick / k_verify_sample_close : the same for a top-k sampled request, token for token.
//
// Roofline: HBM (4 * len * dh * nh bytes per layer, once for all rows); the VALU work grows with R (R * dh fused
// multiply-adds per key and head, twice).
#include "attn_device.hip.h"
#include "sampling_device.hip.h"

namespace ftcf {

constexpr int VA_MAX_CHUNK = 256;                                  // cached keys of a workgroup
constexpr int VA_LDP       = VA_MAX_CHUNK + VERIFY_MAX_ROWS + 4;   // row stride of the score tile (floats)
constexpr int VA_MAX_SPLIT = 128;                                  // the merger keeps {max, sum} of every split in a score row
constexpr int VA_WGS       = 512;                                  // workgroups a launch aims for

typedef __attribute__((address_space(1))) unsigned va_gu32;

// keys per workgroup: a multiple of 32 (one round of the four waves at either head size) in [64, 256]
static int verify_chunk(int len, int nh)
{
    const long want = ((long)len * nh + VA_WGS - 1) / VA_WGS;
    const int  c    = (int)((want + 31) / 32 * 32);
    return std::max(64, std::min(VA_MAX_CHUNK, c));
}
// the most splits any len <= s_max gets: 64-key chunks never exceed s_max / 64 splits, a chunk of len * nh / VA_WGS keys or more
// never VA_WGS / nh, 256-key chunks never s_max / 256 (all rounded up)
static int verify_max_split(int nh, int s_max)
{
    nh = std::max(nh, 1);
    return std::max(1, std::min((s_max + 63) / 64, std::max((VA_WGS + nh - 1) / nh, (s_max + VA_MAX_CHUNK - 1) / VA_MAX_CHUNK)));
}
bool verify_attention_supported(int nh, int dh, int s_max)
{
    return (dh == 64 || dh == 128) && nh >= 1 && s_max >= 1 && verify_max_split(nh, s_max) <= VA_MAX_SPLIT;
}
size_t verify_attention_ticket_bytes(int nh)
{
    return ((size_t)nh * sizeof(unsigned) + 255) & ~(size_t)255;
}
size_t verify_attention_workspace_bytes(int R, int nh, int dh, int s_max)
{
    return verify_attention_ticket_bytes(nh) + (size_t)nh * verify_max_split(nh, s_max) * R * (dh + 2) * sizeof(float);
}

template<int DH>
__global__ __launch_bounds__(256) void k_verify_attention(const VerifyAttnParams p, const int chunk, const int nsplit)
{
    constexpr int LPK = DH / 8;    // lanes per key / value row (16 B each)
    constexpr int KPI = 64 / LPK;  // rows per wave-load
    constexpr int RM  = VERIFY_MAX_ROWS;
    constexpr int U   = 4;         // rows per lane and round; two rounds in flight
    constexpr int STEP = 4 * KPI;  // keys of one wave-load of the four waves
    __shared__ __attribute__((aligned(16))) f16 s_q[RM * DH];
    __shared__ __attribute__((aligned(16))) f16 s_k[RM * DH];
    __shared__ __attribute__((aligned(16))) f16 s_v[RM * DH];
    __shared__ float s_p[RM * VA_LDP];
    __shared__ float s_o[RM * DH];
    __shared__ float s_m[RM], s_l[RM];
    __shared__ int   s_last;

    const int  h = blockIdx.x, sp = blockIdx.y;
    const int  lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int  sub = lane % LPK, grp = lane / LPK;
    const int  R = p.R, len = p.len, hl = p.nh * DH;
    const int  t_beg = sp * chunk;
    const int  nk    = min(len - t_beg, chunk);  // cached keys of this split (0 only when len == 0)
    const bool owner = sp == nsplit - 1;         // serves the R new keys
    const int  n_loc = nk + (owner ? R : 0);
    f16*       kc = p.k_cache + (size_t)h * p.s_max * DH;
    f16*       vc = p.v_cache + (size_t)h * p.s_max * DH;

    for (int i = threadIdx.x; i < R * DH; i += 256) {
        const int    r = i / DH, d = i % DH;
        const size_t base = (size_t)r * 3 * hl + h * DH + d;
        s_q[i] = p.qkv[base] + (p.qkv_bias ? p.qkv_bias[h * DH + d] : (f16)0.f);
        if (owner) {
            s_k[i] = p.qkv[base + hl] + (p.qkv_bias ? p.qkv_bias[hl + h * DH + d] : (f16)0.f);
            s_v[i] = p.qkv[base + 2 * hl] + (p.qkv_bias ? p.qkv_bias[2 * hl + h * DH + d] : (f16)0.f);
        }
    }
    __syncthreads();
    const int half = p.rot / 2;
    for (int i = threadIdx.x; i < R * half; i += 256) {
        const int r = i / half, j = i % half;
        float     cs, sn;
        if (p.rot_table) {
            cs = p.rot_table[(size_t)i * 2];
            sn = p.rot_table[(size_t)i * 2 + 1];
        }
        else {
            rotary_coef(j, p.rot, len + r, cs, sn);
        }
        f16 a = s_q[r * DH + j], c = s_q[r * DH + j + half];
        rotary_apply(a, c, cs, sn);
        s_q[r * DH + j]        = a;
        s_q[r * DH + j + half] = c;
        if (owner) {
            f16 ka = s_k[r * DH + j], kc2 = s_k[r * DH + j + half];
            rotary_apply(ka, kc2, cs, sn);
            s_k[r * DH + j]        = ka;
            s_k[r * DH + j + half] = kc2;
        }
    }
    __syncthreads();
    if (owner) {  // append rows [len, len + R) to the cache
        for (int i = threadIdx.x; i < R * DH / 8; i += 256) {
            *reinterpret_cast<u32x4*>(kc + (size_t)len * DH + i * 8) = *reinterpret_cast<const u32x4*>(s_k + i * 8);
            *reinterpret_cast<u32x4*>(vc + (size_t)len * DH + i * 8) = *reinterpret_cast<const u32x4*>(s_v + i * 8);
        }
    }

    // the split's cached rows of `base`, U per lane and round, the next round requested before this one is consumed (clamped,
    // never conditional: consume() gets `valid`)
    auto stream_rows = [&](const f16* base, auto&& consume) {
        if (nk <= 0) {
            return;
        }
        u32x4 ra[U], rb[U];
        auto  ld = [&](u32x4 (&r)[U], const int l0) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                int li = l0 + u * STEP + wid * KPI + grp;
                li     = li < nk ? li : nk - 1;
                r[u]   = *reinterpret_cast<const u32x4*>(base + (size_t)(t_beg + li) * DH + sub * 8);
            }
        };
        auto use = [&](const u32x4 (&r)[U], const int l0) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int li = l0 + u * STEP + wid * KPI + grp;
                consume(__builtin_bit_cast(f16x8, r[u]), li, li < nk);
            }
        };
        int l0 = 0;
        ld(ra, 0);
        for (;;) {
            ld(rb, l0 + U * STEP);
            use(ra, l0);
            l0 += U * STEP;
            if (l0 >= nk) {
                break;
            }
            ld(ra, l0 + U * STEP);
            use(rb, l0);
            l0 += U * STEP;
            if (l0 >= nk) {
                break;
            }
        }
    };

    // ---- phase 1: scores of every key of the split against all rows ----
    const float inv_sqrt_dh = rsqrtf((float)DH);
    {
        f16x8 qv[RM];
#pragma unroll
        for (int r = 0; r < RM; r++) {
            qv[r] = r < R ? *reinterpret_cast<const f16x8*>(s_q + r * DH + sub * 8) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        // jnew: the key is new key jnew (masked for the rows before it), -1: a cached key
        auto score = [&](const f16x8 kv, const int li, const bool valid, const int jnew) {
#pragma unroll
            for (int r = 0; r < RM; r++) {
                if (r < R) {
                    float a = 0.f;
                    a       = dot2(f16x2{qv[r][0], qv[r][1]}, f16x2{kv[0], kv[1]}, a);
                    a       = dot2(f16x2{qv[r][2], qv[r][3]}, f16x2{kv[2], kv[3]}, a);
                    a       = dot2(f16x2{qv[r][4], qv[r][5]}, f16x2{kv[4], kv[5]}, a);
                    a       = dot2(f16x2{qv[r][6], qv[r][7]}, f16x2{kv[6], kv[7]}, a);
                    a       = group_sum_dpp<LPK>(a) * inv_sqrt_dh;
                    if (valid && sub == 0) {
                        s_p[r * VA_LDP + li] = jnew > r ? -INFINITY : a;
                    }
                }
            }
        };
        stream_rows(kc, [&](const f16x8 kv, const int li, const bool valid) { score(kv, li, valid, -1); });
        if (owner) {
            for (int j0 = 0; j0 < R; j0 += STEP) {
                const int   j  = j0 + wid * KPI + grp;
                const int   jc = j < R ? j : R - 1;
                const f16x8 kv = *reinterpret_cast<const f16x8*>(s_k + jc * DH + sub * 8);
                score(kv, nk + j, j < R, jc);
            }
        }
    }
    __syncthreads();
    // ---- phase 2: per row, exp against the split's maximum and the local sum (a wave per row) ----
    for (int r = wid; r < R; r += 4) {
        float mx = -INFINITY;
        for (int i = lane; i < n_loc; i += 64) {
            mx = fmaxf(mx, s_p[r * VA_LDP + i]);
        }
        mx        = wave_max_dpp(mx);
        float sum = 0.f;
        for (int i = lane; i < n_loc; i += 64) {
            const float v = s_p[r * VA_LDP + i];
            const float e = (v == -INFINITY || mx == -INFINITY) ? 0.f : __expf(v - mx);
            s_p[r * VA_LDP + i] = e;
            sum += e;
        }
        sum = wave_sum_dpp(sum);
        if (lane == 0) {
            s_m[r] = mx;
            s_l[r] = sum;
        }
    }
    __syncthreads();
    // ---- phase 3: P.V (fp32 accumulate), every value row once for all rows ----
    float acc[RM][8];
#pragma unroll
    for (int r = 0; r < RM; r++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            acc[r][j] = 0.f;
        }
    }
    auto pv = [&](const f16x8 vv, const int li, const bool valid) {
        if (valid) {
#pragma unroll
            for (int r = 0; r < RM; r++) {
                if (r < R) {
                    const float pt = s_p[r * VA_LDP + li];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        acc[r][j] = fmaf(pt, (float)vv[j], acc[r][j]);
                    }
                }
            }
        }
    };
    stream_rows(vc, pv);
    if (owner) {
        for (int j0 = 0; j0 < R; j0 += STEP) {
            const int   j  = j0 + wid * KPI + grp;
            const int   jc = j < R ? j : R - 1;
            const f16x8 vv = *reinterpret_cast<const f16x8*>(s_v + jc * DH + sub * 8);
            pv(vv, nk + jc, j < R);  // (a masked pair holds probability 0)
        }
    }
    // fold the key groups of a wave (every lane gets the sum), then the four waves in wave order
#pragma unroll
    for (int r = 0; r < RM; r++) {
        if (r < R) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                acc[r][j] = across_groups_sum<LPK>(acc[r][j]);
            }
        }
    }
    for (int w = 0; w < 4; w++) {
        if (wid == w && grp == 0) {
#pragma unroll
            for (int r = 0; r < RM; r++) {
                if (r < R) {
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        float* o = &s_o[r * DH + sub * 8 + j];
                        *o       = (w == 0 ? 0.f : *o) + acc[r][j];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (nsplit == 1) {
        for (int i = threadIdx.x; i < R * DH; i += 256) {
            const int   r = i / DH, d = i % DH;
            const float inv = 1.f / (s_l[r] + 1.e-6f);
            p.ctx[(size_t)r * hl + h * DH + d] = (f16)(s_o[i] * inv);
        }
        return;
    }
    // ---- publish the partial {o[R][DH], max, sum} (write-through: the merger may sit on another XCD), then a ticket ----
    constexpr int NE      = DH + 2;
    unsigned*     tickets = reinterpret_cast<unsigned*>(p.ws);
    float*        parts   = reinterpret_cast<float*>(reinterpret_cast<char*>(p.ws) + (((size_t)p.nh * 4 + 255) & ~(size_t)255))
                   + (size_t)h * nsplit * R * NE;
    {
        va_gu32* mine = (va_gu32*)(parts + (size_t)sp * R * NE);
        for (int i = threadIdx.x; i < R * DH; i += 256) {
            const int r = i / DH, d = i % DH;
            __hip_atomic_store(mine + (size_t)r * NE + d, __float_as_uint(s_o[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if ((int)threadIdx.x < R) {
            __hip_atomic_store(mine + (size_t)threadIdx.x * NE + DH, __float_as_uint(s_m[threadIdx.x]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mine + (size_t)threadIdx.x * NE + DH + 1, __float_as_uint(s_l[threadIdx.x]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add((va_gu32*)(tickets + h), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last           = t == (unsigned)(nsplit - 1) ? 1 : 0;
        if (s_last) {
            __hip_atomic_store((va_gu32*)(tickets + h), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
        }
    }
    __syncthreads();
    if (!s_last) {
        return;
    }
    // ---- merger: every split's {max, sum} -> weights and the denominator per row, in split order ----
    const va_gu32* all = (const va_gu32*)parts;
    for (int i = threadIdx.x; i < R * nsplit; i += 256) {
        const int r = i / nsplit, s2 = i % nsplit;
        s_p[r * VA_LDP + s2]                = __uint_as_float(__hip_atomic_load(all + ((size_t)s2 * R + r) * NE + DH, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT));
        s_p[r * VA_LDP + VA_MAX_SPLIT + s2] = __uint_as_float(__hip_atomic_load(all + ((size_t)s2 * R + r) * NE + DH + 1,
                                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();
    if ((int)threadIdx.x < R) {
        const int r = threadIdx.x;
        float     m = -INFINITY;
        for (int s2 = 0; s2 < nsplit; s2++) {
            m = fmaxf(m, s_p[r * VA_LDP + s2]);
        }
        float L = 0.f;  // fixed-order sum over splits
        for (int s2 = 0; s2 < nsplit; s2++) {
            const float ms = s_p[r * VA_LDP + s2];
            const float w  = (ms == -INFINITY) ? 0.f : __expf(ms - m);
            L += w * s_p[r * VA_LDP + VA_MAX_SPLIT + s2];
            s_p[r * VA_LDP + s2] = w;
        }
        s_l[r] = L;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * DH; i += 256) {
        const int r = i / DH, d = i % DH;
        float     o = 0.f;
        for (int s2 = 0; s2 < nsplit; s2++) {
            o += s_p[r * VA_LDP + s2]
                 * __uint_as_float(__hip_atomic_load(all + ((size_t)s2 * R + r) * NE + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        const float inv = 1.f / (s_l[r] + 1.e-6f);
        p.ctx[(size_t)r * hl + h * DH + d] = (f16)(o * inv);
    }
}

void launch_verify_attention(const VerifyAttnParams& p, hipStream_t s)
{
    FTCF_CHECK_ARG(p.dh == 64 || p.dh == 128, "verify attention: size_per_head must be 64 or 128");
    FTCF_CHECK_ARG(p.R >= 1 && p.R <= VERIFY_MAX_ROWS, "verify attention: 1 <= rows <= 16");
    FTCF_CHECK_ARG(p.nh >= 1 && p.len >= 0 && p.len + p.R <= p.s_max, "verify attention: the rows do not fit the cache");
    FTCF_CHECK_ARG(p.rot >= 0 && p.rot % 2 == 0 && p.rot <= p.dh, "rotary_embedding_dim must be even and <= size_per_head");
    const int chunk  = verify_chunk(p.len, p.nh);
    const int nsplit = std::max(1, (p.len + chunk - 1) / chunk);
    FTCF_CHECK_ARG(nsplit <= VA_MAX_SPLIT && nsplit <= verify_max_split(p.nh, p.s_max), "verify attention: context too long");
    FTCF_CHECK_ARG(nsplit == 1 || p.ws != nullptr, "verify attention: no workspace");
    dim3 grid(p.nh, nsplit);
    if (p.dh == 128) {
        hipLaunchKernelGGL((k_verify_attention<128>), grid, dim3(256), 0, s, p, chunk, nsplit);
    }
    else {
        hipLaunchKernelGGL((k_verify_attention<64>), grid, dim3(256), 0, s, p, chunk, nsplit);
    }
    FTCF_HIP_CHECK(hipGetLastError());
}

__global__ void k_verify_rotary(float* table, int len, int rot)
{
    const int r = blockIdx.x, half = rot / 2;
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        float cs, sn;
        rotary_coef(j, rot, len + r, cs, sn);
        table[((size_t)r * half + j) * 2]     = cs;
        table[((size_t)r * half + j) * 2 + 1] = sn;
    }
}
void launch_verify_rotary(float* table, int len, int R, int rot, hipStream_t s)
{
    if (rot <= 0) {
        return;
    }
    hipLaunchKernelGGL(k_verify_rotary, dim3(R), dim3(64), 0, s, table, len, rot);
    FTCF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// drafting
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ngram_draft(const int* __restrict__ tokens, int n, const int* d_n, int K, int N,
                                                     const int* __restrict__ ext, int ext_base, int ext_len, int* draft, int* n_draft,
                                                     int* h_n_draft, const int* d_stop)
{
    __shared__ int s_best;
    if (d_n) {
        n = *d_n;
    }
    int cnt = 0;
    if (d_stop && *d_stop) {
        // every row has finished: nothing to draft
    }
    else if (ext) {
        if (threadIdx.x == 0) {
            const int j = n - ext_base;
            while (j >= 0 && cnt < K && j + cnt < ext_len && ext[j + cnt] >= 0) {
                draft[cnt] = ext[j + cnt];
                cnt++;
            }
        }
    }
    else {
        int fs = -1, fg = 0;
        for (int g = min(N, n - 1); g >= 1; g--) {
            if (threadIdx.x == 0) {
                s_best = -1;
            }
            __syncthreads();
            int best = -1;
            for (int s = threadIdx.x; s <= n - g - 1; s += 256) {  // (increasing: the last hit of a thread is its largest)
                bool eq = true;
                for (int i = 0; i < g; i++) {
                    eq &= tokens[s + i] == tokens[n - g + i];
                }
                if (eq) {
                    best = s;
                }
            }
            if (best >= 0) {
                atomicMax(&s_best, best);
            }
            __syncthreads();
            const int b = s_best;
            __syncthreads();
            if (b >= 0) {
                fs = b;
                fg = g;
                break;
            }
        }
        if (fs >= 0) {
            cnt = min(K, n - (fs + fg));
            for (int i = threadIdx.x; i < cnt; i += 256) {
                draft[i] = tokens[fs + fg + i];
            }
        }
    }
    if (threadIdx.x == 0) {
        *n_draft = cnt;
        if (h_n_draft) {
            *h_n_draft = cnt;
        }
    }
}

void launch_ngram_draft(const int* tokens, int n, const int* d_n, int K, int N, const int* ext, int ext_base, int ext_len, int* draft,
                        int* n_draft, int* h_n_draft, const int* d_stop, hipStream_t s)
{
    FTCF_CHECK_ARG(K >= 1 && K <= VERIFY_MAX_ROWS - 1 && N >= 1 && N <= 8, "draft: 1 <= K <= 15 and 1 <= N <= 8");
    FTCF_CHECK_ARG(draft && n_draft && (tokens || ext), "draft: NULL tensor");
    hipLaunchKernelGGL(k_ngram_draft, dim3(1), dim3(256), 0, s, tokens, n, d_n, K, N, ext, ext_base, ext_len, draft, n_draft, h_n_draft,
                       d_stop);
    FTCF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// the pass's input rows
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_verify_embed(f16* x, const f16* __restrict__ wte, const int* __restrict__ tokens,
                                                      const int* __restrict__ draft, int step, int H)
{
    const int  r   = blockIdx.x;
    const int  id  = r == 0 ? tokens[step - 1] : draft[r - 1];
    const f16* src = wte + (size_t)id * H;
    f16*       dst = x + (size_t)r * H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        *reinterpret_cast<f16x8*>(dst + i) = *reinterpret_cast<const f16x8*>(src + i);
    }
}
void launch_verify_embed(f16* x, const f16* wte, const int* tokens, const int* draft, int step, int R, int H, hipStream_t s)
{
    FTCF_CHECK_ARG(H % 8 == 0 && R >= 1 && R <= VERIFY_MAX_ROWS && step >= 1, "verify embed: bad arguments");
    hipLaunchKernelGGL(k_verify_embed, dim3(R), dim3(256), 0, s, x, wte, tokens, draft, step, H);
    FTCF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// The decode tail of a verify pass of a greedy request -- bare, or with stop words, log-probabilities or a streaming callback
//  -- in two launches:
//  * k_verify_slices : grid (VS_SLICES, R).  A workgroup reduces its contiguous slice of its row to {best value, best index,
//      slice max, sum of exp(v - slice max)} -- the partial of k_greedy_decode -- with VS_MAXE loads per thread in flight, chunk by
//      chunk for a slice longer than 256 * VS_MAXE logits (any V).  Against one workgroup per row (V / 256 DEPENDENT loads per
//      thread, 394 at V = 100864) a row is read by 32 workgroups at 13 independent loads per thread.
//  * k_verify_close  : one workgroup.  Every row's partials are merged in slice order by one thread (a fixed order: two launches
//      give identical bits), then the step is closed in one place: the accepted prefix, the tokens, their log-probabilities, the
//      end token, the stop words (stop_word_ends_at, the rule of decode_finish_body), the length criterion, the state words and
//      the pinned flags -- with the emitted tokens and the sequence length behind each, so that the host's callback copies nothing.
// No workgroup waits for another: the launch boundary orders the partials.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int VS_SLICES = VERIFY_ACCEPT_SLICES;
constexpr int VS_MAXE   = 16;  // logits per thread and chunk

__global__ __launch_bounds__(256) void k_verify_slices(const float* __restrict__ logits, const int V, float* part)
{
    __shared__ float redv[4], redm[4], reds[4];
    __shared__ int   redi[4];
    const int    r = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int    slice = (V + VS_SLICES - 1) / VS_SLICES;
    const int    i0 = blk * slice;
    const int    n  = max(0, min(slice, V - i0));
    const float* l  = logits + (size_t)r * V + i0;
    VI    best{-INFINITY, 0x7fffffff};
    float m = -FLT_MAX, se = 0.f;
    for (int c0 = 0; c0 < n; c0 += 256 * VS_MAXE) {
        float vals[VS_MAXE];
#pragma unroll
        for (int j = 0; j < VS_MAXE; j++) {  // (clamped, never conditional: all loads of the chunk are in flight together)
            const int i = c0 + (int)threadIdx.x + 256 * j;
            vals[j]     = l[i < n ? i : n - 1];
        }
        float cm = m;
#pragma unroll
        for (int j = 0; j < VS_MAXE; j++) {
            const int i = c0 + (int)threadIdx.x + 256 * j;
            if (i < n) {
                cm = fmaxf(cm, vals[j]);
                if (best.i == 0x7fffffff || better(vals[j], i0 + i, best.v, best.i)) {
                    best.v = vals[j];
                    best.i = i0 + i;
                }
            }
        }
        se *= __expf(m - cm);
#pragma unroll
        for (int j = 0; j < VS_MAXE; j++) {
            if (c0 + (int)threadIdx.x + 256 * j < n) {
                se += __expf(vals[j] - cm);
            }
        }
        m = cm;
    }
    // the wave's, then the four waves' in wave order
    const VI    wb = wave_best(best);
    const float wm = wave_max(m);
    const float ws = wave_sum(se * __expf(m - wm));  // (a thread without an element adds 0 * exp(.) = 0)
    if (lane == 0) {
        redv[wid] = wb.v;
        redi[wid] = wb.i;
        redm[wid] = wm;
        reds[wid] = ws;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float    bm, tot;
        const VI b = merge_waves<4>(redv, redi, redm, reds, 1, bm, tot);
        // write-through stores (agent scope: the closing workgroup may sit on another XCD)
        va_gu32* o = (va_gu32*)(part + ((size_t)r * VS_SLICES + blk) * 4);
        __hip_atomic_store(o + 0, __float_as_uint(n > 0 ? b.v : -INFINITY), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, (unsigned)(n > 0 ? b.i : 0x7fffffff), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 2, __float_as_uint(n > 0 ? bm : -FLT_MAX), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 3, __float_as_uint(n > 0 ? tot : 0.f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The LDS words of verify_close_stages that do not depend on the rows' tokens (VERIFY_MAX_ROWS of each): the drafts, -1 behind the
// last, and the stop marks.  The caller's next barrier publishes them.
__device__ __forceinline__ void verify_close_setup(const VerifyCloseParams& p, int* s_draft, int* s_stop)
{
    if ((int)threadIdx.x < VERIFY_MAX_ROWS) {
        s_draft[threadIdx.x] = (int)threadIdx.x < p.R - 1 ? p.draft[threadIdx.x] : -1;
        s_stop[threadIdx.x]  = 0;
    }
}

// Stages 1 - 4 of a pass's close, shared by k_verify_close and k_verify_sample_close: s_a[r] / s_lp[r] are row r's token and its
// log-probability, s_draft[] / s_stop[] verify_close_setup's, all in LDS behind a barrier.  Returns the tokens emitted (in thread
// 0; 0 in every other thread).
__device__ __forceinline__ int verify_close_stages(const VerifyCloseParams& p, const bool lp_on, const int* s_a, const float* s_lp,
                                                   const int* s_draft, int* s_stop, int* s_m_slot)
{
    const int R = p.R, st = p.step;
    int       emitted = 0;
    // ---- stage 1: m, the longest prefix of drafts the model agrees with ----
    if (threadIdx.x == 0) {
        int m = 0;
        while (m < R - 1 && s_draft[m] == s_a[m]) {
            m++;
        }
        *s_m_slot = m;
    }
    __syncthreads();
    const int m = *s_m_slot;
    // ---- the stop words at every candidate position st + i, i <= m (stop_criteria_kernels.cu:24-83): a (position, word) pair per
    // thread; tokens before st are the history, tokens from st on the ones this pass is about to write ----
    if (p.stop_words) {
        const int* words = p.stop_words;
        const int* offs  = words + p.stop_len;
        for (int w = threadIdx.x; w < (m + 1) * p.stop_len; w += 256) {
            const int i = w / p.stop_len, id = w % p.stop_len;
            if (stop_word_ends_at(words, offs, id, st + i, [&](const int pos) { return pos >= st ? s_a[pos - st] : p.output_ids[pos]; })) {
                atomicOr(&s_stop[i], 1);
            }
        }
    }
    __syncthreads();
    // ---- stages 2 - 4: the tokens in order, cut after the first one that finishes the row; the state words and the flags ----
    if (threadIdx.x == 0) {
        float     cum = p.cum_log_probs ? p.cum_log_probs[0] : 0.f;
        const int sl0 = p.seq_len[0];
        int       e = 0, fin = 0;
        for (int i = 0; i <= m && !fin; i++) {
            const int id = s_a[i], step = st + i;
            p.output_ids[step] = id;
            if (lp_on) {
                cum += s_lp[i];  // (sequential fp32 adds in token order: the sum of the stored values is cum_log_probs, bit for bit)
                if (p.output_log_probs) {
                    p.output_log_probs[step - p.max_input_len] = s_lp[i];
                }
            }
            fin = id == p.end_id;
            fin |= s_stop[i];
            fin |= step >= p.total_len;  // length_criterion (stop_criteria_kernels.cu:106-158), limit = total_len
            e++;
            if (p.h_flags) {
                p.h_flags[FLAG_SPEC_TOKENS + i]  = id;
                p.h_flags[FLAG_SPEC_SEQ_LEN + i] = sl0 + e;
            }
            if (p.tokens) {
                p.tokens[i] = id;
            }
        }
        const int acc = m < e ? m : e;  // drafts that became output tokens
        if (p.cum_log_probs && lp_on) {
            p.cum_log_probs[0] = cum;
        }
        p.seq_len[0]  = sl0 + e;
        p.finished[0] = (uint8_t)fin;
        if (p.emitted) {
            *p.emitted = e;
        }
        if (p.accepted) {
            *p.accepted = acc;
        }
        if (p.state) {
            p.state->all_finished = fin;
            p.state->steps_done += e;
            p.state->step = st + e;
        }
        if (p.h_flags) {  // (the host reads them behind a synchronisation of the stream)
            p.h_flags[FLAG_LAST_STEP]     = st + e - 1;
            p.h_flags[FLAG_SPEC_EMITTED]  = e;
            p.h_flags[FLAG_SPEC_ACCEPTED] = acc;
            __threadfence_system();
            p.h_flags[FLAG_ALL_FINISHED] = fin;
        }
        emitted = e;
    }
    return emitted;
}

__global__ __launch_bounds__(256) void k_verify_close(const VerifyCloseParams p, const float* part)
{
    constexpr int RM = VERIFY_MAX_ROWS;
    __shared__ unsigned s_part[RM * VS_SLICES * 4];
    __shared__ int   s_a[RM], s_draft[RM], s_stop[RM];
    __shared__ float s_lp[RM];
    __shared__ int   s_m;
    const int  R = p.R;
    const bool lp_on = p.cum_log_probs || p.output_log_probs;
    {  // every row's partials, requested together
        const va_gu32* q = (const va_gu32*)part;
        for (int i = threadIdx.x; i < R * VS_SLICES * 4; i += 256) {
            s_part[i] = __hip_atomic_load(q + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        verify_close_setup(p, s_draft, s_stop);
    }
    __syncthreads();
    // ---- a[r] and its log-probability: row r's partials in slice order, by one thread (merge_waves' order, written out: a
    // slice's four words lie together as stored, the index among the floats, and are read as what they are) ----
    if ((int)threadIdx.x < R) {
        const unsigned* q = s_part + threadIdx.x * VS_SLICES * 4;
        VI    b{__uint_as_float(q[0]), (int)q[1]};
        float M = __uint_as_float(q[2]);
        for (int sl = 1; sl < VS_SLICES; sl++) {
            const float v = __uint_as_float(q[sl * 4]);
            const int   i = (int)q[sl * 4 + 1];
            if (better(v, i, b.v, b.i)) {
                b.v = v;
                b.i = i;
            }
            M = fmaxf(M, __uint_as_float(q[sl * 4 + 2]));
        }
        float tot = 0.f;
        for (int sl = 0; sl < VS_SLICES; sl++) {
            tot += __uint_as_float(q[sl * 4 + 3]) * __expf(__uint_as_float(q[sl * 4 + 2]) - M);
        }
        s_a[threadIdx.x]  = (b.i == 0x7fffffff || b.i < 0) ? 0 : b.i;
        s_lp[threadIdx.x] = lp_on ? logf(__expf(b.v - M) / (tot + 1e-6f)) : 0.f;
    }
    __syncthreads();
    (void)verify_close_stages(p, lp_on, s_a, s_lp, s_draft, s_stop, &s_m);
}

size_t verify_close_workspace_bytes()
{
    return (size_t)VERIFY_MAX_ROWS * VS_SLICES * 4 * sizeof(float);
}

// what either close asks of a pass's parameters (its own workspace apart); who: the prefix of its messages
static void check_close_params(const VerifyCloseParams& p, const std::string& who)
{
    FTCF_CHECK_ARG(p.R >= 1 && p.R <= VERIFY_MAX_ROWS && p.V >= 1, who + ": 1 <= rows <= 16, vocabulary >= 1");
    FTCF_CHECK_ARG(p.logits && p.output_ids && p.finished && p.seq_len && (p.R == 1 || p.draft), who + ": NULL tensor");
    FTCF_CHECK_ARG(p.step >= 1 && p.max_input_len >= 0 && p.step >= p.max_input_len && p.step + p.R <= p.total_len,
                   who + ": the rows' positions step .. step + R - 1 must lie in [max(1, max_input_len), total_len)");
    FTCF_CHECK_ARG(!p.stop_words || p.stop_len >= 1, who + ": stop_words needs stop_len >= 1");
}

void launch_verify_close(const VerifyCloseParams& p, hipStream_t s)
{
    check_close_params(p, "verify accept");
    FTCF_CHECK_ARG(p.ws, "verify accept: NULL tensor");
    hipLaunchKernelGGL(k_verify_slices, dim3(VS_SLICES, p.R), dim3(256), 0, s, p.logits, p.V, p.ws);
    hipLaunchKernelGGL(k_verify_close, dim3(1), dim3(256), 0, s, p, (const float*)p.ws);
    FTCF_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// The tail of a verify pass of a TOP-K SAMPLED request, in three launches.  The engine's random numbers are
// counter based (ftcf_uniform(seed, 0, draw)): the n-th generated token of a request consumes draw n whatever happened before, and
// row i of a pass is reached only behind i accepted rows, i.e. behind exactly i draws.  So row i is SAMPLED with draw
// draw_counter + i, draft i is accepted only when it is the sampled token, and the counter advances by the tokens emitted: the
// output is the plain sampled run's token sequence for the same seed.
//  * k_verify_topk_slices  : grid (VS_SLICES, R), the first half of k_topk_decode for row blockIdx.y: the slice's logits in registers
//      (multiplied by k_decode_prep's temperature factor on load; the buffer is left alone), its {max, sum of exponentials} when
//      log-probabilities are wanted, its k best as a set (slice_select; block_best for one), written through (agent scope).
//  * k_verify_pick         : grid (R).  Row r's workgroup merges the 32 candidate sets as k_topk_decode's finishing workgroup does
//      (the same functions under the same conditions), one thread draws with draw_counter[0] + r (topk_draw_at) and leaves the token
//      and logf(probability), commit_pick's value.
//  * k_verify_sample_close : one workgroup, verify_close_stages on the sampled tokens, then draw_counter[0] += emitted.
// No workgroup waits for another: the launch boundaries order candidates, picks and the counter.  Every merge order is fixed: two
// launches give identical bits.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int VT_MAXE = 16;  // logits per thread: V <= 32 * 256 * 16 = 131072 (VERIFY_SAMPLE_MAX_V)
constexpr int VT_MAXK = VERIFY_SAMPLE_MAX_K;
constexpr size_t VT_CAND  = (size_t)VERIFY_MAX_ROWS * VS_SLICES * VT_MAXK;  // candidate values, then as many ids ...
constexpr size_t VT_STATS = (size_t)VERIFY_MAX_ROWS * VS_SLICES * 2;        // ... {max, sum of exponentials} per slice ...
constexpr size_t VT_PICKS = (size_t)VERIFY_MAX_ROWS * 2;                    // ... every row's token, then its log-probability

__global__ __launch_bounds__(256) void k_verify_topk_slices(const float* __restrict__ logits, const int V, const int k, const int lp_on,
                                                            const int apply_temperature, const float temperature, float* ws)
{
    __shared__ float redv[4];
    __shared__ int   redi[4];
    __shared__ int   hist[256];
    __shared__ int   hist8[8][257];
    __shared__ int   s_sel[4];
    const int    r = blockIdx.y, blk = blockIdx.x;
    const int    slice = (V + VS_SLICES - 1) / VS_SLICES;
    const int    i0 = blk * slice;
    const int    n  = max(0, min(slice, V - i0));
    const float* l  = logits + (size_t)r * V + i0;
    float*       ov = ws + ((size_t)r * VS_SLICES + blk) * VT_MAXK;
    int*         oi = reinterpret_cast<int*>(ws + VT_CAND) + ((size_t)r * VS_SLICES + blk) * VT_MAXK;
    const float  scale = apply_temperature ? 1.0f / (temperature + 1e-6f) : 1.f;  // sampling_penalty_kernels.cu:117-147
    float        vals[VT_MAXE], lmax;
    const int    ne   = n > (int)threadIdx.x ? (n - (int)threadIdx.x + 255) / 256 : 0;
    const VI     best = slice_load(vals, l, ne, -1, lmax, scale);
    if (lp_on) {  // {max, sum of exp(v - max)} of the slice for the row's soft-max
        float       m;
        const float sum = slice_stats(vals, ne, lmax, redv, m);
        if (threadIdx.x == 0) {
            va_gu32* st = (va_gu32*)(ws + 2 * VT_CAND + ((size_t)r * VS_SLICES + blk) * 2);
            __hip_atomic_store(st + 0, __float_as_uint(n > 0 ? m : -FLT_MAX), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(st + 1, __float_as_uint(n > 0 ? sum : 0.f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const int ke = k < n ? k : n;  // candidates this slice can supply
    for (int i = ke + threadIdx.x; i < k; i += 256) {
        put_cand<true>(ov, oi, i, -INFINITY, -1);
    }
    if (ke == 1) {
        const VI b = block_best(best, redv, redi);
        if (threadIdx.x == 0) {
            put_cand<true>(ov, oi, 0, b.v, i0 + b.i);
        }
    }
    else if (ke > 1) {
        slice_select<VT_MAXE, true>(vals, ne, n, ke, l, i0, ov, oi, hist8, hist, s_sel, redi, false, -1, scale);
    }
}

__global__ __launch_bounds__(256) void k_verify_pick(float* ws, const int k, const int lp_on, const uint64_t seed,
                                                     const uint64_t* __restrict__ draw_counter, const float p_topk)
{
    __shared__ float redv[4];
    __shared__ int   redi[4];
    __shared__ int   hist[256];
    __shared__ int   hist8[8][257];
    __shared__ int   s_sel[4];
    __shared__ float sv[VS_SLICES * VT_MAXK];
    __shared__ int   si[VS_SLICES * VT_MAXK];
    __shared__ float tv[VT_MAXK];
    __shared__ int   ti[VT_MAXK];
    const int row = blockIdx.x;
    int       n2 = 1;
    while (n2 < VS_SLICES * k) {
        n2 <<= 1;
    }
    int k2 = 1;
    while (k2 < k) {
        k2 <<= 1;
    }
    {
        const va_gu32* cv = (const va_gu32*)(ws + (size_t)row * VS_SLICES * VT_MAXK);
        const va_gu32* ci = (const va_gu32*)(ws + VT_CAND + (size_t)row * VS_SLICES * VT_MAXK);
        // (all of a thread's candidates requested together: one round trip, not eight)
        constexpr int NC = VS_SLICES * VT_MAXK / 256;
        unsigned      rv[NC], ri[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            const int c  = threadIdx.x + 256 * j;
            const int cc = c < VS_SLICES * k ? c : 0;
            const int q = cc / k, e = cc - q * k;
            ri[j] = __hip_atomic_load(ci + q * VT_MAXK + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rv[j] = __hip_atomic_load(cv + q * VT_MAXK + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int j = 0; j < NC; j++) {
            const int c = threadIdx.x + 256 * j;
            if (c < n2) {
                const bool ok = c < VS_SLICES * k && (int)ri[j] >= 0;
                sv[c]         = ok ? __uint_as_float(rv[j]) : -INFINITY;
                si[c]         = ok ? (int)ri[j] : 0x7fffffff;
            }
        }
    }
    if (k > 1 && n2 >= 4 * k2) {
        union_topk(sv, si, n2, k, k2, tv, ti, hist, s_sel, redi, hist8);
    }
    else if (k > 1) {
        bitonic_sort_best_first(sv, si, n2);
    }
    else {
        best_of_slices(sv, si, VS_SLICES, redv, redi);
    }
    // ---- top-k layer: sv / si [0, k) are the row's k best; the draw of the token this row would be ----
    if (threadIdx.x == 0) {
        const va_gu32* st   = (const va_gu32*)(ws + 2 * VT_CAND + (size_t)row * VS_SLICES * 2);
        const int      pick = topk_draw_at<VS_SLICES>(lp_on != 0, seed, draw_counter[0] + (uint64_t)row, p_topk, k, sv, [&](const int i) {
            return __uint_as_float(__hip_atomic_load(st + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        });
        int id = si[pick];
        if (id == 0x7fffffff || id < 0) {  // (commit_pick's rule)
            id = 0;
        }
        va_gu32* out = (va_gu32*)(ws + 2 * VT_CAND + VT_STATS);
        __hip_atomic_store(out + row, (unsigned)id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(out + VERIFY_MAX_ROWS + row, __float_as_uint(lp_on ? logf(sv[pick]) : 0.f), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_verify_sample_close(const VerifyCloseParams p, const float* ws, uint64_t* draw_counter)
{
    constexpr int RM = VERIFY_MAX_ROWS;
    __shared__ int   s_a[RM], s_draft[RM], s_stop[RM];
    __shared__ float s_lp[RM];
    __shared__ int   s_m;
    const int  R = p.R;
    const bool lp_on = p.cum_log_probs || p.output_log_probs;
    if ((int)threadIdx.x < RM) {
        const int      r = threadIdx.x, rc = r < R ? r : 0;
        const va_gu32* q = (const va_gu32*)(ws + 2 * VT_CAND + VT_STATS);
        const unsigned id = __hip_atomic_load(q + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned lp = __hip_atomic_load(q + RM + rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_a[r]     = r < R ? (int)id : 0;
        s_lp[r]    = r < R ? __uint_as_float(lp) : 0.f;
    }
    verify_close_setup(p, s_draft, s_stop);
    __syncthreads();
    const int e = verify_close_stages(p, lp_on, s_a, s_lp, s_draft, s_stop, &s_m);
    if (threadIdx.x == 0) {
        draw_counter[0] += (uint64_t)e;  // one draw per emitted token: the rows behind the accepted run consumed none
    }
}

size_t verify_sample_workspace_bytes()
{
    return (2 * VT_CAND + VT_STATS + VT_PICKS) * sizeof(float);
}

void launch_verify_sample(const VerifySampleParams& q, hipStream_t s)
{
    const VerifyCloseParams& p = q.c;
    check_close_params(p, "verify sample");
    FTCF_CHECK_ARG(q.top_k >= 1 && q.top_k <= VERIFY_SAMPLE_MAX_K && p.V <= VERIFY_SAMPLE_MAX_V,
                   "verify sample: 1 <= top_k <= 64, vocabulary <= 131072");
    FTCF_CHECK_ARG(q.ws && q.draw_counter, "verify sample: NULL tensor");
    const int lp_on = (p.cum_log_probs || p.output_log_probs) ? 1 : 0;
    hipLaunchKernelGGL(k_verify_topk_slices, dim3(VS_SLICES, p.R), dim3(256), 0, s, p.logits, p.V, q.top_k, lp_on, q.apply_temperature,
                       q.temperature, q.ws);
    hipLaunchKernelGGL(k_verify_pick, dim3(p.R), dim3(256), 0, s, q.ws, q.top_k, lp_on, q.random_seed, (const uint64_t*)q.draw_counter,
                       q.top_p_topk);
    hipLaunchKernelGGL(k_verify_sample_close, dim3(1), dim3(256), 0, s, p, (const float*)q.ws, q.draw_counter);
    FTCF_HIP_CHECK(hipGetLastError());
}

}  // namespace ftcf
