// The stand-alone C ABI of include/ftcf.h: everything that is not an engine (`ftcf_gptneox_*`, engine.hip), a communicator
// (comm.hip) or a batcher (batcher.hip) -- the error text, version and device count, the host / device quantiser entries and the
// kernel-level entry points (GEMMs, LM head, LayerNorms, attention, paged copies, one dynamic-decode / logit-process /
// beam-search step).  Thin wrappers: argument checks, then exactly the launcher the engine calls.
#include "engine.hip.h"

thread_local std::string g_last_error;

extern "C" const char* ftcf_last_error(void)
{
    return g_last_error.c_str();
}
extern "C" int ftcf_version(void)
{
    return FTCF_VERSION;
}
extern "C" int ftcf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}


// ---------------------------------------------------------------------------------------------------------------
// host quantiser entry points (libth_common counterpart)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int ftcf_symmetric_quantize_int8(const void* weight, ftcf_dtype dtype, size_t E, size_t K, size_t N,
                                            int8_t* out_q, void* out_scale)
{
    return guarded([&] { host_symmetric_quantize_int8(weight, (int)dtype, E, K, N, out_q, out_scale); });
}
extern "C" size_t ftcf_symmetric_quantize_int8_device_workspace(size_t E, size_t N)
{
    return symmetric_quantize_int8_workspace_bytes(E, N);
}
extern "C" int ftcf_symmetric_quantize_int8_device(const void* weight, ftcf_dtype dtype, size_t E, size_t K, size_t N,
                                                   int8_t* out_q, void* out_scale, void* workspace, size_t workspace_bytes,
                                                   void* stream)
{
    return guarded([&] {
        require_device();
        check_symmetric_quantize_args(weight, (int)dtype, E, K, N, out_q, out_scale);  // (the host function's rule)
        FTCF_CHECK_ARG(workspace != nullptr, "NULL workspace");
        FTCF_CHECK_ARG(workspace_bytes >= symmetric_quantize_int8_workspace_bytes(E, N), "workspace too small");
        FTCF_CHECK_ARG(((uintptr_t)weight | (uintptr_t)out_q | (uintptr_t)out_scale | (uintptr_t)workspace) % 16 == 0,
                       "device quantiser pointers must be 16-byte aligned");
        launch_symmetric_quantize_int8(weight, (int)dtype, E, K, N, out_q, out_scale, workspace, (hipStream_t)stream);
    });
}
extern "C" int ftcf_int8_rowmajor_to_tiled(const int8_t* q, size_t K, size_t N, int8_t* out)
{
    return guarded([&] { host_int8_rowmajor_to_tiled(q, K, N, out); });
}
extern "C" int ftcf_int8_tiled_to_rowmajor(const int8_t* q, size_t K, size_t N, int8_t* out)
{
    return guarded([&] { host_int8_tiled_to_rowmajor(q, K, N, out); });
}
extern "C" int ftcf_int8_cuda_sm80_to_rowmajor(const int8_t* q, size_t K, size_t N, int8_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(q && out && K % 64 == 0 && N % 2 == 0, "SM80 int8 layout needs K % 64 == 0 and N % 2 == 0");
        host_int8_cuda_sm80_to_rowmajor(q, K, N, out);
    });
}
extern "C" int ftcf_int8_rowmajor_to_cuda_sm80(const int8_t* q, size_t K, size_t N, int8_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(q && out && K % 64 == 0 && N % 2 == 0, "SM80 int8 layout needs K % 64 == 0 and N % 2 == 0");
        host_int8_rowmajor_to_cuda_sm80(q, K, N, out);
    });
}
extern "C" int ftcf_fp16_rowmajor_to_tiled(const void* w, size_t K, size_t N, void* out, void* stream)
{
    return guarded([&] {
        require_device();
        launch_fp16_rowmajor_to_tiled((const f16*)w, K, N, (f16*)out, (hipStream_t)stream);
    });
}

// ---------------------------------------------------------------------------------------------------------------
// kernel-level entry points
// ---------------------------------------------------------------------------------------------------------------
// the stand-alone GEMM entry points carry no workspace argument (the reference's runner takes one from its caller:
// fpA_intB_gemm.h gemm(..., workspace_ptr, workspace_bytes)): one split-K workspace per (device, stream) that has called with
// 17..768 rows, kept for the life of the process
static float* abi_gemm_workspace(int m, hipStream_t s)
{
    if (m <= 16 || m > gemm_tiled_splitk_max_m()) {
        return nullptr;  // (only the split-K form of 17..768 rows uses it)
    }
    static std::mutex                                    mu;
    static std::map<std::pair<int, hipStream_t>, float*> ws;
    int                                                  dev = 0;
    FTCF_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    float*&                     p = ws[{dev, s}];
    if (!p) {
        FTCF_HIP_CHECK(hipMalloc(&p, gemm_tiled_workspace_bytes()));
        // only the tickets need zeros (the partial tiles are written before they are read), and on the CALLER's stream: a
        // null-stream memset is not ordered with a launch on a non-blocking stream
        FTCF_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char*>(p) + gemm_tiled_workspace_bytes() - gemm_tiled_ticket_bytes(), 0,
                                      gemm_tiled_ticket_bytes(), s));
    }
    return p;
}

extern "C" int ftcf_fpA_intB_gemm(const void* A, const int8_t* B, const void* scales, const void* bias, ftcf_act act,
                                  void* C, int m, int n, int k, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(k % 64 == 0 && n % 16 == 0 && m >= 1, "fpA_intB GEMM needs k % 64 == 0, n % 16 == 0");
        gemm_dispatch((const f16*)A, B, (const f16*)scales, (const f16*)bias, (int)act, (f16*)C, m, n, k, true,
                      (hipStream_t)stream, nullptr, 0, 256, nullptr, nullptr, abi_gemm_workspace(m, (hipStream_t)stream));
    });
}
extern "C" int ftcf_fp16_gemm(const void* A, const void* W, const void* bias, ftcf_act act, void* C, int m, int n,
                              int k, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(k % 64 == 0 && n % 16 == 0 && m >= 1, "fp16 GEMM needs k % 64 == 0, n % 16 == 0");
        gemm_dispatch((const f16*)A, W, nullptr, (const f16*)bias, (int)act, (f16*)C, m, n, k, false,
                      (hipStream_t)stream, nullptr, 0, 256, nullptr, nullptr, abi_gemm_workspace(m, (hipStream_t)stream));
    });
}
extern "C" int ftcf_gemm_tiled_plan(int m, int n, int k, int int8, int has_workspace, ftcf_gemm_plan* out)
{
    return guarded([&] {  // (host only: no require_device)
        FTCF_CHECK_ARG(out && m >= 1 && n >= 16 && k >= 64 && k % 64 == 0 && n % 16 == 0, "GEMM plan needs k % 64 == 0, n % 16 == 0");
        const GemmTiledPlan p = gemm_tiled_plan(m, n, k, int8 != 0, has_workspace != 0);
        *out = ftcf_gemm_plan{p.family, p.tile_rows, p.gx, p.gy, p.slices, p.steps_per_slice, p.ring, p.prefetch, p.two_per_cu, p.lone,
                              p.grid};
    });
}
extern "C" int ftcf_lm_head(const void* A, const void* W, float* logits, int m, int n, int k, int ldc, void* stream)
{
    return guarded([&] {
        require_device();
        lm_head_dispatch((const f16*)A, (const f16*)W, logits, m, n, k, ldc, (hipStream_t)stream);
    });
}
// the forms the engine launches for batched decode, short prompt phases, the batcher and the verify pass, one call each
// (thin wrappers: argument checks, then exactly the launcher the engine calls)
extern "C" size_t ftcf_gemm_smallm_workspace_bytes(int m, int n, int k, int int8)
{
    return gemm_smallm_workspace_bytes(m, n, k, int8 != 0);
}
extern "C" size_t ftcf_gemm_smallm_ticket_bytes(void)
{
    return gemm_smallm_ticket_bytes();
}
extern "C" int ftcf_gemm_smallm_group(const ftcf_smallm_problem* problems, int np, int m, int int8, void* workspace,
                                      size_t partial_bytes, size_t partial_offset, const int* d_step, unsigned* launch_counter,
                                      void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(problems && np >= 1 && np <= 2 && m >= 1 && m <= 16 && workspace && launch_counter,
                       "small-m GEMM group: 1..2 problems, 1..16 rows, a workspace and a launch counter");
        FTCF_CHECK_ARG(partial_bytes % 8 == 0 && partial_offset % 8 == 0 && partial_offset <= partial_bytes,
                       "small-m GEMM group: partial_bytes / partial_offset are multiples of 8, offset <= bytes");
        SmallmDesc d[2];
        for (int i = 0; i < np; i++) {
            const ftcf_smallm_problem& q = problems[i];
            FTCF_CHECK_ARG(q.A && q.W && q.C && (!int8 || q.scale), "small-m GEMM group: NULL tensor");
            FTCF_CHECK_ARG(q.n >= 16 && q.k >= 64 && q.n % 16 == 0 && q.k % 64 == 0, "small-m GEMM group: n % 16 == 0, k % 64 == 0");
            FTCF_CHECK_ARG((q.act == 0 || q.act == 1) && (q.act == 0 || q.bias), "small-m GEMM group: act 0 / 1 (1 needs a bias)");
            d[i] = SmallmDesc{(const f16*)q.A, q.W, (const f16*)q.scale, (const f16*)q.bias, q.act, (f16*)q.C, q.n, q.k};
        }
        launch_gemm_smallm_group(d, np, (float*)workspace, partial_bytes, m, int8 != 0, (hipStream_t)stream, d_step, launch_counter,
                                 partial_offset);
    });
}
extern "C" int ftcf_residual_dual_layernorm(void* x, const void* ffn, const void* attn, const void* bias, int tp, int inplace_variant,
                                            const void* g1, const void* b1, const void* g2, const void* b2, void* out1, void* out2,
                                            int m, int n, float eps, int bias_mul, int sum_mul, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(x && m >= 0 && n >= 8, "residual + dual LayerNorm: x [m, n]");
        FTCF_CHECK_ARG(!ffn || (attn && bias && tp >= 1 && bias_mul >= 1 && sum_mul >= 1),
                       "residual + dual LayerNorm: the residual needs ffn, attn, bias, tp >= 1 and multipliers >= 1");
        FTCF_CHECK_ARG(!g1 || (b1 && g2 && b2 && out1 && out2), "residual + dual LayerNorm: both LayerNorms or none");
        launch_residual_dual_ln((f16*)x, (const f16*)ffn, (const f16*)attn, (const f16*)bias, tp, inplace_variant, (const f16*)g1,
                                (const f16*)b1, (const f16*)g2, (const f16*)b2, (f16*)out1, (f16*)out2, m, n, eps,
                                (hipStream_t)stream, bias_mul, sum_mul);
    });
}
extern "C" int ftcf_add_bias_residual(void* out, const void* a, const void* b, const void* bias, int m, int n, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(out && a && b && m >= 0 && n >= 1, "bias + residual: out, a, b [m, n]");
        launch_add_bias_residual((f16*)out, (const f16*)a, (const f16*)b, (const f16*)bias, m, n, (hipStream_t)stream);
    });
}
// (dynamic LDS a launch may ask for without raising the kernel's limit)
static constexpr size_t ABI_MAX_DYNAMIC_LDS = 64 * 1024;
extern "C" int ftcf_lm_head_layernorm(const void* A, const void* W, const void* gamma, const void* beta, float eps, const int* d_stop,
                                      float* logits, int m, int n, int k, int ldc, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(A && W && logits && gamma && beta, "LM head with LayerNorm: NULL tensor");
        FTCF_CHECK_ARG(m >= 1 && m <= 4 && n >= 1 && k >= 8 && ldc >= n, "LM head with LayerNorm: 1..4 rows, ldc >= n");
        FTCF_CHECK_ARG((size_t)m * (k + 8) * 2 + 64 <= ABI_MAX_DYNAMIC_LDS, "LM head with LayerNorm: the rows do not fit the LDS");
        launch_lm_head((const f16*)A, (const f16*)W, logits, m, n, k, ldc, (hipStream_t)stream, (const f16*)gamma, (const f16*)beta,
                       eps, d_stop);
    });
}
extern "C" int ftcf_ln_gemv(const ftcf_ln_gemv_args* a, int m, int int8, int wpg, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a && a->x && m >= 1 && m <= 4 && wpg >= 0 && wpg <= 4, "LN + GEMV: 1..4 rows, wpg 0..4");
        FTCF_CHECK_ARG(a->K >= 64 && a->K % 64 == 0 && a->N0 >= 0 && a->N1 >= 0 && a->N0 % 16 == 0 && a->N1 % 16 == 0
                           && a->N0 + a->N1 > 0,
                       "LN + GEMV: K % 64 == 0, N0 % 16 == 0, N1 % 16 == 0");
        FTCF_CHECK_ARG(a->N0 == 0 || (a->gamma0 && a->beta0 && a->W0 && a->out0 && (!int8 || a->scale0)), "LN + GEMV: segment 0 tensors");
        FTCF_CHECK_ARG(a->N1 == 0 || (a->gamma1 && a->beta1 && a->W1 && a->out1 && a->bias1 && (!int8 || a->scale1)),
                       "LN + GEMV: segment 1 tensors");
        FTCF_CHECK_ARG((size_t)m * (a->K + 8) * 2 + (size_t)(2 * 4 + 4 * m * 16) * 4 + 64 <= ABI_MAX_DYNAMIC_LDS,
                       "LN + GEMV: the rows do not fit the LDS");
        LnGemvParams p{};
        p.x = (const f16*)a->x;
        p.gamma0 = (const f16*)a->gamma0;
        p.beta0 = (const f16*)a->beta0;
        p.gamma1 = (const f16*)a->gamma1;
        p.beta1 = (const f16*)a->beta1;
        p.W0 = a->W0;
        p.W1 = a->W1;
        p.scale0 = (const f16*)a->scale0;
        p.scale1 = (const f16*)a->scale1;
        p.bias1 = (const f16*)a->bias1;
        p.out0 = (f16*)a->out0;
        p.out1 = (f16*)a->out1;
        p.K = a->K;
        p.NT0 = a->N0 / 16;
        p.NT1 = a->N1 / 16;
        p.blocks0 = (p.NT0 + 3) / 4;
        p.blocks1 = (p.NT1 + 3) / 4;
        p.eps = a->eps;
        if (wpg > 0) {
            launch_ln_gemv_group(p, int8 != 0, m, wpg, (hipStream_t)stream);
        }
        else {
            launch_ln_gemv(p, int8 != 0, m, (hipStream_t)stream);
        }
    });
}
extern "C" size_t ftcf_residual_gemv_workspace_bytes(int N, int m, int Q)
{
    return chunk_workspace_bytes(N, m, Q);
}
extern "C" int ftcf_residual_gemv(const ftcf_residual_gemv_args* a, int m, int int8, int Q, void* granules, size_t granule_bytes,
                                  const int* d_step, int step, int salt, void* stream)
{
    return guarded([&] {
        require_device();
        const int tk = int8 ? TILE_K_I8 : TILE_K_F16;
        FTCF_CHECK_ARG(a && m >= 1 && m <= 4 && Q >= 0 && Q <= 8, "residual GEMV: 1..4 rows, Q 0..8");
        FTCF_CHECK_ARG(a->x_a && a->x_b && a->W_a && a->W_b && a->bias && a->x_in && a->out && (!int8 || (a->scale_a && a->scale_b)),
                       "residual GEMV: NULL tensor");
        FTCF_CHECK_ARG(a->N >= 16 && a->N % 16 == 0 && a->K_a >= tk && a->K_b >= tk && a->K_a % tk == 0 && a->K_b % tk == 0 && a->tp >= 1,
                       "residual GEMV: N % 16 == 0, K_a / K_b whole tiles (64 int8, 32 fp16), tp >= 1");
        if (Q == 0) {  // one workgroup per column group, its waves split the two segments
            SplitKParams c{};
            c.x_a = (const f16*)a->x_a;
            c.x_b = (const f16*)a->x_b;
            c.W_a = a->W_a;
            c.W_b = a->W_b;
            c.scale_a = (const f16*)a->scale_a;
            c.scale_b = (const f16*)a->scale_b;
            c.bias = (const f16*)a->bias;
            c.x_in = (const f16*)a->x_in;
            c.out = (f16*)a->out;
            c.N = a->N;
            c.KT_a = a->K_a / tk;
            c.KT_b = a->K_b / tk;
            c.tp = a->tp;
            c.inplace_variant = a->inplace_variant;
            plan_splitk(c, int8 != 0, m, 10);
            FTCF_CHECK_ARG((size_t)c.nwaves * m * c.slice_halves * 2 + (size_t)c.nwaves * m * 16 * 4 <= ABI_MAX_DYNAMIC_LDS,
                           "residual GEMV: the x slices do not fit the LDS");
            launch_gemv_splitk(c, int8 != 0, m, EPI_RESIDUAL, (hipStream_t)stream);
            return;
        }
        ChunkParams c{};
        c.x_a = (const f16*)a->x_a;
        c.x_b = (const f16*)a->x_b;
        c.W_a = a->W_a;
        c.W_b = a->W_b;
        c.scale_a = (const f16*)a->scale_a;
        c.scale_b = (const f16*)a->scale_b;
        c.bias = (const f16*)a->bias;
        c.x_in = (const f16*)a->x_in;
        c.out = (f16*)a->out;
        c.N = a->N;
        c.KT_a = a->K_a / tk;
        c.KT_b = a->K_b / tk;
        c.Q = Q;
        c.T = (c.KT_a + c.KT_b + Q - 1) / Q;
        c.tp = a->tp;
        c.inplace_variant = a->inplace_variant;
        c.gran = (unsigned long long*)granules;
        c.d_step = d_step;
        c.step = step;
        c.salt = salt;
        FTCF_CHECK_ARG(Q == 1 || (granules && granule_bytes >= chunk_workspace_bytes(a->N, m, Q)), "residual GEMV: granule workspace too small");
        FTCF_CHECK_ARG(salt >= 0 && salt < 1024, "residual GEMV: salt 0..1023");
        FTCF_CHECK_ARG((size_t)2 * m * ((c.T / 2 + 2) * tk + 8) * 2 + (size_t)2 * 2 * m * 16 * 4 <= ABI_MAX_DYNAMIC_LDS,
                       "residual GEMV: the x slices do not fit the LDS");
        launch_gemv_chunked(c, int8 != 0, m, (hipStream_t)stream);
    });
}
extern "C" int ftcf_lm_head_log_probs(const void* A, const void* W, const int* targets, float* log_probs, float* row_logsumexp, int m,
                                      int n, int k, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(A && W && targets && log_probs, "NULL tensor");
        launch_lm_head_log_probs((const f16*)A, (const f16*)W, targets, log_probs, row_logsumexp, m, n, k,
                                 lm_head_log_probs_workspace(m, n, (hipStream_t)stream), (hipStream_t)stream);
    });
}
extern "C" int ftcf_layernorm(const void* x, const void* gamma, const void* beta, void* out, int m, int n, float eps,
                              ftcf_dtype dtype, void* stream)
{
    return guarded([&] {
        require_device();
        launch_layernorm(x, gamma, beta, out, m, n, eps, dtype == FTCF_FP16, (hipStream_t)stream);
    });
}
extern "C" int ftcf_add_bias_attn_ffn_residual(void* out, const void* ffn, const void* attn, const void* in,
                                               const void* bias, int m, int n, int tp, int inplace_variant,
                                               ftcf_dtype dtype, void* stream)
{
    return guarded([&] {
        require_device();
        launch_add_bias_attn_ffn_residual(out, ffn, attn, in, bias, m, n, tp, inplace_variant, dtype == FTCF_FP16,
                                          (hipStream_t)stream);
    });
}
extern "C" size_t ftcf_masked_multihead_attention_workspace(int B, int nh, int dh, int s_max)
{
    return mmha_workspace_bytes(B, nh, dh, mmha_pick_nsplit(B, nh, s_max));
}
// fills the parameters of one stand-alone fp16 launch (cache_indir NULL: no beams), clears the granules and launches
static void abi_launch_mmha(const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache, const int* seq_len,
                            const int* pad_count, const uint8_t* masked_tokens, const uint8_t* finished, const int* cache_indir,
                            int beam_width, int max_input_len, int B, int nh, int dh, int rot, int s_max, int step, int nsplit,
                            void* ctx, void* workspace, size_t workspace_bytes, hipStream_t stream)
{
    MmhaParams p{};
    p.qkv = (const f16*)qkv;
    p.qkv_bias = (const f16*)qkv_bias;
    p.k_cache = (f16*)k_cache;
    p.v_cache = (f16*)v_cache;
    p.seq_len = seq_len;
    p.pad_count = pad_count;
    p.masked_tokens = masked_tokens;
    p.finished = finished;
    p.d_step = nullptr;
    p.step = step;
    p.B = B;
    p.nh = nh;
    p.dh = dh;
    p.rot = rot;
    p.s_max = s_max;
    p.ctx = (f16*)ctx;
    p.gran = (unsigned long long*)workspace;
    p.layer = 0;
    p.nsplit = nsplit;
    p.cache_indir = cache_indir;
    p.beam_width = beam_width;
    p.max_input_len = max_input_len;
    p.indir_plane = (size_t)B * s_max;
    FTCF_CHECK_ARG(workspace_bytes >= mmha_workspace_bytes(B, nh, dh, p.nsplit), "MMHA workspace too small");
    // the granule tags must not match anything left from an earlier call
    FTCF_HIP_CHECK(hipMemsetAsync(p.gran, 0, mmha_workspace_bytes(B, nh, dh, p.nsplit), stream));
    launch_mmha(p, stream);
}
extern "C" int ftcf_masked_multihead_attention(const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache,
                                               const int* seq_len, const int* pad_count, const uint8_t* masked_tokens,
                                               const uint8_t* finished, int B, int nh, int dh, int rot, int s_max,
                                               int step, void* ctx, void* workspace, size_t workspace_bytes,
                                               void* stream)
{
    return guarded([&] {
        require_device();
        abi_launch_mmha(qkv, qkv_bias, k_cache, v_cache, seq_len, pad_count, masked_tokens, finished, nullptr, 0, 0, B, nh, dh, rot,
                        s_max, step, mmha_pick_nsplit(B, nh, s_max), ctx, workspace, workspace_bytes, (hipStream_t)stream);
    });
}
// the launch with the beam-search arguments and an explicit split count (0: the launcher's choice), fp16 or fp32
extern "C" int ftcf_masked_multihead_attention_beams(ftcf_dtype dtype, const void* qkv, const void* qkv_bias, void* k_cache,
                                                     void* v_cache, const int* seq_len, const int* pad_count,
                                                     const uint8_t* masked_tokens, const uint8_t* finished, const int* cache_indir,
                                                     int beam_width, int max_input_len, int B, int nh, int dh, int rot, int s_max,
                                                     int step, int nsplit, void* ctx, void* workspace, size_t workspace_bytes,
                                                     void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(dtype == FTCF_FP16 || dtype == FTCF_FP32, "MMHA with beams: dtype fp16 or fp32");
        FTCF_CHECK_ARG(qkv && k_cache && v_cache && seq_len && ctx, "NULL tensor");
        FTCF_CHECK_ARG(B >= 1 && nh >= 1 && s_max >= 1 && mmha_head_size_supported(dh) && rot >= 0 && rot % 2 == 0
                           && rot <= dh,
                       "MMHA with beams: bad geometry");
        FTCF_CHECK_ARG(nsplit >= 0 && nsplit <= 16, "MMHA with beams: nsplit 0..16");
        if (cache_indir) {
            FTCF_CHECK_ARG(beam_width > 1 && B % beam_width == 0 && max_input_len >= 0,
                           "cache indirection needs beam_width > 1 and rows = batch * beam_width");
        }
        if (dtype == FTCF_FP32) {
            FTCF_CHECK_ARG((size_t)(3 * dh + s_max + 1 + 8) * sizeof(float) <= ABI_MAX_DYNAMIC_LDS,
                           "fp32 MMHA: a row's scores do not fit the LDS");
            Mmha32Params p{};
            p.qkv = (const float*)qkv;
            p.qkv_bias = (const float*)qkv_bias;
            p.k_cache = (float*)k_cache;
            p.v_cache = (float*)v_cache;
            p.seq_len = seq_len;
            p.pad_count = pad_count;
            p.masked_tokens = masked_tokens;
            p.finished = finished;
            p.B = B;
            p.nh = nh;
            p.dh = dh;
            p.rot = rot;
            p.s_max = s_max;
            p.ctx = (float*)ctx;
            p.cache_indir = cache_indir;
            p.beam_width = beam_width;
            p.max_input_len = max_input_len;
            p.indir_plane = (size_t)B * s_max;
            // k32_mmha reads the step from the device: one word of this call's own, released once the launch has drained
            DeviceBuffer d_step;
            d_step.reserve(sizeof(int));
            FTCF_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_step.ptr, step, 1, (hipStream_t)stream));
            p.d_step = (const int*)d_step.ptr;
            launch32_mmha(p, (hipStream_t)stream);
            FTCF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
            return;
        }
        const int ns = nsplit ? nsplit : mmha_pick_nsplit(B, nh, s_max);
        FTCF_CHECK_ARG(workspace != nullptr, "NULL workspace");
        FTCF_CHECK_ARG(mmha_smem_bytes(dh, s_max, ns) <= ABI_MAX_DYNAMIC_LDS, "MMHA: a split's scores do not fit the LDS");
        abi_launch_mmha(qkv, qkv_bias, k_cache, v_cache, seq_len, pad_count, masked_tokens, finished, cache_indir, beam_width,
                        max_input_len, B, nh, dh, rot, s_max, step, ns, ctx, workspace, workspace_bytes, (hipStream_t)stream);
    });
}
// speculative decoding's kernels, one call each (the engine launches them through the same launchers)
extern "C" size_t ftcf_verify_attention_workspace(int R, int nh, int dh, int s_max)
{
    return verify_attention_workspace_bytes(R, nh, dh, s_max);
}
extern "C" int ftcf_verify_attention(const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache, int cache_row, int len,
                                     int R, int nh, int dh, int rot, int s_max, void* ctx, void* workspace, size_t workspace_bytes,
                                     void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(qkv && k_cache && v_cache && ctx && workspace, "NULL tensor");
        FTCF_CHECK_ARG(cache_row >= 0 && R >= 1 && R <= VERIFY_MAX_ROWS && verify_attention_supported(nh, dh, s_max),
                       "verify attention: bad geometry (size_per_head 64 / 128, at most ~32000 positions)");
        FTCF_CHECK_ARG(workspace_bytes >= verify_attention_workspace_bytes(R, nh, dh, s_max), "verify attention workspace too small");
        VerifyAttnParams p{};
        p.qkv      = (const f16*)qkv;
        p.qkv_bias = (const f16*)qkv_bias;
        p.k_cache  = (f16*)k_cache + (size_t)cache_row * nh * s_max * dh;
        p.v_cache  = (f16*)v_cache + (size_t)cache_row * nh * s_max * dh;
        p.ctx      = (f16*)ctx;
        p.ws       = (float*)workspace;
        p.len      = len;
        p.R        = R;
        p.nh       = nh;
        p.dh       = dh;
        p.rot      = rot;
        p.s_max    = s_max;
        FTCF_HIP_CHECK(hipMemsetAsync(workspace, 0, verify_attention_ticket_bytes(nh), (hipStream_t)stream));
        launch_verify_attention(p, (hipStream_t)stream);
    });
}
extern "C" int ftcf_ngram_draft(const int* tokens, int n, int K, int N, int* draft, int* n_draft, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(tokens && n >= 1, "draft: tokens [n], n >= 1");
        launch_ngram_draft(tokens, n, nullptr, K, N, nullptr, 0, 0, draft, n_draft, nullptr, nullptr, (hipStream_t)stream);
    });
}
extern "C" int ftcf_verify_accept(const ftcf_verify_accept_args* a, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a != nullptr, "NULL argument");
        FTCF_CHECK_ARG(a->struct_size == (int)sizeof(ftcf_verify_accept_args), "verify accept: struct_size is not sizeof(ftcf_verify_accept_args)");
        FTCF_CHECK_ARG(a->R >= 1 && a->R <= VERIFY_MAX_ROWS && a->V >= 1, "verify accept: 1 <= R <= 16, V >= 1");
        FTCF_CHECK_ARG(a->logits && a->output_ids && a->finished && a->seq_len && (a->R == 1 || a->draft), "verify accept: NULL tensor");
        FTCF_CHECK_ARG(a->emitted && a->accepted && a->tokens, "verify accept: NULL output");
        FTCF_CHECK_ARG(a->workspace && a->workspace_bytes >= verify_close_workspace_bytes(), "verify accept: workspace too small");
        FTCF_CHECK_ARG(a->end_id >= 0 && a->end_id < a->V, "verify accept: end_id outside the vocabulary");
        FTCF_CHECK_ARG(!a->stop_words || (a->stop_len >= 1 && a->stop_len <= 4096), "verify accept: stop_len must be in [1, 4096]");
        VerifyCloseParams p{};
        p.logits           = a->logits;
        p.R                = a->R;
        p.V                = a->V;
        p.step             = a->step;
        p.end_id           = a->end_id;
        p.max_input_len    = a->max_input_len;
        p.total_len        = a->total_len;
        p.draft            = a->draft;
        p.output_ids       = a->output_ids;
        p.stop_words       = a->stop_words;
        p.stop_len         = a->stop_len;
        p.finished         = a->finished;
        p.seq_len          = a->seq_len;
        p.cum_log_probs    = a->cum_log_probs;
        p.output_log_probs = a->output_log_probs;
        p.emitted          = a->emitted;
        p.accepted         = a->accepted;
        p.tokens           = a->tokens;
        p.ws               = (float*)a->workspace;
        launch_verify_close(p, (hipStream_t)stream);
    });
}
static_assert(FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES
                  == (2 * VERIFY_MAX_ROWS * VERIFY_ACCEPT_SLICES * VERIFY_SAMPLE_MAX_K + VERIFY_MAX_ROWS * VERIFY_ACCEPT_SLICES * 2
                      + VERIFY_MAX_ROWS * 2)
                         * sizeof(float),
              "FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES is verify_sample_workspace_bytes()");
extern "C" int ftcf_verify_sample(const ftcf_verify_sample_args* a, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a != nullptr, "NULL argument");
        FTCF_CHECK_ARG(a->struct_size == (int)sizeof(ftcf_verify_sample_args), "verify sample: struct_size is not sizeof(ftcf_verify_sample_args)");
        FTCF_CHECK_ARG(a->R >= 1 && a->R <= VERIFY_MAX_ROWS && a->V >= 1, "verify sample: 1 <= R <= 16, V >= 1");
        FTCF_CHECK_ARG(a->top_k >= 1 && a->top_k <= VERIFY_SAMPLE_MAX_K && a->V <= VERIFY_SAMPLE_MAX_V,
                       "verify sample: 1 <= top_k <= 64, V <= 131072");
        FTCF_CHECK_ARG(a->logits && a->output_ids && a->finished && a->seq_len && a->draw_counter && (a->R == 1 || a->draft),
                       "verify sample: NULL tensor");
        FTCF_CHECK_ARG(a->emitted && a->accepted && a->tokens, "verify sample: NULL output");
        FTCF_CHECK_ARG(a->workspace && a->workspace_bytes >= verify_sample_workspace_bytes(), "verify sample: workspace too small");
        FTCF_CHECK_ARG(a->end_id >= 0 && a->end_id < a->V, "verify sample: end_id outside the vocabulary");
        FTCF_CHECK_ARG(!a->stop_words || (a->stop_len >= 1 && a->stop_len <= 4096), "verify sample: stop_len must be in [1, 4096]");
        FTCF_CHECK_ARG(a->top_p_topk > 0.f && a->top_p_topk <= 1.f && a->temperature >= 0.f, "verify sample: top_p_topk in (0, 1], temperature >= 0");
        VerifySampleParams q{};
        VerifyCloseParams& p = q.c;
        p.logits           = a->logits;
        p.R                = a->R;
        p.V                = a->V;
        p.step             = a->step;
        p.end_id           = a->end_id;
        p.max_input_len    = a->max_input_len;
        p.total_len        = a->total_len;
        p.draft            = a->draft;
        p.output_ids       = a->output_ids;
        p.stop_words       = a->stop_words;
        p.stop_len         = a->stop_len;
        p.finished         = a->finished;
        p.seq_len          = a->seq_len;
        p.cum_log_probs    = a->cum_log_probs;
        p.output_log_probs = a->output_log_probs;
        p.emitted          = a->emitted;
        p.accepted         = a->accepted;
        p.tokens           = a->tokens;
        q.top_k             = a->top_k;
        q.top_p_topk        = a->top_p_topk;
        q.apply_temperature = (a->temperature != 0.f && a->temperature != 1.f) ? 1 : 0;
        q.temperature       = a->temperature;
        q.random_seed       = (uint64_t)a->random_seed;
        q.draw_counter      = reinterpret_cast<uint64_t*>(a->draw_counter);
        q.ws                = (float*)a->workspace;
        launch_verify_sample(q, (hipStream_t)stream);
    });
}
extern "C" int ftcf_context_attention(const void* qkv, const void* qkv_bias, const int* input_lengths, void* k_cache,
                                      void* v_cache, int B, int S, int nh, int dh, int rot, int s_max, void* ctx,
                                      void* stream)
{
    return guarded([&] {
        require_device();
        launch_context_attention((const f16*)qkv, (const f16*)qkv_bias, input_lengths, (f16*)k_cache, (f16*)v_cache, B,
                                 S, nh, dh, rot, s_max, (f16*)ctx, (hipStream_t)stream);
    });
}
extern "C" int ftcf_context_attention_range(ftcf_dtype dtype, void* qkv, const void* qkv_bias, const int* input_lengths,
                                            void* k_cache, void* v_cache, int B, int S, int nh, int dh, int rot, int s_max,
                                            int cache_row_mult, int s_lo, int s_hi, void* ctx, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(dtype == FTCF_FP16 || dtype == FTCF_FP32, "context attention: dtype fp16 or fp32");
        FTCF_CHECK_ARG(qkv && qkv_bias && input_lengths && k_cache && v_cache && ctx, "NULL tensor");
        FTCF_CHECK_ARG(B >= 1 && nh >= 1 && cache_row_mult >= 1 && mmha_head_size_supported(dh) && rot >= 0 && rot % 2 == 0
                           && rot <= dh && S >= 1 && S <= s_max,
                       "context attention: bad geometry");
        if (dtype == FTCF_FP32) {
            FTCF_CHECK_ARG(s_lo == 0 && (s_hi == -1 || s_hi == S), "fp32 context attention: the whole prompt only");
            FTCF_CHECK_ARG((size_t)(S + dh + 4) * sizeof(float) <= ABI_MAX_DYNAMIC_LDS,
                           "fp32 context attention: a query's scores do not fit the LDS");
            launch32_context_attention((float*)qkv, (const float*)qkv_bias, input_lengths, (float*)k_cache, (float*)v_cache, B, S,
                                       nh, dh, rot, s_max, (float*)ctx, (hipStream_t)stream, cache_row_mult);
            FTCF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
            return;
        }
        FTCF_CHECK_ARG(s_lo >= 0 && s_lo < s_hi && s_hi <= S, "context attention: bad token range");
        launch_context_attention((const f16*)qkv, (const f16*)qkv_bias, input_lengths, (f16*)k_cache, (f16*)v_cache, B, S, nh,
                                 dh, rot, s_max, (f16*)ctx, (hipStream_t)stream, cache_row_mult, s_lo, s_hi);
    });
}
// the batcher's paged kernels, one call each (the batcher itself launches them through the same launchers)
extern "C" int ftcf_paged_attention(const void* qkv, const void* qkv_bias, void* k_pool, void* v_pool, const int* page_table,
                                    const int* lengths, const uint8_t* finished, int B, int nh, int dh, int rot, int page_tokens,
                                    int max_pages, int max_len, void* ctx, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(qkv && qkv_bias && k_pool && v_pool && page_table && lengths && finished && ctx, "NULL tensor");
        FTCF_CHECK_ARG(B >= 1 && nh >= 1 && page_tokens >= 1 && max_pages >= 1 && max_len >= 1 && max_len <= max_pages * page_tokens,
                       "paged attention: bad geometry");
        MmhaPagedParams p{};
        p.qkv = (const f16*)qkv;
        p.qkv_bias = (const f16*)qkv_bias;
        p.kpool = (f16*)k_pool;
        p.vpool = (f16*)v_pool;
        p.page_table = page_table;
        p.len = lengths;
        p.finished = finished;
        p.B = B;
        p.nh = nh;
        p.dh = dh;
        p.rot = rot;
        p.P = page_tokens;
        p.max_pages = max_pages;
        p.ctx = (f16*)ctx;
        launch_mmha_paged(p, max_len, (hipStream_t)stream);
    });
}
extern "C" int ftcf_scatter_kv_to_pages(const void* k_cache, const void* v_cache, void* k_pool, void* v_pool, const int* pages, int L,
                                        int nh, int dh, int s_max, int S, int page_tokens, size_t pool_layer_elems,
                                        size_t src_layer_elems, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(k_cache && v_cache && k_pool && v_pool && pages, "NULL tensor");
        FTCF_CHECK_ARG(L >= 1 && nh >= 1 && page_tokens >= 1 && S >= 0 && S <= s_max && dh % 8 == 0, "scatter_kv_to_pages: bad geometry");
        launch_scatter_kv_to_pages((const f16*)k_cache, (const f16*)v_cache, (f16*)k_pool, (f16*)v_pool, pages, L, nh, dh, s_max, S,
                                   page_tokens, pool_layer_elems, (hipStream_t)stream, src_layer_elems);
    });
}
extern "C" int ftcf_gather_pages_to_kv(void* k_cache, void* v_cache, const void* k_pool, const void* v_pool, const int* pages, int L,
                                       int nh, int dh, int s_max, int T, int page_tokens, size_t pool_layer_elems,
                                       size_t dst_layer_elems, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(k_cache && v_cache && k_pool && v_pool && pages, "NULL tensor");
        FTCF_CHECK_ARG(L >= 1 && nh >= 1 && page_tokens >= 1, "gather_pages_to_kv: bad geometry");
        launch_gather_pages_to_kv((f16*)k_cache, (f16*)v_cache, (const f16*)k_pool, (const f16*)v_pool, pages, L, nh, dh, s_max, T,
                                  page_tokens, pool_layer_elems, (hipStream_t)stream, dst_layer_elems);
    });
}
extern "C" int ftcf_pages_pack(void* staging, const void* k_pool, const void* v_pool, const int* pages, int n, int L, int nh, int dh,
                               int page_tokens, size_t pool_layer_elems, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(staging && k_pool && v_pool && pages, "NULL tensor");
        FTCF_CHECK_ARG(n >= 0 && L >= 1 && nh >= 1 && page_tokens >= 1 && dh >= 8 && dh % 8 == 0, "pages_pack: bad geometry");
        launch_pages_pack((f16*)staging, (const f16*)k_pool, (const f16*)v_pool, pages, n, L, (size_t)nh * page_tokens * dh,
                          pool_layer_elems, (hipStream_t)stream);
    });
}
extern "C" int ftcf_pages_unpack(const void* staging, void* k_pool, void* v_pool, const int* pages, int n, int L, int nh, int dh,
                                 int page_tokens, size_t pool_layer_elems, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(staging && k_pool && v_pool && pages, "NULL tensor");
        FTCF_CHECK_ARG(n >= 0 && L >= 1 && nh >= 1 && page_tokens >= 1 && dh >= 8 && dh % 8 == 0, "pages_unpack: bad geometry");
        launch_pages_unpack((const f16*)staging, (f16*)k_pool, (f16*)v_pool, pages, n, L, (size_t)nh * page_tokens * dh,
                            pool_layer_elems, (hipStream_t)stream);
    });
}

// ---- one step of the dynamic-decode layer / of the beam-search layer on the CALLER's logits and state ----
// (the engine and the batcher launch the same launchers; these entries own what a request's arena holds for them: the
// DecodeState, the pinned flag words, the workspace and the device copies of the runtime arguments, for the one call)
namespace {
struct StepScratch {  // freed when the call returns, also when it throws
    std::vector<void*> dev;
    void*              pinned = nullptr;
    ~StepScratch()
    {
        for (void* d : dev) {
            (void)hipFree(d);
        }
        if (pinned) {
            (void)hipHostFree(pinned);
        }
    }
    template<typename T>
    T* alloc(size_t n)
    {
        void* d = nullptr;
        FTCF_HIP_CHECK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
        dev.push_back(d);
        return (T*)d;
    }
    template<typename T>
    T* upload(const std::vector<T>& v, hipStream_t s)
    {
        T* d = alloc<T>(v.size());
        FTCF_HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        return d;
    }
    DecodeState* state(int step, hipStream_t s)  // as k_decode_init leaves it, at `step`
    {
        const DecodeState h{step, 0, 0, 0};
        DecodeState*      d = alloc<DecodeState>(1);
        FTCF_HIP_CHECK(hipMemcpyAsync(d, &h, sizeof(h), hipMemcpyHostToDevice, s));
        FTCF_HIP_CHECK(hipStreamSynchronize(s));  // (`h` dies at scope exit)
        return d;
    }
};
}  // namespace

extern "C" int ftcf_dynamic_decode_step(const ftcf_dynamic_decode_args* a, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a != nullptr, "NULL arguments");
        hipStream_t s = (hipStream_t)stream;
        const int   B = a->B, V = a->V;
        FTCF_CHECK_ARG(a->logits && a->output_ids && a->finished && a->seq_len && a->draw_counter && a->input_lengths, "NULL tensor");
        FTCF_CHECK_ARG(B >= 1 && V >= 1 && a->max_input_len >= 0 && a->total_len >= 1, "dynamic decode step: bad geometry");
        FTCF_CHECK_ARG(a->row_len || (a->step >= a->max_input_len && a->step <= a->total_len),
                       "dynamic decode step: step must be in [max_input_len, total_len]");
        FTCF_CHECK_ARG(a->end_id >= 0 && a->end_id < V, "dynamic decode step: end_id outside the vocabulary");
        FTCF_CHECK_ARG(!a->output_log_probs || a->row_len || a->step < a->total_len, "output_log_probs has no row for step == total_len");
        FTCF_CHECK_ARG(!a->stop_words || a->stop_len >= 1, "stop_words needs stop_len >= 1");
        FTCF_CHECK_ARG(!a->optional_last_tokens || a->optional_count >= 1, "optional_last_tokens needs optional_count >= 1");
        FTCF_CHECK_ARG(a->top_logprobs >= 0 && a->top_logprobs <= TOP_LOGPROBS_MAX, "top_logprobs must be in [0, 20]");
        FTCF_CHECK_ARG(a->top_logprobs == 0 || (a->top_ids && a->top_log_probs), "top_logprobs needs top_ids and top_log_probs");
        FTCF_CHECK_ARG(a->top_logprobs == 0 || a->row_len || a->step < a->total_len, "top_logprobs has no row for step == total_len");
        auto top_k = broadcast_arg<int>(a->top_k, a->n_top_k, B, 0, "top_k");
        auto top_p = broadcast_arg<float>(a->top_p, a->n_top_p, B, 0.f, "top_p");
        auto temp  = broadcast_arg<float>(a->temperature, a->n_temperature, B, 1.f, "temperature");
        auto rep   = broadcast_arg<float>(a->repetition_penalty, a->n_repetition_penalty, B, 1.f, "repetition_penalty");
        auto seed  = broadcast_arg<uint64_t>(a->random_seed, a->n_random_seed, B, 0, "random_seed");
        auto minl  = broadcast_arg<int>(a->min_length, a->n_min_length, B, 0, "min_length");
        const SamplingRouting route = route_sampling_args(top_k, top_p, temp, rep, minl, a->n_repetition_penalty > 0);

        StepScratch    mem;
        SamplingParams sp{};
        sp.logits             = a->logits;
        sp.B                  = B;
        sp.V                  = V;
        sp.max_input_len      = a->max_input_len;
        sp.total_len          = a->total_len;
        sp.end_id             = a->end_id;
        sp.input_lengths      = a->input_lengths;
        sp.top_k              = mem.upload(route.k_eff, s);
        sp.top_p_topk         = mem.upload(route.p_topk, s);
        sp.top_p_topp         = mem.upload(route.p_topp, s);
        sp.temperature        = mem.upload(temp, s);
        sp.repetition_penalty = mem.upload(rep, s);
        sp.min_length         = mem.upload(minl, s);
        route.apply(sp);
        sp.random_seed          = mem.upload(seed, s);
        sp.draw_counter         = a->draw_counter;
        sp.stop_words           = a->stop_words;
        sp.stop_len             = a->stop_len;
        sp.optional_last_tokens = a->optional_last_tokens;
        sp.optional_count       = a->optional_count;
        sp.return_cum_log_probs = (a->return_cum_log_probs || a->output_log_probs || a->top_logprobs > 0) ? 1 : 0;
        sp.output_ids           = a->output_ids;
        sp.finished             = a->finished;
        sp.seq_len              = a->seq_len;
        sp.cum_log_probs        = a->cum_log_probs;
        sp.output_log_probs     = a->output_log_probs;
        if (a->top_logprobs > 0) {
            sp.top_logprobs       = a->top_logprobs;
            sp.top_logprob_ids    = a->top_ids;
            sp.top_logprob_values = a->top_log_probs;
        }
        sp.row_len              = a->row_len;
        sp.pad_count            = a->pad_count;
        if (!sp.pad_count) {
            sp.pad_count = mem.alloc<int>(B);
            FTCF_HIP_CHECK(hipMemsetAsync(sp.pad_count, 0, (size_t)B * sizeof(int), s));
        }
        sp.ws = mem.alloc<char>(sampling_workspace_bytes(B, V));
        FTCF_HIP_CHECK(hipHostMalloc(&mem.pinned, 8 * sizeof(int), hipHostMallocDefault));
        sp.h_flags = (int*)mem.pinned;
        memset(sp.h_flags, 0, 8 * sizeof(int));
        sp.state = mem.state(a->step, s);  // (synchronises: the host vectors above have been copied)
        const bool finish = a->finish != 0;
        if (a->form) {
            *a->form = dynamic_decode_form(sp, finish);
        }
        launch_dynamic_decode(sp, s, finish);
        DecodeState h{};
        FTCF_HIP_CHECK(hipMemcpyAsync(&h, sp.state, sizeof(h), hipMemcpyDeviceToHost, s));
        FTCF_HIP_CHECK(hipStreamSynchronize(s));
        if (a->all_finished) {
            *a->all_finished = h.all_finished;
        }
        if (a->next_step) {
            *a->next_step = h.step;
        }
    });
}

extern "C" int ftcf_logit_process(const ftcf_logit_process_args* a, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a != nullptr, "NULL arguments");
        FTCF_CHECK_ARG(a->struct_size == (int)sizeof(ftcf_logit_process_args), "logit process: struct_size is not sizeof(ftcf_logit_process_args)");
        FTCF_CHECK_ARG(a->logits, "NULL tensor");
        LogitProcessParams p{};
        p.logits       = a->logits;
        p.B            = a->batch_size;
        p.V            = a->vocab_size;
        p.end_id       = a->end_id;
        p.finished     = a->finished;
        p.row_on       = a->row_on;
        p.hist         = a->hist;
        p.stride_t     = a->stride_t;
        p.stride_b     = a->stride_b;
        p.hist_len     = a->hist_len;
        p.gen_start    = a->gen_start;
        p.hist_len_add = a->hist_len_add;
        p.presence     = a->presence_penalty;
        p.frequency    = a->frequency_penalty;
        p.min_new      = a->min_new_tokens;
        p.bias_ids     = a->bias_ids;
        p.bias_values  = a->bias_values;
        p.n_bias       = a->n_bias;
        p.bias_stride  = a->bias_stride;
        p.bad_words    = a->bad_words;
        p.bad_len      = a->bad_words_len;
        p.mask         = a->mask;
        p.mask_on      = a->mask_on;
        p.slice        = a->slice;
        launch_logit_process(p, (hipStream_t)stream);
    });
}

extern "C" int ftcf_beam_search_step(const ftcf_beam_search_args* a, void* stream)
{
    return guarded([&] {
        require_device();
        FTCF_CHECK_ARG(a != nullptr, "NULL arguments");
        hipStream_t s = (hipStream_t)stream;
        const int   B = a->B, K = a->K, V = a->V;
        FTCF_CHECK_ARG(a->logits && a->output_ids && a->parent_ids && a->finished && a->seq_len && a->cum_log_probs && a->cache_indir
                           && a->input_lengths,
                       "NULL tensor");
        FTCF_CHECK_ARG(B >= 1 && K >= 2 && K <= BEAM_MAX_K && V >= K && a->max_input_len >= 0 && a->total_len >= 1 && a->s_max >= 1,
                       "beam search step: bad geometry (beam_width in [2, 64], at least beam_width tokens)");
        FTCF_CHECK_ARG(a->step >= a->max_input_len && a->step >= 1 && a->step < a->total_len,
                       "beam search step: step must be in [max(1, max_input_len), total_len)");
        FTCF_CHECK_ARG(a->end_id >= 0 && a->end_id < V, "beam search step: end_id outside the vocabulary");
        FTCF_CHECK_ARG(!a->stop_words || a->stop_len >= 1, "stop_words needs stop_len >= 1");
        FTCF_CHECK_ARG(!a->optional_last_tokens || a->optional_count >= 1, "optional_last_tokens needs optional_count >= 1");
        auto temp = broadcast_arg<float>(a->temperature, a->n_temperature, B, 1.f, "temperature");
        auto rep  = broadcast_arg<float>(a->repetition_penalty, a->n_repetition_penalty, B, 1.f, "repetition_penalty");
        auto divr = broadcast_arg<float>(a->beam_search_diversity_rate, a->n_beam_search_diversity_rate, B, 0.f, "beam_search_diversity_rate");
        auto lenp = broadcast_arg<float>(a->len_penalty, a->n_len_penalty, B, 0.f, "len_penalty");
        auto minl = broadcast_arg<int>(a->min_length, a->n_min_length, B, 0, "min_length");
        bool any_min = false;
        for (int b = 0; b < B; b++) {
            any_min |= (minl[b] > 0);
        }
        StepScratch mem;
        BeamParams  bp{};
        bp.logits               = a->logits;
        bp.B                    = B;
        bp.K                    = K;
        bp.V                    = V;
        bp.max_input_len        = a->max_input_len;
        bp.total_len            = a->total_len;
        bp.end_id               = a->end_id;
        bp.s_max                = a->s_max;
        bp.input_lengths        = a->input_lengths;
        bp.temperature          = mem.upload(temp, s);
        bp.repetition_penalty   = a->n_repetition_penalty > 0 ? mem.upload(rep, s) : nullptr;  // penalty type None otherwise
        bp.diversity_rate       = mem.upload(divr, s);
        bp.len_penalty          = mem.upload(lenp, s);
        bp.min_length           = any_min ? mem.upload(minl, s) : nullptr;
        bp.stop_words           = a->stop_words;
        bp.stop_len             = a->stop_len;
        bp.optional_last_tokens = a->optional_last_tokens;
        bp.optional_count       = a->optional_count;
        bp.output_ids           = a->output_ids;
        bp.parent_ids           = a->parent_ids;
        bp.finished             = a->finished;
        bp.seq_len              = a->seq_len;
        bp.cum_log_probs        = a->cum_log_probs;
        bp.step_log_probs       = a->step_log_probs;
        bp.cache_indir          = a->cache_indir;
        bp.ws                   = mem.alloc<char>(beam_workspace_bytes(B, K));
        bp.state                = mem.state(a->step, s);  // (synchronises: the host vectors above have been copied)
        launch_beam_search(bp, s);
        FTCF_HIP_CHECK(hipStreamSynchronize(s));
    });
}

