// Host-side engine + C ABI (include/ftcf.h) of the MI355X GPT-NeoX / CodeFuse decoder.
//
// Host classes mirror the reference's layer split (layers are thin: they own no scratch of their own and never
// reMalloc per call -- one arena is planned per request shape):
//   GptNeoX               <- models/gptneox/GptNeoX.cc:386-1052 (generation loop, LM head, dynamic decode, outputs)
//   GptNeoXContextDecoder <- models/gptneox/GptNeoXContextDecoder.cc:223-512 (prefill)
//   GptNeoXDecoder        <- models/gptneox/GptNeoXDecoder.cc:197-389 (one token through L layers)
//   DecoderSelfAttentionLayer / FfnLayer / DynamicDecodeLayer are the launch helpers used by those.
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
static float* abi_gemm_workspace(int m, hipStream_t s);
void gemm_dispatch(const f16* A, const void* W, const f16* scale, const f16* bias, int act, f16* C, int m, int n, int k, bool int8,
                   hipStream_t s, float* smallm_ws, size_t smallm_partial, int num_cu, const int* d_step, unsigned* smallm_seq,
                   float* tiled_ws)
{
    if (m <= 4) {
        SplitKParams p{};
        p.x_a = A;
        p.W_a = W;
        p.scale_a = scale;
        p.bias = bias;
        p.out = C;
        p.N = n;
        p.KT_a = k / (int8 ? TILE_K_I8 : TILE_K_F16);
        p.KT_b = 0;
        p.act = act;
        p.tp = 1;
        plan_splitk(p, int8, m, 4);
        launch_gemv_splitk(p, int8, m, EPI_PLAIN, s);
    }
    else if (m <= 16) {
        launch_gemm_smallm(A, W, scale, bias, act, C, smallm_ws, smallm_partial, m, n, k, int8, num_cu, s, d_step,
                           smallm_seq);
    }
    else {
        launch_gemm_tiled(A, W, scale, bias, act, C, m, n, k, int8, s, tiled_ws);
    }
}

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
void lm_head_dispatch(const f16* A, const f16* W, float* logits, int m, int n, int k, int ldc, hipStream_t s)
{
    if (m <= 4) {
        launch_lm_head(A, W, logits, m, n, k, ldc, s);
    }
    else {
        launch_gemm_nk_f32out(A, W, logits, m, n, k, ldc, s);
    }
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

template<typename T>
static std::vector<T> broadcast_arg(const T* p, int n, int B, T dflt, const char* name)
{
    std::vector<T> v((size_t)B, dflt);
    if (n > 0) {
        FTCF_CHECK_ARG(p != nullptr, std::string(name) + " pointer is NULL");
        FTCF_CHECK_ARG(n == 1 || n == B, std::string(name) + " must have 1 or batch_size entries");
        for (int b = 0; b < B; b++) {
            v[b] = p[n == 1 ? 0 : b];
        }
    }
    return v;
}

// The runtime-arg routing of TopKSamplingLayer.cu:27-77 / TopPSamplingLayer.cu:30-110 and the ALL_OF switches of
// BaseSamplingLayer.cc:283-313, in ONE place (the engine's begin() and the kernel-level ftcf_dynamic_decode_step): from the
// broadcast host arguments to what the decode kernels read.  k == 0 && p == 0 is greedy (k = 1), k is cut at 1024, a top-k row
// without a p samples from all of its k, and a penalty switches on for the batch as soon as one row differs from its default.
struct SamplingRouting {
    std::vector<int>   k_eff;           // per row: the k of the top-k layer, 0 = the row belongs to the top-p layer
    std::vector<float> p_topk, p_topp;  // per row: the p each layer uses
    int  max_top_k = 1, any_top_p = 0, apply_temperature = 0, apply_repetition = 0;
    bool any_min = false, rep_given = false;
    // the host view of the batch; sp.repetition_penalty / sp.min_length hold the device copies and are dropped where not given
    void apply(SamplingParams& sp) const
    {
        sp.max_top_k         = max_top_k;
        sp.any_top_p         = any_top_p;
        sp.apply_temperature = apply_temperature;
        sp.apply_repetition  = apply_repetition;
        if (!rep_given) {
            sp.repetition_penalty = nullptr;
        }
        if (!any_min) {
            sp.min_length = nullptr;
        }
    }
};
static SamplingRouting route_sampling_args(const std::vector<int>& top_k, const std::vector<float>& top_p, const std::vector<float>& temp,
                                           const std::vector<float>& rep, const std::vector<int>& minl, bool rep_given)
{
    const int       batch = (int)top_k.size();
    SamplingRouting r;
    r.k_eff.resize(batch);
    r.p_topk.resize(batch);
    r.p_topp.resize(batch);
    r.rep_given = rep_given;
    bool temp_all_one = true, rep_all_default = true;
    for (int b = 0; b < batch; b++) {
        int   k = top_k[b];
        float p = top_p[b];
        FTCF_CHECK_ARG(k >= 0, "top_k must be >= 0");
        if (k == 0 && p == 0.0f) {
            k = 1;
        }
        float pk = p;
        if (k > 0 && pk == 0.0f) {
            pk = 1.0f;
        }
        r.k_eff[b]  = k > 1024 ? 1024 : k;
        r.p_topk[b] = pk < 0.f ? 0.f : (pk > 1.f ? 1.f : pk);
        r.p_topp[b] = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
        temp_all_one &= (temp[b] == 1.0f);
        rep_all_default &= (rep[b] == 1.0f);
        r.any_min |= (minl[b] > 0);
        r.max_top_k = std::max(r.max_top_k, r.k_eff[b]);
        r.any_top_p |= (r.k_eff[b] == 0);
    }
    r.apply_temperature = temp_all_one ? 0 : 1;
    r.apply_repetition  = (rep_given && !rep_all_default) ? 1 : 0;
    return r;
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
        bp.cache_indir          = a->cache_indir;
        bp.ws                   = mem.alloc<char>(beam_workspace_bytes(B, K));
        bp.state                = mem.state(a->step, s);  // (synchronises: the host vectors above have been copied)
        launch_beam_search(bp, s);
        FTCF_HIP_CHECK(hipStreamSynchronize(s));
    });
}


// ---------------------------------------------------------------------------------------------------------------
// the engine
// ---------------------------------------------------------------------------------------------------------------

// transposeAxis01 for the TP logits all-gather: [tp][B][vl] -> [B][V] (GptNeoX.cc:913-924); src >= 0 reads every slice
// from slot [src] (fake peers: only the rank's own slot was written)
__global__ void k_transpose_gathered_logits(float* out, const float* in, int tp, int B, int vl, int src)
{
    const size_t total = (size_t)tp * B * vl;
    const size_t slot  = (size_t)B * vl;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int    j = (int)(i % vl);
        const size_t t = i / vl;
        const int    b = (int)(t % B), r = (int)(t / B);
        out[(size_t)b * tp * vl + (size_t)r * vl + j] = in[src < 0 ? i : (size_t)src * slot + (i % slot)];
    }
}

// the all-reduce of fake peers: TP identical partials sum to TP x the buffer (fp32 product, one rounding)
template<typename T>
__global__ void k_scale_by_tp(T* buf, size_t n, float tp)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        buf[i] = (T)((float)buf[i] * tp);
    }
}
template __global__ void k_scale_by_tp<f16>(f16*, size_t, float);
template __global__ void k_scale_by_tp<float>(float*, size_t, float);

// The prompt phase of a request (GptNeoX.cc:640-735): embedding -> context decoder -> the last token's hidden state into x, for
// fp32 or fp16 / int8 rows, with or without beams (a beam request prefills ONE row per request into cache row b * K and tiles its
// last hidden state); a prompt of one token has no prompt phase, its token is the first decode step's input.
// in_ids / in_len: the inputs per ROW (tiled for beams)
void ftcf_gptneox::prompt_phase(const ftcf_forward_args& a, const int* in_ids, const int* in_len)
{
    const int K = a.beam_width, batch = a.batch_size, B = batch * K, S = a.max_input_len, s_max = S + a.output_len;
    if (S > 1 && K > 1 && fp32) {
        launch32_prompt_embedding(F(px), nullptr, F(wte), a.input_ids, batch, S, H, stream);
        launch_tile_prompt_ids(step_ids, a.input_ids, batch, K, S, stream);
        context_decoder32(batch, S, a.input_lengths, s_max, K);
        launch32_gather_last_token(F(x), F(px), a.input_lengths, batch, S, H, stream, K);
    }
    else if (S > 1 && fp32) {
        launch32_prompt_embedding(F(px), step_ids, F(wte), in_ids, B, S, H, stream);
        context_decoder32(B, S, in_len, s_max, 1);
        launch32_gather_last_token(F(x), F(px), in_len, B, S, H, stream);
    }
    else if (S > 1 && K > 1) {
        launch_prompt_embedding(px, nullptr, wte, a.input_ids, batch, S, H, stream);
        launch_tile_prompt_ids(step_ids, a.input_ids, batch, K, S, stream);
        context_decoder(batch, S, a.input_lengths, s_max, K);
        launch_gather_last_token(x, px, a.input_lengths, batch, S, H, stream, K);
    }
    else if (S > 1) {
        launch_prompt_embedding(px, step_ids, wte, in_ids, B, S, H, stream);
        context_decoder(B, S, in_len, s_max, 1);
        launch_gather_last_token(x, px, in_len, B, S, H, stream);
    }
    else {
        FTCF_HIP_CHECK(hipMemcpyAsync(step_ids, in_ids, (size_t)B * 4, hipMemcpyDeviceToDevice, stream));
    }
}

void ftcf_gptneox::begin(const ftcf_forward_args& a)
{
    {  // (once per request, not per token)
        const char* m       = getenv("FTCF_DECODE_OVERLAP");
        decode_overlap_mode = !m ? 0 : (!strcmp(m, "auto") ? 2 : (atoi(m) ? 1 : 0));
    }
    Range r("ftcf.begin");
    FT_LOG_TRACE(cfg.device, "begin: batch %d x beam %d, max_input_len %d, output_len %d", a.batch_size, a.beam_width, a.max_input_len,
                 a.output_len);
    const int B = a.batch_size * (a.beam_width > 0 ? a.beam_width : 1);  // rows
    const int S = a.max_input_len, out_len = a.output_len;
    FTCF_CHECK_ARG(a.batch_size >= 1 && S >= 1 && out_len >= 1, "batch_size, max_input_len and output_len must be >= 1");
    FTCF_CHECK_ARG(a.input_ids && a.input_lengths && a.output_ids && a.sequence_lengths, "NULL tensor");
    const int K = a.beam_width, batch = a.batch_size;
    FTCF_CHECK_ARG(K >= 1 && K <= BEAM_MAX_K, "beam_width must be in [1, 64]");
    FTCF_CHECK_ARG(prefill_begin == 0 || (!fp32 && K == 1 && batch == 1 && prefill_begin < S),
                   "a prompt phase from a token offset needs one fp16 / int8 sequence without beams, longer than the offset");
    FTCF_CHECK_ARG(!a.output_log_probs || K == 1,
                   "output_log_probs is not supported with beam_width > 1 (the values would have to follow the beams' parents)");
    FTCF_CHECK_ARG(a.top_logprobs >= 0 && a.top_logprobs <= TOP_LOGPROBS_MAX, "top_logprobs must be in [0, 20]");
    FTCF_CHECK_ARG(a.top_logprobs == 0 || (a.top_logprob_ids && a.top_logprob_values),
                   "top_logprobs needs top_logprob_ids and top_logprob_values");
    FTCF_CHECK_ARG(a.top_logprobs == 0 || K == 1,
                   "top_logprobs is not supported with beam_width > 1 (the pairs would have to follow the beams' parents)");
    FTCF_CHECK_ARG(!a.context_log_probs || !fp32, "context_log_probs needs an fp16 / int8 engine");
    FTCF_CHECK_ARG(!a.context_log_probs || prefill_begin == 0, "context_log_probs needs the whole prompt phase");
    FTCF_HIP_CHECK(hipSetDevice(cfg.device));
    abandon_session();  // (a request left open -- begin / step without finish, or a step that threw -- must not leak its graph)
    stats.window_allreduces = 0;
    // everything the caller enqueued on its stream (input tensors) happens-before the engine's work
    FTCF_HIP_CHECK(hipEventRecord(ev_user, user_stream));
    FTCF_HIP_CHECK(hipStreamWaitEvent(stream, ev_user, 0));
    const int total = S + out_len;  // max_output_seq_len == max_seq_len == max_cache_seq_len (GptNeoX.cc:520-523)
    const int s_max = total;
    ses.K = K;  // (decoder path selection reads it)
    const int  tpn     = cfg.tensor_para_size;
    const bool want_tp = tpn > 1 && persist && persist_tp && K == 1 && B <= 2 && cfg.use_gptj_residual && tpn <= PERSIST_MAX_TP;
    // message buffers of the RCCL-free prompt-phase all-reduce (k_window_allreduce) behind the granules of the decode exchange
    static const int winar_on = getenv("FTCF_TP_WINAR") ? atoi(getenv("FTCF_TP_WINAR")) : 1;
    static const int winar_mb = getenv("FTCF_TP_WINAR_MB") ? atoi(getenv("FTCF_TP_WINAR_MB")) : 16;
    const bool want_ar = tpn > 1 && tpn <= 8 && winar_on && !fp32 && cfg.comm && !cfg.comm->local && !cfg.comm->ar_failed;
    if (want_tp || want_ar) {
        // (collective: every rank sees the same request shape) room for two rows: [tp][2 * H / 2] granules
        // (two planes by layer parity: persist_device.hip.h ps_tp_exchange), then 16 flags, then four message buffers
        const size_t gran = ((size_t)2 * tpn * H * 8 + 4095) & ~(size_t)4095;
        const size_t cap  = want_ar ? (size_t)std::max(1, winar_mb) << 20 : 0;
        const bool   had  = cfg.comm->win_ok && cfg.comm->win_bytes >= gran + 4096 + 4 * cap;
        comm_ensure_window(cfg.comm, gran + 4096 + 4 * cap, stream);
        if (cfg.comm->win_ok && cfg.comm->win_bytes >= gran + 4096 + 4 * cap && cap > 0 && (!had || cfg.comm->ar_cap != cap)) {
            cfg.comm->ar_flag_off = gran;  // (a fresh window is zero: the call numbers start over)
            cfg.comm->ar_data_off = gran + 4096;
            cfg.comm->ar_cap      = cap;
            if (!had) {
                cfg.comm->ar_seq = 0;
                if (cfg.comm->ar_sync) {
                    FTCF_HIP_CHECK(hipMemsetAsync(cfg.comm->ar_sync, 0, 64, stream));
                }
            }
        }
    }
    // speculative greedy decoding: a hint that cannot change a result -- a request it does not cover
    // runs as it always has, and the stats say so
    FTCF_CHECK_ARG(a.speculative_tokens >= 0 && a.speculative_tokens <= VERIFY_MAX_ROWS - 1, "speculative_tokens must be in [0, 15]");
    FTCF_CHECK_ARG(a.speculative_ngram >= 0 && a.speculative_ngram <= 8, "speculative_ngram must be in [0, 8]");
    bool spec = a.speculative_tokens > 0 && batch == 1 && K == 1 && !fp32 && tpn == 1 && cfg.use_gptj_residual && prefill_begin == 0
                && verify_attention_supported(nhl, dh, total) && H % 64 == 0 && hl % 64 == 0 && il % 64 == 0 && !a.callback && !a.return_cum_log_probs
                && !a.output_log_probs && a.top_logprobs == 0 && !a.debug_logits && !a.stop_words_list && !a.optional_last_tokens && a.n_min_length == 0
                && (a.n_top_k == 0 || (a.top_k && a.top_k[0] <= 1)) && (a.n_top_p == 0 || (a.top_p && a.top_p[0] == 0.f))
                && (a.n_repetition_penalty == 0 || (a.repetition_penalty && a.repetition_penalty[0] == 1.f)) && !logits_hook;
    if (spec) {  // (the token history must be dense from position 0: a prompt as long as its row)
        int h_len = 0;
        FTCF_HIP_CHECK(hipMemcpyAsync(&h_len, a.input_lengths, sizeof(int), hipMemcpyDeviceToHost, stream));
        comm_stream_sync(cfg.comm, stream);
        spec = h_len == S;
    }
    spec_plan = spec;
    plan(B, S, total, K);
    if (want_tp && pplan.ok) {
        // granule tags repeat from request to request: every rank's window is zeroed between two barriers -- nobody is
        // still writing into it from the previous request, nobody writes before it is clean
        if (!tp_scratch) {
            FTCF_HIP_CHECK(hipMalloc((void**)&tp_scratch, 256));
            FTCF_HIP_CHECK(hipMemsetAsync(tp_scratch, 0, 256, stream));
        }
        comm_barrier(cfg.comm, stream, tp_scratch);
        // (this rank's own window: with fake peers it is the only one, whatever the rank)
        FTCF_HIP_CHECK(hipMemsetAsync(cfg.comm->win[fake_peers() ? 0 : cfg.tensor_para_rank], 0, (size_t)2 * tpn * H * 8, stream));
        comm_barrier(cfg.comm, stream, tp_scratch);
    }

    // ---- runtime args: routing of TopKSamplingLayer.cu:27-77 / TopPSamplingLayer.cu:30-110 ----
    auto top_k = broadcast_arg<int>(a.top_k, a.n_top_k, batch, 0, "top_k");
    auto top_p = broadcast_arg<float>(a.top_p, a.n_top_p, batch, 0.f, "top_p");
    auto temp  = broadcast_arg<float>(a.temperature, a.n_temperature, batch, 1.f, "temperature");
    auto rep   = broadcast_arg<float>(a.repetition_penalty, a.n_repetition_penalty, batch, 1.f, "repetition_penalty");
    auto seed  = broadcast_arg<uint64_t>(a.random_seed, a.n_random_seed, batch, 0, "random_seed");
    auto minl  = broadcast_arg<int>(a.min_length, a.n_min_length, batch, 0, "min_length");
    auto divr  = broadcast_arg<float>(a.beam_search_diversity_rate, a.n_beam_search_diversity_rate, batch, 0.f,
                                      "beam_search_diversity_rate");
    auto lenp  = broadcast_arg<float>(a.len_penalty, a.n_len_penalty, batch, 0.f, "len_penalty");
    const SamplingRouting route = route_sampling_args(top_k, top_p, temp, rep, minl, a.n_repetition_penalty > 0);
    const std::vector<int>&   k_eff  = route.k_eff;
    const std::vector<float>& p_topk = route.p_topk;
    const std::vector<float>& p_topp = route.p_topp;
    FTCF_HIP_CHECK(hipMemcpyAsync(d_top_k, k_eff.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_p_topk, p_topk.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_p_topp, p_topp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_temp, temp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_rep, rep.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_seed, seed.data(), batch * 8, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_min_length, minl.data(), batch * 4, hipMemcpyHostToDevice, stream));
    if (K > 1) {
        FTCF_HIP_CHECK(hipMemcpyAsync(d_div, divr.data(), batch * 4, hipMemcpyHostToDevice, stream));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_lenpen, lenp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    }
    comm_stream_sync(cfg.comm, stream);  // the host vectors die at scope exit

    hipEvent_t e0 = get_event(), e1 = get_event();
    FTCF_HIP_CHECK(hipEventRecord(e0, stream));
    FTCF_HIP_CHECK(hipMemsetAsync(mmha_ws, 0, mmha_workspace_bytes(B, nhl, dh, nsplit), stream));
    FTCF_HIP_CHECK(hipMemsetAsync(chunk_ws, 0, chunk_workspace_bytes(H, std::min(B, 4), 8), stream));
    if (tiled_ws) {  // tickets of the split-K tiles (re-armed by every launch; a failed request may leave one drawn)
        FTCF_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char*>(tiled_ws) + gemm_tiled_workspace_bytes() - gemm_tiled_ticket_bytes(), 0,
                                      gemm_tiled_ticket_bytes(), stream));
    }
    if (smallm_ws) {
        // granules of the batched-decode GEMMs' in-launch reduction: their tags repeat from request to request
        FTCF_HIP_CHECK(hipMemsetAsync(smallm_ws, 0, smallm_partial + gemm_smallm_ticket_bytes(), stream));
    }
    if (spec_plan) {  // tickets of the verify attention, granules and tickets of the verify pass's burst GEMMs
        FTCF_HIP_CHECK(hipMemsetAsync(spec_aws, 0, verify_attention_ticket_bytes(nhl), stream));
        FTCF_HIP_CHECK(hipMemsetAsync(spec_gws, 0, spec_partial + gemm_smallm_ticket_bytes(), stream));
        FTCF_HIP_CHECK(hipMemsetAsync(spec_ndraft, 0, 4 * sizeof(int), stream));
    }
    if (pplan.ok || rplan.ok) {
        const std::vector<PersistLayer> pl = persist_layer_table(layers, k_cache, v_cache, (size_t)B * nhl * s_max * dh);
        FTCF_HIP_CHECK(hipMemcpyAsync(d_players, pl.data(), sizeof(PersistLayer) * L, hipMemcpyHostToDevice, stream));
        if (rplan.ok) {  // the rows kernel's flags are monotone tags of (step, layer): steps repeat from request to request
            FTCF_HIP_CHECK(hipMemsetAsync(rows_ws, 0, rows_flag_bytes(rplan, B, nhl), stream));
        }
        if (pplan.ok) {
            FTCF_HIP_CHECK(hipMemsetAsync(ps_gq, 0, (ps_slab_n + 8) * 8, stream));
        }
        ps_tab_ready = false;
        if (pplan.ok && ps_tab && !(cfg.tensor_para_size > 1 && cfg.comm && cfg.comm->local)) {
            // the run / tile tables of this plan: one launch over no layers builds and stores them, every token's launch
            // loads them (17 us of table building per launch otherwise)
            PersistParams pp = persist_params(B, s_max);
            pp.l_begin = pp.l_end = 0;
            pp.tab_mode = 1;
            pp.d_stop   = nullptr;  // (the flag still holds the previous request's outcome here)
            launch_decode_persistent(pp, int8, stream);
            ps_tab_ready = true;
        }
        comm_stream_sync(cfg.comm, stream);  // `pl` dies at scope exit
    }
    // beam search: the reference tiles the inputs K times and runs the context phase on all batch * K rows
    // (GptNeoX.cc:560-574, 640-735).  Every beam reads the prompt K/V of beam 0 anyway (the cache indirection starts at 0),
    // so the prompt is prefilled once per request into cache row b * K and its last hidden state is tiled.
    const int* in_ids = a.input_ids;
    const int* in_len = a.input_lengths;
    if (K > 1) {
        launch_tile_inputs(tiled_ids, tiled_len, a.input_ids, a.input_lengths, batch, K, S, stream);
        FTCF_HIP_CHECK(hipMemsetAsync(cache_indir, 0, (size_t)2 * B * s_max * 4, stream));
        FTCF_HIP_CHECK(hipMemsetAsync(parent_ids, 0, (size_t)total * B * 4, stream));
        in_ids = tiled_ids;
        in_len = tiled_len;
    }
    launch_decode_init(finished, seq_len, cum, pad_count, masked, draws, in_len, state, B, S, s_max, stream, K);
    if (B <= 2 && !fp32) {  // the tagged partials of k_lm_head_greedy: a tag is the step, and steps repeat from request to request
        FTCF_HIP_CHECK(hipMemsetAsync(samp_ws, 0, lm_head_greedy_partial_bytes(B), stream));
    }
    // what the stats will say of THIS request's overlapped forms: the prompt phase below and the token loop set them
    ov_ran = ov_eligible = false;
    dv_ran = dv_eligible = false;
    prompt_phase(a, in_ids, in_len);
    if (a.context_log_probs) {
        // (ParallelGpt.cc:403-470) px holds the last layer's output of every prompt row, once per request (beams included, tensor
        // parallel ranks alike: the head is replicated): the final LayerNorm, then the fused LM head -> log-prob kernel
        if (S > 1) {
            launch_layernorm(px, final_g, final_b, pnrm, batch * S, H, 1e-5f, true, stream);
            launch_context_log_probs(a.context_log_probs, pnrm, lm_head, a.input_ids, a.input_lengths, ctx_tgt, ctx_lp, batch, S, V, H,
                                     stream);
        }
        else {
            FTCF_HIP_CHECK(hipMemsetAsync(a.context_log_probs, 0, (size_t)batch * S * 4, stream));
        }
    }
    if (a.output_log_probs) {
        FTCF_HIP_CHECK(hipMemsetAsync(olp, 0, (size_t)out_len * B * 4, stream));  // (steps after a row finished hold 0)
    }
    if (a.top_logprobs > 0) {  // (steps after a row finished keep the pattern the buffers start with)
        const size_t pairs = (size_t)out_len * B * a.top_logprobs;
        if (pairs > tlp_pairs) {
            comm_stream_sync(cfg.comm, stream);
            if (tlp_ids) {
                FTCF_HIP_CHECK(hipFree(tlp_ids));
                FTCF_HIP_CHECK(hipFree(tlp_values));
                tlp_ids    = nullptr;
                tlp_values = nullptr;
                tlp_pairs  = 0;
            }
            FTCF_HIP_CHECK(hipMalloc((void**)&tlp_ids, pairs * sizeof(int)));
            FTCF_HIP_CHECK(hipMalloc((void**)&tlp_values, pairs * sizeof(float)));
            tlp_pairs = pairs;
        }
        launch_fill_top_logprobs(tlp_ids, tlp_values, pairs, stream);
    }
    FTCF_HIP_CHECK(hipEventRecord(e1, stream));

    SamplingParams sp{};
    sp.logits = logits;
    sp.B = B;
    sp.V = V;
    sp.max_input_len = S;
    sp.total_len = total;
    sp.end_id = cfg.end_id;
    sp.input_lengths = in_len;
    sp.top_k = d_top_k;
    sp.top_p_topk = d_p_topk;
    sp.top_p_topp = d_p_topp;
    sp.temperature = d_temp;
    sp.repetition_penalty = d_rep;
    sp.min_length = d_min_length;
    route.apply(sp);
    sp.random_seed = d_seed;
    sp.draw_counter = draws;
    sp.stop_words = K > 1 ? nullptr : a.stop_words_list;  // (the beam kernel checks them along the parent chain)
    sp.stop_len = a.stop_words_len;
    sp.optional_last_tokens = a.optional_last_tokens;
    sp.optional_count = a.optional_last_tokens_count;
    // (output_log_probs needs the soft-max statistics: sampling_topk_kernels.cu:273 switches them on for either output)
    sp.return_cum_log_probs = (a.return_cum_log_probs || a.output_log_probs || a.top_logprobs > 0) ? 1 : 0;
    sp.output_ids = step_ids;
    sp.finished = finished;
    sp.seq_len = seq_len;
    sp.cum_log_probs = cum;
    sp.output_log_probs = a.output_log_probs ? olp : nullptr;
    if (a.top_logprobs > 0) {  // (the step then takes the general form: kernels_sampling.hip dynamic_decode_is_*_fused)
        sp.top_logprobs       = a.top_logprobs;
        sp.top_logprob_ids    = tlp_ids;
        sp.top_logprob_values = tlp_values;
    }
    sp.pad_count = pad_count;
    sp.state = state;
    sp.h_flags = h_flags;
    sp.ws = samp_ws;
    if (!fp32 && H % 8 == 0) {  // k_greedy_decode prepares the next token's input itself (no k_step_prologue launch then)
        sp.next_x    = x;
        sp.wte       = wte;
        sp.rot_table = rot_table;
        sp.H         = H;
        sp.rot       = cfg.rotary_embedding_dim;
    }

    BeamParams bp{};
    if (K > 1) {
        bp.logits = logits;
        bp.B = batch;
        bp.K = K;
        bp.V = V;
        bp.max_input_len = S;
        bp.total_len = total;
        bp.end_id = cfg.end_id;
        bp.s_max = s_max;
        bp.input_lengths = in_len;
        bp.temperature = d_temp;
        bp.repetition_penalty = a.n_repetition_penalty > 0 ? d_rep : nullptr;  // penalty type None otherwise
        bp.diversity_rate = d_div;
        bp.len_penalty = d_lenpen;
        bp.min_length = route.any_min ? d_min_length : nullptr;
        bp.stop_words = a.stop_words_list;
        bp.stop_len = a.stop_words_len;
        bp.optional_last_tokens = a.optional_last_tokens;
        bp.optional_count = a.optional_last_tokens_count;
        bp.output_ids = step_ids;
        bp.parent_ids = parent_ids;
        bp.finished = finished;
        bp.seq_len = seq_len;
        bp.cum_log_probs = cum;
        bp.cache_indir = cache_indir;
        bp.state = state;
        bp.ws = beam_ws;
    }

    ses.active = true;
    ses.a = a;
    ses.sp = sp;
    ses.bp = bp;
    ses.K = K;
    ses.batch = batch;
    ses.B = B;
    ses.S = S;
    ses.total = total;
    ses.s_max = s_max;
    ses.next_step = S;
    ses.steps = 0;
    ses.path_logged = false;
    ses.all_finished = false;
    ses.e0 = e0;
    ses.e1 = e1;
    ses.spec   = spec_plan;
    ses.spec_K = a.speculative_tokens;
    ses.spec_N = a.speculative_ngram > 0 ? a.speculative_ngram : 3;
    ses.spec_nd = ses.spec_steps = ses.spec_drafted = ses.spec_accepted = 0;
    stats.decode_ms = 0.f;
}

// enqueues one iteration of the token loop (GptNeoX.cc:776-1048) on `stream` (and the side stream)
void ftcf_gptneox::enqueue_step(bool with_decoder)
{
    const ftcf_forward_args& a = ses.a;
    const int B = ses.B, S = ses.S, s_max = ses.s_max;
    const int tp = cfg.tensor_para_size;
    if (with_decoder && fp32) {
        launch32_step_prologue(F(x), F(wte), step_ids, &state->step, rot_table, pad_count, B, H, cfg.rotary_embedding_dim,
                               stream);
        decoder32(B, s_max);
    }
    else if (with_decoder) {
            // (an all-greedy batch: the previous token's k_greedy_decode has written this token's embedding row and rotary
            // table already -- unless this is the request's first dynamic-decode step, a one-token prompt)
            if (!(ses.K == 1 && ses.sp.next_x && ses.steps > 0 && dynamic_decode_is_fused(ses.sp, true))) {
                launch_step_prologue(x, wte, step_ids, &state->step, rot_table, pad_count, B, H, cfg.rotary_embedding_dim,
                                     stream, &state->all_finished);
            }
            decoder(B, s_max);
        }
        // final LayerNorm (GptNeoX.cc:854-863) is fused into the LM-head GEMV for m <= 4
        const bool fuse_ln = B <= 4 && !fp32;
        if (!fuse_ln) {
            launch_layernorm(x, final_g, final_b, nrm, B, H, 1e-5f, !fp32, stream);
        }
        auto lm = [&](const f16* Wrows, float* out, int rows, int ld) {
            if (fp32) {  // Wrows counts f16 elements: the caller's row offset is scaled here
                launch32_lm_head(F(nrm), F(lm_head) + (Wrows - lm_head), out, B, rows, H, ld, stream);
            }
            else if (fuse_ln) {
                launch_lm_head(x, Wrows, out, B, rows, H, ld, stream, final_g, final_b, 1e-5f, &state->all_finished);
            }
            else {
                lm_head_dispatch(nrm, Wrows, out, B, rows, H, ld, stream);
            }
        };
        // one GPU, <= 2 rows, an all-greedy step: the LM head launch picks the tokens, closes the step and prepares the next
        // token's input itself (k_lm_head_greedy) -- nothing is launched behind it
        const bool lm_greedy = tp == 1 && fuse_ln && ses.K == 1 && !logits_hook && lm_head_greedy_ok(ses.sp, H);
        if (lm_greedy) {
            timed(KIND_LM_HEAD, 2.0 * V * H,
                  [&] { launch_lm_head_greedy(x, lm_head, logits, H, final_g, final_b, 1e-5f, ses.sp, stream); });
        }
        else if (tp == 1) {
            timed(KIND_LM_HEAD, 2.0 * V * H, [&] { lm(lm_head, logits, V, V); });
        }
        else {
            // rank r computes rows [r*vl, (r+1)*vl) of the replicated lm_head (GptNeoX.cc:888-925)
            float* mine = gather + (size_t)cfg.tensor_para_rank * B * vl;
            timed(KIND_LM_HEAD, 2.0 * vl * H,
                  [&] { lm(lm_head + (size_t)cfg.tensor_para_rank * vl * H, mine, vl, vl); });
            allgather_logits(gather, logits, B, stream);
        }
        if (a.debug_logits) {
            FTCF_HIP_CHECK(hipMemcpyAsync(a.debug_logits + (size_t)(ses.next_step - S) * B * V, logits,
                                          (size_t)B * V * 4, hipMemcpyDeviceToDevice, stream));
        }
        if (logits_hook && ses.K == 1) {
            logits_hook(logits, B, stream);
        }
    if (ses.K > 1) {
        dynamic_decode_layer.forward(ses.bp, ses.sp, stream);
    }
    else if (!lm_greedy) {
        dynamic_decode_layer.forward(ses.sp, stream);
    }
}

// the token loop of GptNeoX<T>::forward (GptNeoX.cc:776-1048); returns the number of iterations executed
int ftcf_gptneox::step(int max_steps)
{
    Range r("ftcf.step");
    FTCF_CHECK_ARG(ses.active, "no request in flight: call ftcf_gptneox_begin first");
    FTCF_HIP_CHECK(hipSetDevice(cfg.device));
    if (ses.spec) {
        return step_speculative(max_steps);
    }
    const ftcf_forward_args& a = ses.a;
    const int B = ses.B, S = ses.S, total = ses.total;
    const int tp = cfg.tensor_para_size;
    std::vector<int> h_tokens(B), h_idx(B), h_seq(B);
    hipEvent_t ea = get_event(), eb = get_event();
    FTCF_HIP_CHECK(hipEventRecord(ea, stream));
    // (read per call, not once per process: the tests switch it between engines)
    const int graph_tokens_cfg = getenv("FTCF_GRAPH_TOKENS") ? atoi(getenv("FTCF_GRAPH_TOKENS")) : 8;
    int  done    = 0;
    bool lagging = false;  // the host has not yet seen the flags of the token launched last
    int  lag_slot = 0;     // launches of the pipelined loop so far (two events alternate)
    while (done < max_steps && ses.next_step < total && !ses.all_finished) {
        const int  step         = ses.next_step;
        const bool with_decoder = !(S > 1 && step == S);
        // (with tensor parallelism the step contains RCCL collectives or the exchange windows' spins: not captured -- a capture
        // of the RCCL form aborted inside this image's HIP runtime, profiles/r05_notes.md)
        const bool graph_ok     = use_graph && with_decoder && !profiling && tp == 1 && !a.debug_logits && !logits_hook;
        // Several tokens per graph launch (FTCF_GRAPH_TOKENS, default 8): a graph launch costs ~14 us of GPU idle time between
        // two tokens (profiles/r03_notes.md section 6), and every kernel of a persistent-path token returns at once when the
        // device-side "every row has finished" flag is set, so the tokens of a graph behind the request's last one cost a few
        // microseconds each, not a decoder pass.  Persistent decode path, no streaming callback, one GPU.
        const int  graph_tokens = std::max(1, std::min(64, graph_tokens_cfg));
        const bool multi        = graph_ok && graph_tokens > 1 && pplan.ok && ses.K == 1 && !a.callback && tp == 1
                                  && max_steps - done >= graph_tokens && total - step >= graph_tokens;
        int launched = 1;
        if (graph_ok) {
            hipGraphExec_t& ge = multi ? ses.graph_exec_n : ses.graph_exec;
            if (!ge) {
                // capture the regular decode step(s) (all pointers are fixed for the session, the step counter lives
                // on the device) and replay: no per-kernel host launch cost, cross-stream fork/join become edges
                hipGraph_t g = nullptr;
                FTCF_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                try {
                    for (int t = 0; t < (multi ? graph_tokens : 1); t++) {
                        enqueue_step(true);
                    }
                }
                catch (...) {
                    (void)hipStreamEndCapture(stream, &g);
                    if (g) {
                        (void)hipGraphDestroy(g);
                    }
                    throw;
                }
                FTCF_HIP_CHECK(hipStreamEndCapture(stream, &g));
                FTCF_HIP_CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
                FTCF_HIP_CHECK(hipGraphDestroy(g));
            }
            FTCF_HIP_CHECK(hipGraphLaunch(ge, stream));
            launched = multi ? graph_tokens : 1;
        }
        else {
            enqueue_step(with_decoder);
        }
        if (a.debug_logits) {
            // (logits are modified in place by the decode kernels; the tap is taken inside enqueue_step when eager)
        }
        ses.steps += launched;
        ses.next_step += launched;
        done += launched;
        // The reference synchronises once per token here (stop_criteria_kernels.cu:149-156).  Without a streaming
        // callback nothing on the host needs token t before token t+1 is enqueued, so the replayed graph of the next
        // token(s) is launched first and the host only waits for the PREVIOUS launch's event: the GPU never idles for the
        // host round trip (~25 us per token).  `finished` is sticky on the device and the launches behind the last token
        // return at once; the host's counters are set back to the device's when it learns of the end (below).
        if (graph_ok && !a.callback && tp == 1) {  // (tp > 1: every rank must leave the loop at the SAME token -> synchronous)
            hipEvent_t& ev = tok_ev[lag_slot & 1];
            if (!ev) {
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            }
            FTCF_HIP_CHECK(hipEventRecord(ev, stream));
            if (lagging) {
                comm_event_sync(cfg.comm, tok_ev[(lag_slot - 1) & 1]);
                ses.all_finished = h_flags[0] != 0;
            }
            lag_slot++;
            lagging = true;
            continue;
        }
        lagging = false;
        comm_stream_sync(cfg.comm, stream);
        ses.all_finished = h_flags[0] != 0;
        if (a.callback && step + 1 < total && cfg.tensor_para_rank == 0) {
            // pybind_callback_utils.cc:22-103: last token of every row; a row that did not advance reports end_id
            FTCF_HIP_CHECK(hipMemcpy(h_tokens.data(), step_ids + (size_t)step * B, (size_t)B * 4, hipMemcpyDeviceToHost));
            FTCF_HIP_CHECK(hipMemcpy(h_seq.data(), seq_len, (size_t)B * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < B; b++) {
                h_idx[b] = h_seq[b];
                if (h_seq[b] != step) {
                    h_tokens[b] = cfg.end_id;
                }
            }
            a.callback(h_tokens.data(), h_idx.data(), ses.batch, ses.K, a.callback_user);
        }
    }
    FTCF_HIP_CHECK(hipEventRecord(eb, stream));
    comm_event_sync(cfg.comm, eb, "the prefill");
    if (lagging) {
        ses.all_finished = h_flags[0] != 0;
    }
    if (ses.all_finished && ses.K == 1) {
        // launches behind the token that finished the last row did nothing on the device (every kernel of a token returns at
        // once on the flag, k_decode_finish included: the device's step counter stopped): the host's counters follow the
        // device's, so that `steps_done` is the reference's loop count (GptNeoX.cc:776-1048 leaves its loop at that token)
        const int over = ses.next_step - (h_flags[1] + 1);
        if (over > 0) {
            ses.next_step -= over;
            ses.steps -= over;
            done -= over;
        }
    }
    float ms = 0.f;
    FTCF_HIP_CHECK(hipEventElapsedTime(&ms, ea, eb));
    stats.decode_ms += ms;
    event_pool.push_back(ea);
    event_pool.push_back(eb);
    return done;
}

// One verify pass: the token of position step - 1 and `drafts` drafted tokens as R = drafts + 1 rows of the
// one sequence through the batched decode layers in their grouped form (ParallelResidualDecoder, layers.hip.h: the burst GEMM pairs
// [QKV, FFN1] -> attention -> [out-proj, FFN2], residual + both LayerNorms in one pass) with the verify attention, then the final
// LayerNorm, the LM head on R rows and the acceptance kernel, which closes the step as the greedy kernels do.  The K / V rows of
// rejected drafts stay in the cache beyond the sequence's length; the next step overwrites them.
void ftcf_gptneox::verify_pass(int st, int drafts)
{
    Range r("ftcf.verify_pass");
    const int    R = drafts + 1, len = st - 1, s_max = ses.s_max, rot = cfg.rotary_embedding_dim;
    const size_t cache_l = (size_t)ses.B * nhl * s_max * dh;
    launch_verify_embed(vx, wte, step_ids, spec_draft, st, R, H, stream);
    launch_verify_rotary(vrot, len, R, rot, stream);
    ParallelResidualDecoder walk = layer_walk();
    walk.tp = 1;  // (a request speculates at TP = 1 only: no layer of the pass all-reduces)
    walk.x = vx, walk.nrm = vnrm, walk.nrm2 = vnrm2, walk.qkv = vqkv, walk.ctx = vctx, walk.att = vatt, walk.ffn = vffn, walk.mid = vmid;
    walk.ws = spec_gws, walk.partial = spec_partial;
    walk.forward(
        R, DecodeGemms::grouped,
        [&](int l, const LayerWeights& w, int, int, hipStream_t s) {
            VerifyAttnParams ap{};
            ap.qkv       = vqkv;
            ap.qkv_bias  = w.qkv.bias;
            ap.k_cache   = k_cache + l * cache_l;
            ap.v_cache   = v_cache + l * cache_l;
            ap.rot_table = rot > 0 ? vrot : nullptr;
            ap.ctx       = vctx;
            ap.ws        = spec_aws;
            ap.len       = len;
            ap.R         = R;
            ap.nh        = nhl;
            ap.dh        = dh;
            ap.rot       = rot;
            ap.s_max     = s_max;
            launch_verify_attention(ap, s);
        },
        [](f16*, size_t, hipStream_t, bool) {}, [&](double bytes, auto&& launch, hipStream_t s) { timed(KIND_SMALLM, bytes, launch, s); });
    launch_layernorm(vx, final_g, final_b, vnrm, R, H, 1e-5f, true, stream);
    timed(KIND_LM_HEAD, 2.0 * V * H, [&] { lm_head_dispatch(vnrm, lm_head, vlogits, R, V, H, V, stream); });
    VerifyAcceptParams vp{};
    vp.logits     = vlogits;
    vp.R          = R;
    vp.V          = V;
    vp.step       = st;
    vp.end_id     = cfg.end_id;
    vp.draft      = spec_draft;
    vp.output_ids = step_ids;
    vp.finished   = finished;
    vp.seq_len    = seq_len;
    vp.state      = state;
    vp.h_flags    = h_flags;
    vp.argmax_ws  = spec_argmax;
    launch_verify_accept(vp, stream);
    // what the next plain step expects of the step before it (k_greedy_decode's tail): the embedding row of the last token emitted
    // and the rotary table of its position
    launch_step_prologue(x, wte, step_ids, &state->step, rot_table, pad_count, 1, H, rot, stream, &state->all_finished);
}

// The token loop of a request that speculates.  Every iteration ends with the draft kernel for the NEXT step and one host
// synchronisation, which tells the host the tokens emitted, the end of the request and whether the next step has drafts: a
// verify pass then, the plain decode step (its captured graph) otherwise.  Never more than max_steps tokens per call and never
// past output_len: a pass is cut to what is left.
int ftcf_gptneox::step_speculative(int max_steps)
{
    const ftcf_forward_args& a = ses.a;
    const int  S = ses.S, total = ses.total;
    hipEvent_t ea = get_event(), eb = get_event();
    FTCF_HIP_CHECK(hipEventRecord(ea, stream));
    int done = 0;
    while (done < max_steps && ses.next_step < total && !ses.all_finished) {
        const int  st           = ses.next_step;
        const bool with_decoder = !(S > 1 && st == S);
        const int  nd = with_decoder ? std::min(std::min(ses.spec_nd, ses.spec_K), std::min(total - st - 1, max_steps - done - 1)) : 0;
        if (nd > 0) {
            verify_pass(st, nd);
        }
        else if (use_graph && with_decoder && !profiling) {
            if (!ses.graph_exec) {
                hipGraph_t g = nullptr;
                FTCF_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
                try {
                    enqueue_step(true);
                }
                catch (...) {
                    (void)hipStreamEndCapture(stream, &g);
                    if (g) {
                        (void)hipGraphDestroy(g);
                    }
                    throw;
                }
                FTCF_HIP_CHECK(hipStreamEndCapture(stream, &g));
                FTCF_HIP_CHECK(hipGraphInstantiate(&ses.graph_exec, g, nullptr, nullptr, 0));
                FTCF_HIP_CHECK(hipGraphDestroy(g));
            }
            FTCF_HIP_CHECK(hipGraphLaunch(ses.graph_exec, stream));
        }
        else {
            enqueue_step(with_decoder);
        }
        // the next step's drafts: the caller's (draft_ids from the generated index of the device's step on) or the n-gram lookup
        // over the tokens so far
        launch_ngram_draft(step_ids, 0, &state->step, ses.spec_K, ses.spec_N, a.draft_ids, S, total - S, spec_draft, spec_ndraft,
                           h_flags + 4, &state->all_finished, stream);
        comm_stream_sync(cfg.comm, stream);
        const int emitted = nd > 0 ? h_flags[3] : 1;
        if (nd > 0) {
            ses.spec_steps++;
            ses.spec_drafted += nd;
            ses.spec_accepted += h_flags[5];
        }
        ses.steps += emitted;
        ses.next_step += emitted;
        done += emitted;
        ses.all_finished = h_flags[0] != 0;
        ses.spec_nd      = h_flags[4];
    }
    FTCF_HIP_CHECK(hipEventRecord(eb, stream));
    comm_event_sync(cfg.comm, eb, "the token loop");
    float ms = 0.f;
    FTCF_HIP_CHECK(hipEventElapsedTime(&ms, ea, eb));
    stats.decode_ms += ms;
    event_pool.push_back(ea);
    event_pool.push_back(eb);
    return done;
}

void ftcf_gptneox::finish()
{
    Range r("ftcf.finish");
    FTCF_CHECK_ARG(ses.active, "no request in flight");
    const ftcf_forward_args& a = ses.a;
    // setOutputTensors (GptNeoX.cc:1090-1181)
    if (ses.K > 1) {
        launch_gather_tree_beam(a.output_ids, a.sequence_lengths, step_ids, parent_ids, seq_len, tiled_len, ses.batch,
                                ses.K, ses.S, ses.total, cfg.end_id, stream);
    }
    else {
        launch_gather_tree(a.output_ids, a.sequence_lengths, step_ids, seq_len, a.input_lengths, ses.B, ses.S,
                           ses.total, cfg.end_id, stream);
    }
    if (a.cum_log_probs) {
        FTCF_HIP_CHECK(hipMemcpyAsync(a.cum_log_probs, cum, (size_t)ses.B * 4, hipMemcpyDeviceToDevice, stream));
    }
    if (a.output_log_probs) {
        launch_transpose_log_probs(a.output_log_probs, olp, ses.total - ses.S, ses.B, stream);
    }
    if (a.top_logprobs > 0) {
        launch_transpose_top_logprobs(a.top_logprob_ids, a.top_logprob_values, tlp_ids, tlp_values, ses.total - ses.S, ses.B,
                                      a.top_logprobs, stream);
    }
    int ps_error = 0, smallm_error = 0;
    if (pplan.ok) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&ps_error, ps_err, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    if (smallm_ws) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&smallm_error, reinterpret_cast<char*>(smallm_ws) + smallm_partial, sizeof(int),
                                      hipMemcpyDeviceToHost, stream));
    }
    int rows_error = 0;
    if (rplan.ok) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&rows_error, rows_ws, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    comm_stream_sync(cfg.comm, stream);
    float ms = 0.f;
    FTCF_HIP_CHECK(hipEventElapsedTime(&ms, ses.e0, ses.e1));
    stats.prefill_ms   = ms;
    stats.decode_steps = ses.steps;
    stats.spec_active   = ses.spec ? 1 : 0;
    stats.spec_steps    = ses.spec_steps;
    stats.spec_drafted  = ses.spec_drafted;
    stats.spec_accepted = ses.spec_accepted;
    if (ov_eligible && ov_trial < 2) {  // a trial of the auto mode: every rank keeps the slowest rank's time
        const int us   = comm_max(cfg.comm, (int)(ms * 1000.f), stream, tp_scratch);
        ov_ms[ov_trial] = us * 1e-3f;
        ov_trial++;
        if (ov_trial == 2) {
            FT_LOG_INFO(cfg.device, "prompt-phase all-reduce overlap (auto): plain %.2f ms, overlapped %.2f ms -> %s", ov_ms[0], ov_ms[1],
                        ov_ms[1] < ov_ms[0] ? "overlapped from now on" : "plain from now on");
        }
    }
    if (dv_eligible && dv_trial < 2 && ses.steps > 0) {  // a trial of the decode overlap's auto mode (engine.hip.h decoder_overlapped)
        const int us = comm_max(cfg.comm, (int)(stats.decode_ms * 1000.f / ses.steps), stream, tp_scratch);
        dv_ms[dv_trial] = us * 1e-3f;
        dv_trial++;
        if (dv_trial == 2) {
            FT_LOG_INFO(cfg.device, "decode all-reduce overlap (auto): plain %.3f ms per step, overlapped %.3f -> %s", dv_ms[0], dv_ms[1],
                        dv_ms[1] < dv_ms[0] ? "overlapped from now on" : "plain from now on");
        }
    }
    stats.decode_overlap            = dv_ran ? 1 : 0;
    stats.decode_step_ms_plain      = dv_ms[0];
    stats.decode_step_ms_overlapped = dv_ms[1];
    stats.prefill_overlap        = ov_ran ? 1 : 0;
    stats.prefill_ms_plain       = ov_ms[0];
    stats.prefill_ms_overlapped  = ov_ms[1];
    event_pool.push_back(ses.e0);
    event_pool.push_back(ses.e1);
    ses.e0 = ses.e1 = nullptr;
    ses.active = false;
    if (ses.graph_exec) {
        (void)hipGraphExecDestroy(ses.graph_exec);
        ses.graph_exec = nullptr;
    }
    if (ses.graph_exec_n) {
        (void)hipGraphExecDestroy(ses.graph_exec_n);
        ses.graph_exec_n = nullptr;
    }
    drain_events();
    if (pplan.ok && ps_ts) {
        std::vector<long long> h((size_t)pplan.NB * L * 128);
        FTCF_HIP_CHECK(hipMemcpy(h.data(), ps_ts, h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(ps_ts_file.c_str(), "wb")) {
            const int hdr[4] = {pplan.NB, L, 8, 16};
            fwrite(hdr, 4, 4, f);
            fwrite(h.data(), 8, h.size(), f);
            fclose(f);
        }
    }
    if (rplan.ok && rows_ts) {
        std::vector<long long> h((size_t)rplan.NB * L * 128);
        FTCF_HIP_CHECK(hipMemcpy(h.data(), rows_ts, h.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = fopen(ps_ts_file.c_str(), "wb")) {
            const int hdr[4] = {rplan.NB, L, 8, 16};
            fwrite(hdr, 4, 4, f);
            fwrite(h.data(), 8, h.size(), f);
            fclose(f);
        }
    }
    if (rplan.ok && persist_fail_once) {  // the same test hook for the rows kernel
        persist_fail_once = 0;
        rows_error        = 99;
    }
    if (rplan.ok && cfg.tensor_para_size > 1) {
        if (!tp_scratch) {
            FTCF_HIP_CHECK(hipMalloc((void**)&tp_scratch, 256));
            FTCF_HIP_CHECK(hipMemsetAsync(tp_scratch, 0, 256, stream));
        }
        rows_error = comm_max(cfg.comm, rows_error, stream, tp_scratch);
    }
    if (pplan.ok && persist_fail_once) {  // test hook (FTCF_PERSIST_FAIL_ONCE=1): pretend the kernel gave up once
        persist_fail_once = 0;
        ps_error          = 99;
    }
    if (pplan.ok && cfg.tensor_para_size > 1) {
        ps_error = comm_max(cfg.comm, ps_error, stream, tp_scratch);  // every rank learns of any rank's failure
    }
    if (cfg.tensor_para_size > 1 && cfg.comm && cfg.comm->ar_seq > 0 && !cfg.comm->ar_failed) {
        // the window all-reduce's sticky give-up word (a peer that never arrived: its bounded waits ran out), agreed on
        int ar_err = 0;
        FTCF_HIP_CHECK(hipMemcpy(&ar_err, cfg.comm->ar_sync + 2, sizeof(int), hipMemcpyDeviceToHost));
        if (!tp_scratch) {
            FTCF_HIP_CHECK(hipMalloc((void**)&tp_scratch, 256));
            FTCF_HIP_CHECK(hipMemsetAsync(tp_scratch, 0, 256, stream));
        }
        ar_err = comm_max(cfg.comm, ar_err, stream, tp_scratch);
        if (ar_err != 0) {
            cfg.comm->ar_failed = true;  // this communicator keeps RCCL (or the emulation) for the prompt phase from now on
            winar_failed        = true;
            throw Error(-2, "exchange-window all-reduce gave up waiting for a peer (its kernel was not running next to this one)");
        }
    }
    if (h_flags[2] != 0) {  // k_lm_head_greedy's finishing workgroup never saw some workgroup's partial (cannot happen: bounded all the same)
        h_flags[2] = 0;
        throw Error(-2, "LM head + greedy decode: the finishing workgroup gave up waiting for the partials of the launch");
    }
    if (smallm_error != 0) {
        throw Error(-2, "batched decode GEMM: a split-K reducer gave up waiting for its sibling workgroups' partial sums");
    }
    if (rows_error != 0) {
        persist_failed = true;
        rows           = 0;  // the next request (and the replay of this one) is planned on the general path
        throw Error(-2, "rows decode kernel gave up waiting for a hand-off (code " + std::to_string(rows_error)
                            + "): not every workgroup was resident");
    }
    if (ps_error != 0) {
        persist_failed = true;
        persist        = 0;  // whoever drives begin / step / finish: the next request is planned off the persistent path
        throw Error(-2, "persistent decode kernel gave up waiting for a hand-off (code " + std::to_string(ps_error)
                            + "): not every workgroup was resident");
    }
}

extern "C" int ftcf_gptneox_create(const ftcf_gptneox_config* cfg, const ftcf_gptneox_weights* w, ftcf_gptneox_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(cfg && w && out, "NULL argument");
        require_device();
        FTCF_CHECK_ARG(cfg->pipeline_para_size == 1, "pipeline_para_size must be 1 (the CodeFuse harness forces it)");
        if (cfg->dtype != FTCF_FP16 && cfg->dtype != FTCF_FP32) {
            throw Error(FTCF_ERR_UNSUPPORTED, "the GPU engine instantiates fp16 and fp32 (as GptNeoXOp.cc:56-105)");
        }
        FTCF_CHECK_ARG(cfg->int8_mode == 0 || cfg->int8_mode == 1, "int8_mode must be 0 or 1");
        if (cfg->dtype == FTCF_FP32 && cfg->int8_mode != 0) {
            throw Error(FTCF_ERR_UNSUPPORTED, "weight-only int8 needs half activations (CutlassFpAIntBGemmRunner<half, uint8_t>)");
        }
        const int tp = cfg->tensor_para_size;
        FTCF_CHECK_ARG(tp >= 1 && cfg->head_num % tp == 0 && cfg->inter_size % tp == 0 && cfg->vocab_size % tp == 0,
                       "head_num, inter_size and vocab_size must be divisible by tensor_para_size");
        const int L = cfg->num_layer;
        FTCF_CHECK_ARG(w->n_weights == 12 * L + 4, "weights must hold 12*L+4 tensors");
        FTCF_CHECK_ARG(L >= 1 && L <= 256, "num_layer must be in 1..256");
        FTCF_HIP_CHECK(hipSetDevice(cfg->device));
        FT_LOG_INFO(cfg->device, "GptNeoX engine on device %d: %d layers, %d heads x %d, inter %d, vocab %d, rotary %d, %s%s, "
                                 "tensor_para %d/%d, %s residual",
                    cfg->device, L, cfg->head_num, cfg->size_per_head, cfg->inter_size, cfg->vocab_size, cfg->rotary_embedding_dim,
                    cfg->dtype == FTCF_FP32 ? "fp32" : "fp16", cfg->int8_mode ? " + int8 weights" : "", cfg->tensor_para_rank, tp,
                    cfg->use_gptj_residual ? "parallel" : "sequential");
        auto e   = std::make_unique<ftcf_gptneox>();
        e->cfg   = *cfg;
        e->L     = L;
        e->dh    = cfg->size_per_head;
        e->H     = cfg->head_num * cfg->size_per_head;
        e->nhl   = cfg->head_num / tp;
        e->hl    = e->nhl * e->dh;
        e->il    = cfg->inter_size / tp;
        e->V     = cfg->vocab_size;
        e->vl    = e->V / tp;
        e->int8  = cfg->int8_mode == 1;
        e->fp32  = cfg->dtype == FTCF_FP32;
        e->user_stream = (hipStream_t)cfg->stream;
        FTCF_HIP_CHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        FTCF_HIP_CHECK(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
        FTCF_HIP_CHECK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        FTCF_HIP_CHECK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
        FTCF_HIP_CHECK(hipEventCreateWithFlags(&e->ev_user, hipEventDisableTiming));
        // weights still being uploaded / produced on the caller's stream happen-before the re-tiling below
        FTCF_HIP_CHECK(hipEventRecord(e->ev_user, e->user_stream));
        FTCF_HIP_CHECK(hipStreamWaitEvent(e->stream, e->ev_user, 0));
        if (e->fp32) {
            FTCF_CHECK_ARG(e->dh >= 32 && e->dh <= 256 && e->dh % 2 == 0, "size_per_head must be even, 32..256");
        }
        else {
            // the reference's list (DecoderSelfAttentionLayer.cc:280-282).  64 and 128 run every decode path; the other sizes
            // take the general path (one attention launch per layer): the persistent and the fused per-stage kernels, and the
            // paged attention of the batcher, keep their two tuned lane layouts
            FTCF_CHECK_ARG(mmha_head_size_supported(e->dh), "size_per_head must be one of 32, 48, 64, 80, 96, 128, 144, 160, 192, 224, 256");
            FTCF_CHECK_ARG(e->H % 64 == 0 && e->hl % 64 == 0 && e->il % 64 == 0,
                           "hidden, local hidden and local inter sizes must be multiples of 64");
        }
        if (e->int8) {
            FTCF_CHECK_ARG(w->n_int8_weights == 4 * L && w->n_scales == 4 * L, "int8 lists must hold 4*L tensors");
        }
        auto W = [&](int g, int l) { return w->weights[(size_t)g * L + l]; };
        e->layers.resize(L);
        const int H = e->H, hl = e->hl, il = e->il;
        for (int l = 0; l < L; l++) {
            LayerWeights& lw = e->layers[l];
            lw.ln1_b = (const f16*)W(0, l);
            lw.ln1_g = (const f16*)W(1, l);
            lw.qkv.bias = (const f16*)W(3, l);
            lw.attn_out.bias = (const f16*)W(5, l);
            lw.ffn1.bias = (const f16*)W(7, l);
            lw.ffn2.bias = (const f16*)W(9, l);
            lw.ln2_b = (const f16*)W(10, l);
            lw.ln2_g = (const f16*)W(11, l);
            FTCF_CHECK_ARG(lw.ln1_b && lw.ln1_g && lw.ln2_b && lw.ln2_g && lw.qkv.bias && lw.ffn1.bias && lw.ffn2.bias,
                           "missing layernorm / bias tensor");
            FTCF_CHECK_ARG(cfg->use_gptj_residual || lw.attn_out.bias,
                           "use_gptj_residual == 0 needs the attention output bias (weights[5*L + l])");
            if (e->int8) {
                lw.qkv.kernel = w->int8_weights[0 * L + l];
                lw.attn_out.kernel = w->int8_weights[1 * L + l];
                lw.ffn1.kernel = w->int8_weights[2 * L + l];
                lw.ffn2.kernel = w->int8_weights[3 * L + l];
                lw.qkv.scale = (const f16*)w->scales[0 * L + l];
                lw.attn_out.scale = (const f16*)w->scales[1 * L + l];
                lw.ffn1.scale = (const f16*)w->scales[2 * L + l];
                lw.ffn2.scale = (const f16*)w->scales[3 * L + l];
                FTCF_CHECK_ARG(lw.qkv.kernel && lw.attn_out.kernel && lw.ffn1.kernel && lw.ffn2.kernel && lw.qkv.scale
                                   && lw.attn_out.scale && lw.ffn1.scale && lw.ffn2.scale,
                               "missing int8 kernel / scale tensor");
            }
            else if (e->fp32) {
                // row-major [K, N] fp32 kernels are read in place
                lw.qkv.kernel = W(2, l);
                lw.attn_out.kernel = W(4, l);
                lw.ffn1.kernel = W(6, l);
                lw.ffn2.kernel = W(8, l);
                FTCF_CHECK_ARG(lw.qkv.kernel && lw.attn_out.kernel && lw.ffn1.kernel && lw.ffn2.kernel, "missing fp32 kernel tensor");
            }
            else {
                // re-tile the reference-layout [K, N] fp16 kernels once (the binding keeps the originals alive)
                struct {
                    int          g;
                    size_t       K, N;
                    DenseWeight* d;
                } items[4] = {{2, (size_t)H, (size_t)3 * hl, &lw.qkv},
                              {4, (size_t)hl, (size_t)H, &lw.attn_out},
                              {6, (size_t)H, (size_t)il, &lw.ffn1},
                              {8, (size_t)il, (size_t)H, &lw.ffn2}};
                // FTCF_FP16_RETILE_IN_PLACE=1: the caller's row-major kernels are OVERWRITTEN with the tiled image (through one
                // bounce buffer) instead of being kept next to a tiled copy -- the engine then holds one copy of the fp16 weights
                // (26 GB instead of 52 GB at 13B); the caller must not read those tensors as [K, N] matrices afterwards
                const bool in_place = getenv("FTCF_FP16_RETILE_IN_PLACE") && atoi(getenv("FTCF_FP16_RETILE_IN_PLACE")) != 0;
                for (auto& it : items) {
                    const void* src = W(it.g, l);
                    FTCF_CHECK_ARG(src != nullptr, "missing fp16 kernel tensor");
                    const size_t bytes = it.K * it.N * 2;
                    if (in_place) {
                        if (e->bounce_bytes < bytes) {
                            if (e->bounce) {
                                FTCF_HIP_CHECK(hipStreamSynchronize(e->stream));
                                (void)hipFree(e->bounce);
                            }
                            FTCF_HIP_CHECK(hipMalloc(&e->bounce, bytes));
                            e->bounce_bytes = bytes;
                        }
                        launch_fp16_rowmajor_to_tiled((const f16*)src, it.K, it.N, (f16*)e->bounce, e->stream);
                        FTCF_HIP_CHECK(hipMemcpyAsync(const_cast<void*>(src), e->bounce, bytes, hipMemcpyDeviceToDevice, e->stream));
                        it.d->kernel = src;
                        continue;
                    }
                    void* dst = nullptr;
                    FTCF_HIP_CHECK(hipMalloc(&dst, bytes));
                    e->owned.push_back(dst);
                    launch_fp16_rowmajor_to_tiled((const f16*)src, it.K, it.N, (f16*)dst, e->stream);
                    it.d->kernel = dst;
                }
            }
        }
        e->wte     = (const f16*)w->weights[12 * L];
        e->final_g = (const f16*)w->weights[12 * L + 1];  // GptNeoXOp.h:172-173: slot 12L+1 = gamma
        e->final_b = (const f16*)w->weights[12 * L + 2];
        e->lm_head = (const f16*)w->weights[12 * L + 3];
        FTCF_CHECK_ARG(e->wte && e->final_g && e->final_b && e->lm_head, "missing embedding / final layernorm / lm_head");
        e->k3_q = e->fp32 ? 1 : chunk_pick_q(e->H / 16, (e->hl + e->il) / (e->int8 ? TILE_K_I8 : TILE_K_F16));
        if (const char* m = getenv("FTCF_STAGE_MAX_ROWS")) {
            e->STAGE_MAX_ROWS = std::max(0, std::min(4, atoi(m)));
        }
        if (const char* m = getenv("FTCF_SMALLM_MAX_ROWS")) {
            e->SMALLM_MAX_ROWS = std::max(16, std::min(256, atoi(m)));
        }
        {
            hipDeviceProp_t prop;
            FTCF_HIP_CHECK(hipGetDeviceProperties(&prop, cfg->device));
            e->num_cu = prop.multiProcessorCount;
        }
        if (const char* m = getenv("FTCF_PERSIST")) {
            e->persist = atoi(m);
        }
        if (const char* m = getenv("FTCF_ROWS")) {
            e->rows = atoi(m);
        }
        if (const char* m = getenv("FTCF_ROWS_NB")) {
            e->rows_nb = atoi(m);
        }
        if (const char* m = getenv("FTCF_PERSIST_FAIL_ONCE")) {
            e->persist_fail_once = atoi(m);
        }
        if (const char* m = getenv("FTCF_TP_PERSIST")) {
            e->persist_tp = atoi(m);
        }
        if (const char* m = getenv("FTCF_PERSIST_TS")) {
            e->ps_ts_file = m;
        }
        if (const char* m = getenv("FTCF_PERSIST_NB")) {
            e->persist_nb = atoi(m);
        }
        if (const char* m = getenv("FTCF_PERSIST_CS1")) {
            e->persist_cs1 = atoi(m);
        }
        if (const char* m = getenv("FTCF_PERSIST_CS3")) {
            e->persist_cs3 = atoi(m);
        }
        if (const char* m = getenv("FTCF_PERSIST_OWN")) {  // 0: P3 as K pieces merged by an owner (the form until round 5), 1: own-group
                                                            // layout wherever the shape divides, 2 (default): where it measured faster
            e->persist_own = atoi(m);
        }
        e->decode_branches = cfg->tensor_para_size == 1 ? 1 : 0;
        if (const char* m = getenv("FTCF_DECODE_BRANCHES")) {
            e->decode_branches = atoi(m);
        }
        e->use_graph = cfg->use_hip_graph != 0;
        if (const char* m = getenv("FTCF_TP_PAIR_AR")) {
            e->tp_pair_ar = atoi(m) != 0;
        }
        if (const char* m = getenv("FTCF_USE_GRAPH")) {
            e->use_graph = atoi(m) != 0;
        }
        if (cfg->tensor_para_size > 1) {
            // scratch word of the communicator helpers (comm_barrier / comm_max / comm_agree): every path of a tensor-parallel
            // engine may reach them (the prompt-phase overlap's trials, the kernels' error words), whatever it planned
            FTCF_HIP_CHECK(hipMalloc((void**)&e->tp_scratch, 256));
            FTCF_HIP_CHECK(hipMemsetAsync(e->tp_scratch, 0, 256, e->stream));
        }
        FTCF_HIP_CHECK(hipHostMalloc((void**)&e->h_flags, 64, hipHostMallocDefault));
        e->h_flags[0] = e->h_flags[1] = e->h_flags[2] = 0;
        FTCF_HIP_CHECK(hipStreamSynchronize(e->stream));
        if (e->bounce) {
            (void)hipFree(e->bounce);
            e->bounce       = nullptr;
            e->bounce_bytes = 0;
        }
        *out = e.release();
    });
}

extern "C" int ftcf_gptneox_forward(ftcf_gptneox_t h, const ftcf_forward_args* args)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h && args, "NULL argument");
        h->forward(*args);
    });
}

extern "C" int ftcf_gptneox_begin(ftcf_gptneox_t h, const ftcf_forward_args* args)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h && args, "NULL argument");
        h->begin(*args);
    });
}
extern "C" int ftcf_gptneox_step(ftcf_gptneox_t h, int max_steps, int* steps_done)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h, "NULL argument");
        const int n = h->step(max_steps);
        if (steps_done) {
            *steps_done = n;
        }
    });
}
extern "C" int ftcf_gptneox_finish(ftcf_gptneox_t h)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h, "NULL argument");
        h->finish();
    });
}

extern "C" int ftcf_gptneox_get_stats(ftcf_gptneox_t h, ftcf_forward_stats* s)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h && s, "NULL argument");
        *s = h->stats;
        // dominant weight-streaming kernel kind
        int best = 0;
        for (int k = 1; k < KIND_COUNT; k++) {
            if (h->kind_ms[k] > h->kind_ms[best]) {
                best = k;
            }
        }
        s->gemv_kind     = best;
        s->gemv_ms_sum   = (float)h->kind_ms[best];
        s->gemv_launches = h->kind_n[best];
        s->gemv_bytes    = h->kind_bytes[best];
    });
}

extern "C" int ftcf_gptneox_set_profiling(ftcf_gptneox_t h, int enabled)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h, "NULL argument");
        h->profiling = enabled != 0;
        for (int k = 0; k < KIND_COUNT; k++) {
            h->kind_ms[k] = h->kind_bytes[k] = 0;
            h->kind_n[k]                     = 0;
        }
    });
}

extern "C" int ftcf_gptneox_destroy(ftcf_gptneox_t h)
{
    return guarded([&] { delete h; });
}
