/*
 * ftcf.h -- C ABI of libftcf.so: the MI355X (gfx950) native engine for the GPT-NeoX / CodeFuse decode path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / pybind types.  The reference's Python
 * extension modules (`libth_gptneox.GptNeoXOp`, `libth_common`) are thin bindings over these entry points
 * (see INTEGRATION.md).  All paths below are relative to the reference tree root.
 *
 * Conventions
 *   - "device pointer" = HIP device memory of the device the handle was created on; "host pointer" = CPU memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - every function returns 0 on success, a negative ftcf_status otherwise; ftcf_last_error() gives the text.
 *     (The reference prints and exit(-1)s on engine errors, th_op/gptneox/GptNeoXOp.h:370-380; the bindings raise.)
 *   - fp16 tensors are IEEE binary16 (`dtype` FTCF_FP16), fp32 tensors `float`.
 */
#ifndef FTCF_H
#define FTCF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTCF_VERSION 100

typedef enum {
    FTCF_OK              = 0,
    FTCF_ERR_INVALID_ARG = -1,
    FTCF_ERR_HIP         = -2,
    FTCF_ERR_UNSUPPORTED = -3,
    FTCF_ERR_COMM        = -4,
    FTCF_ERR_NO_DEVICE   = -5
} ftcf_status;

typedef enum { FTCF_FP32 = 0, FTCF_FP16 = 1, FTCF_BF16 = 2 /* host quantiser input only */ } ftcf_dtype;
typedef enum { FTCF_ACT_NONE = 0, FTCF_ACT_GELU = 1 } ftcf_act;

const char* ftcf_last_error(void);
int         ftcf_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int ftcf_device_count(void);

/* ================================================================================================
 * libth_common counterpart -- host side weight-only quantiser
 *   replaces: th_op/common/WeightOnlyQuantOps.cc:140-233,344-349
 *             (symmetric_quantize_last_axis_of_batched_matrix_int8) and
 *             kernels/cutlass_kernels/cutlass_preprocessors.cc:576-673 (symmetric_quantize) +
 *             :500-539 (preprocess_weights_for_mixed_gemm -- here: the gfx950 tile layout)
 * ================================================================================================ */
/* weight: host [E, K, N] row major (E = 1 for a 2-D matrix), dtype FTCF_FP32, FTCF_FP16 or FTCF_BF16
 * (WeightOnlyQuantOps.cc:149,205).
 * out_q : host int8 [E, K, N] bytes, ENGINE-PRIVATE gfx950 tile layout (opaque, like the reference's).
 * out_scale: host [E, N] in the weight dtype.  Requires K % 64 == 0 and N % 16 == 0. */
int ftcf_symmetric_quantize_int8(const void* weight, ftcf_dtype dtype, size_t E, size_t K, size_t N, int8_t* out_q,
                                 void* out_scale);
/* Device form of ftcf_symmetric_quantize_int8: weight [E, K, N] row major ON THE DEVICE, out_q [E, K, N] bytes in the
 * engine tile layout and out_scale [E, N] in the weight dtype on the device, bit for bit what the host function returns
 * for the same values.  Asynchronous on `stream`; out-of-place (weight is not modified); workspace:
 * ftcf_symmetric_quantize_int8_device_workspace(E, N) = E * N * 4 bytes (the fp32 column maxima), no initial contents
 * required.  The four pointers are 16-byte aligned.  Covers every input whose column maximum / 128 is a normal fp32 number
 * or zero (fp16 subnormal weights and fp16 subnormal scales included; fp32 weights below about 2^-119 are not).
 * The workspace query is host arithmetic and answers without a device. */
int    ftcf_symmetric_quantize_int8_device(const void* weight, ftcf_dtype dtype, size_t E, size_t K, size_t N,
                                           int8_t* out_q, void* out_scale, void* workspace, size_t workspace_bytes,
                                           void* stream);
size_t ftcf_symmetric_quantize_int8_device_workspace(size_t E, size_t N);
/* row-major int8 [K,N] (the reference's "unprocessed" tensor) <-> engine tile layout (host) */
int ftcf_int8_rowmajor_to_tiled(const int8_t* q_rowmajor, size_t K, size_t N, int8_t* q_tiled);
int ftcf_int8_tiled_to_rowmajor(const int8_t* q_tiled, size_t K, size_t N, int8_t* q_rowmajor);
/* int8 [K,N] as a CUDA build of the reference stores it for SM75..SM89 -- what its `.q.bin` files hold
 * (preprocess_weights_for_mixed_gemm, cutlass_preprocessors.cc:500-539; quant_and_save.py:20) -- <-> row major (host).
 * K % 64 == 0, N % 2 == 0.  Importing a CUDA checkpoint = cuda_sm80_to_rowmajor followed by rowmajor_to_tiled. */
int ftcf_int8_cuda_sm80_to_rowmajor(const int8_t* q_cuda, size_t K, size_t N, int8_t* q_rowmajor);
int ftcf_int8_rowmajor_to_cuda_sm80(const int8_t* q_rowmajor, size_t K, size_t N, int8_t* q_cuda);
/* device: fp16 [K,N] row major -> engine fp16 tile layout (out-of-place, K % 32 == 0, N % 16 == 0) */
int ftcf_fp16_rowmajor_to_tiled(const void* w_rowmajor, size_t K, size_t N, void* w_tiled, void* stream);

/* ================================================================================================
 * kernel-level entry points (device pointers).  One per reference `invoke*` / runner on the hot path;
 * used by the parity tests and by the engine itself.
 * ================================================================================================ */
/* CutlassFpAIntBGemmRunner<half,uint8_t>::gemm / gemm_bias_act
 *   (kernels/cutlass_kernels/fpA_intB_gemm/fpA_intB_gemm.h:39-106, fpA_intB_gemm_template.h:511-581):
 *   C[m,n] = half( sum_k A[m,k] * half(q[k,n]*scale[n])  (+bias[n], gelu) ), A/C/scale/bias fp16, q tiled int8. */
int ftcf_fpA_intB_gemm(const void* A, const int8_t* B_tiled, const void* scales, const void* bias, ftcf_act act,
                       void* C, int m, int n, int k, void* stream);
/* cublasMMWrapper::Gemm (utils/cublasMMWrapper.cc:94-386) for the fp16 engine: C[m,n] = half(A[m,k] * W), W tiled fp16;
 * optional fused bias+gelu reproduces invokeAddBiasGeluV2 (kernels/activation_kernels.cu:401-426). */
int ftcf_fp16_gemm(const void* A, const void* W_tiled, const void* bias, ftcf_act act, void* C, int m, int n, int k,
                   void* stream);
/* The form the two GEMMs above run (m, n, k) in above 16 rows (the tiled MFMA GEMM; the engine and the batcher launch it through
 * the same decision).  Host only: no device is needed or touched.  has_workspace: whether the caller holds the split-K workspace;
 * the two entry points above hold one for 17 <= m <= the largest split-K row count of either weight type (768).  The decision
 * reads FTCF_GEMM_SPLITK and FTCF_GEMM_SK128_MIN_M at every call and FTCF_GEMM_SPLITK_MAX_M once per process, as the launch does.
 * m >= 1, n % 16 == 0, k % 64 == 0, else FTCF_ERR_INVALID_ARG. */
typedef struct {
    int family;          /* 0 split-K, 1 32-row form, 2 one workgroup per tile, 3 four-wave form (fp16 weights) */
    int tile_rows;       /* 32 / 48 / 64 / 128 */
    int gx, gy;          /* column blocks (256 columns; 64 in the 32-row form), row blocks */
    int slices;          /* K slices per tile; 1 outside the split-K family */
    int steps_per_slice; /* k-steps (64 k) per slice; the last slice holds the remainder */
    int ring;            /* ring depth in k-steps: 0 (plain loop), 2 or 4 */
    int prefetch;        /* A fragments prefetched */
    int two_per_cu;      /* register budget of two workgroups per CU */
    int lone;            /* one workgroup per tile: at most 256 tiles */
    int grid;            /* workgroups launched */
} ftcf_gemm_plan;
int ftcf_gemm_tiled_plan(int m, int n, int k, int int8, int has_workspace, ftcf_gemm_plan* out);
/* LM head (models/gptneox/GptNeoX.cc:866-912): logits_f32[m, n] = A[m,k] (fp16) x W[n,k]^T (fp16, row major [V,H]) */
int ftcf_lm_head(const void* A, const void* W_nk, float* logits, int m, int n, int k, int ldc, void* stream);
/* The same LM head with the final LayerNorm (GptNeoX.cc:854-863) fused in front, as the engine's token loop runs it for <= 4
 * rows: logits_f32[m, n] = LN(A; gamma, beta, eps)[m, k] x W[n, k]^T, the LayerNorm with ftcf_layernorm's fp16 numerics.
 * 1 <= m <= 4, k % 8 == 0, ldc >= n (a tensor-parallel rank writes its vocabulary slice of a wider row).  d_stop (device int, or
 * NULL): the "every row has finished" flag -- when it is set the launch writes nothing. */
int ftcf_lm_head_layernorm(const void* A, const void* W_nk, const void* gamma, const void* beta, float eps, const int* d_stop,
                           float* logits, int m, int n, int k, int ldc, void* stream);
/* Batched-decode GEMM in the form the engine launches it (general path at 5..16 rows, short prompt phases, the continuous
 * batcher, the speculative verify pass): one launch for ONE or TWO independent GEMMs with the same m,
 * C[m, n] = epilogue(A[m, k] x W), W tiled int8 (with scale [n]) or tiled fp16, act FTCF_ACT_GELU = bias + gelu.  K is cut in
 * slices of 20 tiles (64 k each int8, 32 fp16); the partial sums of all slices but the last travel through `workspace` as
 * {tag, value} granules and the owner of the last slice adds them in slice order.
 *   workspace: [partial_bytes of granules][ftcf_gemm_smallm_ticket_bytes()], caller owned, all zero before the first launch;
 *     the int at byte partial_bytes is a sticky error word (0 = fine).  The problems of one launch take
 *     ftcf_gemm_smallm_workspace_bytes(m, n, k, int8) bytes each, back to back from partial_offset; launches that may run
 *     concurrently (two streams) use disjoint [partial_offset, ...) regions of one workspace.
 *   d_step: device int that is part of the launch's tag (the engine's decode step; read at run time), or NULL.
 *   launch_counter: host counter of the workspace, part of the tag; every launch increments it.
 * 1 <= m <= 16, n % 16 == 0, k % 64 == 0. */
typedef struct {
    const void* A;     /* [m, k] fp16 */
    const void* W;     /* tiled int8 / fp16 [k, n] */
    const void* scale; /* [n] fp16 (int8 only) */
    const void* bias;  /* [n] fp16 or NULL */
    int         act;   /* ftcf_act */
    void*       C;     /* [m, n] fp16 */
    int         n, k;
} ftcf_smallm_problem;
int    ftcf_gemm_smallm_group(const ftcf_smallm_problem* problems, int np, int m, int int8, void* workspace, size_t partial_bytes,
                              size_t partial_offset, const int* d_step, unsigned* launch_counter, void* stream);
size_t ftcf_gemm_smallm_workspace_bytes(int m, int n, int k, int int8);
size_t ftcf_gemm_smallm_ticket_bytes(void);
/* One pass over x [m, n] (in place) for a parallel-residual layer of the batched paths: with ffn != NULL first the previous
 * layer's invokeAddBiasAttentionFfnResidual, x = residual(ffn * sum_mul, attn * sum_mul, x / tp, bias * bias_mul) (the products
 * in fp32, rounded to half once; inplace_variant as ftcf_add_bias_attn_ffn_residual), then out1 = LN(x; g1, b1) and
 * out2 = LN(x; g2, b2) with the element sets and summation order of ftcf_layernorm (bit-identical to it).  g1 == NULL: the
 * residual only, out1 / out2 untouched.  n % 8 == 0 and n <= 8192, anything else is FTCF_ERR_INVALID_ARG. */
int ftcf_residual_dual_layernorm(void* x, const void* ffn, const void* attn, const void* bias, int tp, int inplace_variant,
                                 const void* g1, const void* b1, const void* g2, const void* b2, void* out1, void* out2, int m, int n,
                                 float eps, int bias_mul, int sum_mul, void* stream);
/* Sequential-residual layers (use_gptj_residual == 0; invokeAddBiasResidual, kernels/add_residual_kernels.cu:22-60):
 * out = half((bias + a) + b) with the sums in fp32; bias [n] or NULL; out may alias a or b. */
int ftcf_add_bias_residual(void* out, const void* a, const void* b, const void* bias, int m, int n, void* stream);
/* The per-stage decode step's LayerNorm -> GEMV launch for 1..4 rows: out0 [m, N0] = half(LN(x; gamma0, beta0) x W0) (QKV: no
 * bias) and / or out1 [m, N1] = gelu(LN(x; gamma1, beta1) x W1 + bias1) (FFN1), W tiled int8 (scale0 / scale1) or fp16.  A
 * segment with N = 0 is absent.  wpg = 0: four column groups per workgroup, one wave each; wpg 1..4: one column group per
 * workgroup, wpg waves splitting K.  K % 64 == 0, N0 % 16 == 0, N1 % 16 == 0; x [m, K] must fit the LDS (m * K <= ~32000). */
typedef struct {
    const void* x;
    const void *gamma0, *beta0, *gamma1, *beta1;
    const void *W0, *W1;
    const void *scale0, *scale1;
    const void* bias1;
    void *      out0, *out1;
    int         K, N0, N1;
    float       eps;
} ftcf_ln_gemv_args;
int ftcf_ln_gemv(const ftcf_ln_gemv_args* args, int m, int int8, int wpg, void* stream);
/* The per-stage decode step's closing launch for 1..4 rows: attn = half(x_a x W_a) (out-projection), ffn = half(x_b x W_b)
 * (FFN2), out = residual(ffn, attn, x_in / tp, bias) as ftcf_add_bias_attn_ffn_residual; out may be x_in.  Q = 0: one workgroup
 * per 16-column group, up to 10 waves over the two K ranges.  Q in 1..8: the concatenated K range [x_a ; x_b] of a column group
 * is cut into Q chunks of ceil(tiles / Q) tiles, one workgroup each; the partial sums travel as {tag, value} granules through
 * `granules` (ftcf_residual_gemv_workspace_bytes(N, m, Q) bytes, caller owned, zero before the first launch; unused for Q <= 1).
 * The tag is (step, salt): step = *d_step when d_step != NULL, else `step`; salt in 0..1023; consecutive launches on one
 * workspace need different tags.  K_a / K_b are whole tiles (64 int8, 32 fp16), N % 16 == 0; a shape whose x slices exceed 64 KiB
 * of LDS is FTCF_ERR_INVALID_ARG. */
typedef struct {
    const void *x_a, *x_b;         /* [m, K_a], [m, K_b] fp16 */
    const void *W_a, *W_b;         /* tiled [K_a, N], [K_b, N] */
    const void *scale_a, *scale_b; /* [N] fp16 (int8 only) */
    const void* bias;              /* [N] */
    const void* x_in;              /* [m, N] */
    void*       out;               /* [m, N] */
    int         N, K_a, K_b;
    int         tp, inplace_variant;
} ftcf_residual_gemv_args;
int    ftcf_residual_gemv(const ftcf_residual_gemv_args* args, int m, int int8, int Q, void* granules, size_t granule_bytes,
                          const int* d_step, int step, int salt, void* stream);
size_t ftcf_residual_gemv_workspace_bytes(int N, int m, int Q);
/* Fused LM head -> log-probability of a target token (the prompt-scoring kernel behind context_log_probs; the reference writes
 * the logits and runs kernels/logprob_kernels.cu:36-100 over them).  For each row r, l_j = sum_k A[r,k] W[j,k] (fp16 products,
 * fp32 accumulation, as ftcf_lm_head), log_probs[r] = l[targets[r]] - logsumexp_j l_j; targets[r] < 0 (or >= n) gives 0.
 * row_logsumexp [m] or NULL.  A [m, k] fp16, W [n, k] fp16 row major (the engine's lm_head), targets [m] int32, k % 8 == 0;
 * all device pointers.  Deterministic: two calls give identical bits.  Workspace is internal (kept per device and stream). */
int ftcf_lm_head_log_probs(const void* A, const void* W_nk, const int* targets, float* log_probs, float* row_logsumexp, int m, int n,
                           int k, void* stream);
/* invokeGeneralLayerNorm (kernels/layernorm_kernels.cu:1652-1735), fp16 half2 path numerics (:157-286) */
int ftcf_layernorm(const void* x, const void* gamma, const void* beta, void* out, int m, int n, float eps,
                   ftcf_dtype dtype, void* stream);
/* invokeAddBiasAttentionFfnResidual (kernels/add_residual_kernels.cu:116-178) */
int ftcf_add_bias_attn_ffn_residual(void* out, const void* ffn, const void* attn, const void* in, const void* bias,
                                    int m, int n, int tp, int inplace_variant, ftcf_dtype dtype, void* stream);
/* fusedQKV_masked_attention_dispatch (layers/attention_layers/DecoderSelfAttentionLayer.cc:36-146 ->
 * kernels/decoder_masked_multihead_attention/decoder_masked_multihead_attention_template.hpp:1099-1919).
 * qkv [B,3*Hl] fp16; caches are engine private: k_cache/v_cache [B, nh, s_max, dh] fp16. */
int ftcf_masked_multihead_attention(const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache,
                                    const int* seq_len, const int* pad_count, const uint8_t* masked_tokens,
                                    const uint8_t* finished, int B, int nh, int dh, int rot, int s_max, int step,
                                    void* ctx, void* workspace, size_t workspace_bytes, void* stream);
size_t ftcf_masked_multihead_attention_workspace(int B, int nh, int dh, int s_max);
/* The same step with beam search's arguments and an explicit split count.  dtype FTCF_FP16 or FTCF_FP32 (qkv, qkv_bias, caches
 * and ctx all of that type).  cache_indir [2][B][s_max] int32 or NULL: the key / value of time t < seq_len[b] of row b is read from
 * cache row (b / beam_width) * beam_width + cache_indir[(step - max_input_len) & 1][b][t]; the new key / value goes to row b's own
 * line.  Every entry of both planes, over all s_max positions, must be in [0, beam_width): the kernel may dereference entries
 * beyond seq_len[b].  B = batch * beam_width rows; NULL launches the form without beams (beam_width, max_input_len unused).
 * fp16: nsplit = 0 takes the launcher's own split count (that of ftcf_masked_multihead_attention_workspace), 1..16 forces one;
 * workspace_bytes >= B * nh * nsplit * (dh + 2) * 8 (one 8-byte granule per partial element), and a split's scores
 * (roundup16(ceil(s_max / nsplit)) floats) must fit 64 KiB of LDS beside 22 * dh + 32 bytes.  fp32: nsplit and workspace are ignored
 * (one workgroup per (row, head)); the call returns after the launch has finished.  A bad argument is an error return, never a
 * failed launch. */
int ftcf_masked_multihead_attention_beams(ftcf_dtype dtype, const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache,
                                          const int* seq_len, const int* pad_count, const uint8_t* masked_tokens,
                                          const uint8_t* finished, const int* cache_indir, int beam_width, int max_input_len, int B,
                                          int nh, int dh, int rot, int s_max, int step, int nsplit, void* ctx, void* workspace,
                                          size_t workspace_bytes, void* stream);
/* Speculative decoding's verify attention (no counterpart in the reference): decode attention for R
 * consecutive NEW tokens of ONE sequence.  qkv [R, 3*nh*dh] fp16 are the tokens of positions len .. len + R - 1 of the sequence in
 * row `cache_row` of k_cache / v_cache [rows, nh, s_max, dh], whose positions [0, len) are cached.  Row i: bias, NeoX rotary at
 * len + i, its K / V rows stored at len + i, ctx[i] [nh*dh] = soft-max attention of its rotated q over positions [0, len + i] --
 * the arithmetic and rounding points of ftcf_masked_multihead_attention for a step at that position.  The cached keys are
 * read once for all rows.  1 <= R <= 16, len + R <= s_max <= ~32000, dh 64 / 128.  Nothing outside rows [len, len + R) of that cache
 * row is written.  Deterministic: two calls give identical bits.  workspace: ftcf_verify_attention_workspace bytes. */
int ftcf_verify_attention(const void* qkv, const void* qkv_bias, void* k_cache, void* v_cache, int cache_row, int len, int R,
                          int nh, int dh, int rot, int s_max, void* ctx, void* workspace, size_t workspace_bytes, void* stream);
size_t ftcf_verify_attention_workspace(int R, int nh, int dh, int s_max);
/* Prompt-lookup ("n-gram") drafting over the tokens so far t[0, n) (device int32): for g = min(N, n - 1) down to 1, among the
 * start indices s <= n - g - 1 with t[s, s + g) == t[n - g, n) the LARGEST s is taken; the first g that has one wins and the
 * draft is t[s + g, min(s + g + K, n)).  No match: zero drafts.  draft [K] and n_draft [1] are device int32.  1 <= K <= 15,
 * 1 <= N <= 8. */
int ftcf_ngram_draft(const int* tokens, int n, int K, int N, int* draft, int* n_draft, void* stream);
/* The decode tail of a verify pass of a greedy request, bare or with stop words, log-probabilities or a streaming callback (the
 * engine runs it for every greedy pass, whatever ftcf_gptneox_set_speculative_scope says): two launches and nothing else.
 * logits [R, V] fp32 (device, not modified) are the pass's rows: row i is the model's distribution behind the token of position
 * step + i - 1, i.e. behind draft[i - 1] for i >= 1.  a[i] = the arg max of row i (value descending, index ascending on ties);
 * m = the longest prefix with draft[i] == a[i] (draft [R - 1] device int32; NULL with R = 1).  For i = 0 .. m in order:
 *   - a[i] is written to output_ids[step + i] (output_ids [total_len] device int32: ONE sequence, positions [0, step) are its
 *     history) and to tokens[i];
 *   - with cum_log_probs and / or output_log_probs given (device fp32 [1] / [total_len - max_input_len], either may be NULL):
 *     lp = logf(exp(v - row max) / (sum of exp(. - row max) + 1e-6f)) is added to cum_log_probs[0] and stored at
 *     output_log_probs[step + i - max_input_len] -- the value the plain greedy step commits.  The adds are sequential fp32 adds
 *     in i order: a sequential fp32 sum of the stored values reproduces cum_log_probs bit for bit;
 *   - the row finishes when a[i] == end_id, when a stop word ends at position step + i (stop_words [2, stop_len] device int32 or
 *     NULL: the ids back to back, then cumulative end offsets, -1 padded, as stop_words_list of ftcf_forward_args for one row;
 *     a word may straddle the history and the tokens just written; drafts behind position m are never looked at), or when
 *     step + i >= total_len.
 * Nothing is written behind the first token that finishes the row.  *emitted = the tokens written (1 .. m + 1), *accepted = the
 * drafts among them (min(m, emitted)); seq_len[0] += emitted; finished[0] = whether the last token finished the row (device int32
 * [1] / int32 [1] / int32 [1] / uint8 [1]); tokens is device int32 [16].  Every other cell of every buffer keeps its bits.
 * 1 <= R <= 16, max(1, max_input_len) <= step, step + R <= total_len, 0 <= end_id < V; any V.  Deterministic: two calls give identical
 * bits.  workspace: FTCF_VERIFY_ACCEPT_WORKSPACE_BYTES device bytes.  Enqueues on `stream` and does not synchronise.
 * struct_size != sizeof(ftcf_verify_accept_args), R outside 1..16, a NULL tensor other than the optional ones, positions outside
 * the sequence: FTCF_ERR_INVALID_ARG. */
#define FTCF_VERIFY_ACCEPT_WORKSPACE_BYTES 8192
typedef struct ftcf_verify_accept_args {
    int          struct_size;
    int          R, V, step, end_id, max_input_len, total_len;
    const float* logits;
    const int*   draft;
    int*         output_ids;
    const int*   stop_words;
    int          stop_len;
    uint8_t*     finished;
    int*         seq_len;
    float*       cum_log_probs;
    float*       output_log_probs;
    void*        workspace;
    size_t       workspace_bytes;
    int*         emitted;
    int*         accepted;
    int*         tokens;
} ftcf_verify_accept_args;
int ftcf_verify_accept(const ftcf_verify_accept_args* args, void* stream);
/* The decode tail of a verify pass of a TOP-K SAMPLED request (the engine runs it for every pass of a sampled request that began
 * under ftcf_gptneox_set_speculative_sampling(h, 1)): three launches and nothing else.  Everything is ftcf_verify_accept's but
 * a[i]: row i's logits, each multiplied by 1.0f / (temperature + 1e-6f) as it is read when temperature is neither 0 nor 1 (the
 * buffer is not modified), go through the top-k layer of ftcf_dynamic_decode_step -- the top_k best (value descending, index
 * ascending on ties) become exp(v - best) or, with cum_log_probs / output_log_probs given, their soft-max probabilities over the
 * row, and uniform number u = draw (draw_counter[0] + i) of the stream of random_seed walks them up to u * top_p_topk * their sum
 * -- and a[i] is the token the walk stops at; lp = logf(its probability).  The tokens are emitted as there, and
 * draw_counter[0] += emitted (device uint64 [1]).  Row i is reached only behind i accepted rows, i.e. behind exactly i draws: the
 * emitted tokens are those of `emitted` plain sampled steps from the same state, and a rejected row has consumed no draw.
 * top_p_topk: the p of the top-k layer in (0, 1], 1 = all of the k.  1 <= top_k <= 64 and V <= 131072 (else
 * FTCF_ERR_INVALID_ARG, as for every bad argument of ftcf_verify_accept); draw_counter must not be NULL.  Deterministic: two
 * calls from the same state give identical bits.  workspace: FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES device bytes. */
#define FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES 266368
typedef struct ftcf_verify_sample_args {
    int                 struct_size;
    int                 R, V, step, end_id, max_input_len, total_len;
    const float*        logits;
    const int*          draft;
    int*                output_ids;
    const int*          stop_words;
    int                 stop_len;
    uint8_t*            finished;
    int*                seq_len;
    float*              cum_log_probs;
    float*              output_log_probs;
    void*               workspace;
    size_t              workspace_bytes;
    int*                emitted;
    int*                accepted;
    int*                tokens;
    int                 top_k;
    float               top_p_topk;
    float               temperature;
    unsigned long long  random_seed;
    unsigned long long* draw_counter;
} ftcf_verify_sample_args;
int ftcf_verify_sample(const ftcf_verify_sample_args* args, void* stream);
/* GptContextAttentionLayer<T>::forward minus the two projections (layers/attention_layers/
 * GptContextAttentionLayer.cc:142-345): bias + NeoX rotary + cache fill + causal masked softmax(QK^T)V.
 * qkv [B*S, 3*Hl] fp16 (row = b*S+s), ctx [B*S, Hl] fp16. */
int ftcf_context_attention(const void* qkv, const void* qkv_bias, const int* input_lengths, void* k_cache,
                           void* v_cache, int B, int S, int nh, int dh, int rot, int s_max, void* ctx, void* stream);
/* The same prompt attention with every argument of its launcher: a token range [s_lo, s_hi) of each sequence (one chunk of a
 * chunked prompt phase, or the tail of a prompt whose head is cached already) and a cache row multiplier.  dtype FTCF_FP16 or
 * FTCF_FP32 (qkv, qkv_bias, caches and ctx all of that type).  qkv [B*S, 3*Hl] (row = b*S+s), ctx [B*S, Hl], caches
 * [B * cache_row_mult, nh, s_max, dh]: the K/V of sequence b live in cache row b * cache_row_mult.  len = input_lengths[b].
 * Read: qkv rows [s_lo, s_hi) of each sequence and, of its cache row, positions [0, s_lo) below len -- the keys and values of
 * the earlier chunks, which must be there; no other cache element's value reaches a result.
 * Written: for the positions s of [s_lo, s_hi) below len, the q part of qkv row s (bias + NeoX rotary at position s, in place),
 * the K/V rows of position s (V = v + bias, bit exact) and ctx row s = soft-max attention of that q over positions [0, s];
 * for the positions of [s_lo, s_hi) at or above len, zeros into the K/V rows and into the q part of the qkv row.  Nothing
 * else: the k and v parts of qkv, the qkv rows outside the range, the ctx rows outside the range or at and above len, the cache
 * positions outside the range and every other cache row keep their bits.  Deterministic: two calls give identical bits.  fp16: 0 <= s_lo < s_hi <= S.  fp32: the whole prompt only (s_lo
 * = 0, s_hi = S or -1), S + dh + 4 floats must fit 64 KiB of LDS, and the call returns after the launch has finished.
 * B, nh, cache_row_mult >= 1; dh one of 32, 48, 64, 80, 96, 128, 144, 160, 192, 224, 256; rot even, 0 <= rot <= dh; S <= s_max.
 * A bad argument is an error return, never a failed launch. */
int ftcf_context_attention_range(ftcf_dtype dtype, void* qkv, const void* qkv_bias, const int* input_lengths, void* k_cache,
                                 void* v_cache, int B, int S, int nh, int dh, int rot, int s_max, int cache_row_mult, int s_lo,
                                 int s_hi, void* ctx, void* stream);
/* The continuous batcher's decode attention over paged K/V (one layer): the arithmetic of ftcf_masked_multihead_attention for
 * slot b at position lengths[b] (NeoX rotary at that position), the keys of positions [0, lengths[b]) read through
 * page_table[b][t / page_tokens] at row t % page_tokens, the new key / value row appended there.  qkv [B, 3*nh*dh] fp16,
 * qkv_bias [3*nh*dh], k_pool / v_pool [num_pages][nh][page_tokens][dh] fp16, page_table [B][max_pages] int32, lengths [B]
 * int32 (< max_len), finished [B] uint8 (1: slot skipped, nothing read or written), ctx [B, nh*dh] fp16.  dh 64 / 128; a
 * slot's scores stay in LDS, so max_len (= max_pages * page_tokens in the batcher) is bounded (~15000 tokens at dh 128). */
int ftcf_paged_attention(const void* qkv, const void* qkv_bias, void* k_pool, void* v_pool, const int* page_table,
                         const int* lengths, const uint8_t* finished, int B, int nh, int dh, int rot, int page_tokens,
                         int max_pages, int max_len, void* ctx, void* stream);
/* K/V of tokens [0, S) of one sequence, dense -> paged, for L layers: k_cache / v_cache point at the sequence's row of layer 0
 * of a cache [L][rows][nh][s_max][dh] (src_layer_elems = rows * nh * s_max * dh apart; 0: a one-row cache), the pools are
 * [L][num_pages][nh][page_tokens][dh] (pool_layer_elems = num_pages * nh * page_tokens * dh apart), pages [S / page_tokens
 * rounded up] the sequence's page ids.  A bit-exact copy; nothing beyond token S - 1 is written. */
int ftcf_scatter_kv_to_pages(const void* k_cache, const void* v_cache, void* k_pool, void* v_pool, const int* pages, int L, int nh,
                             int dh, int s_max, int S, int page_tokens, size_t pool_layer_elems, size_t src_layer_elems,
                             void* stream);
/* The inverse (the batcher's prefix cache): tokens [0, T) of a sequence's pages -> its row of the dense cache, T a multiple of
 * page_tokens and <= s_max; same layouts and strides as ftcf_scatter_kv_to_pages.  A bit-exact copy. */
int ftcf_gather_pages_to_kv(void* k_cache, void* v_cache, const void* k_pool, const void* v_pool, const int* pages, int L, int nh,
                            int dh, int s_max, int T, int page_tokens, size_t pool_layer_elems, size_t dst_layer_elems,
                            void* stream);
/* The batcher's swap space (ftcf_batcher_create_opts with overcommit): pages pages[0 .. n) of every layer of both pools
 * (layouts and pool_layer_elems as in ftcf_scatter_kv_to_pages) -> a contiguous DEVICE staging buffer
 * [n][2 (K, V)][L][nh * page_tokens * dh] of fp16; pages: DEVICE array of page ids, each < pool_layer_elems / (nh * page_tokens * dh).
 * A bit-exact copy; nothing beyond n pages of the staging buffer is written. */
int ftcf_pages_pack(void* staging, const void* k_pool, const void* v_pool, const int* pages, int n, int L, int nh, int dh,
                    int page_tokens, size_t pool_layer_elems, void* stream);
/* The exact inverse: the staging buffer -> the pages of (another) page list; no other page of the pools is written. */
int ftcf_pages_unpack(const void* staging, void* k_pool, void* v_pool, const int* pages, int n, int L, int nh, int dh,
                      int page_tokens, size_t pool_layer_elems, void* stream);
/* ONE step of the dynamic-decode layer (DynamicDecodeLayer.cc:192-497 with beam_width 1: optional-token mask, temperature,
 * repetition penalty, min-length mask, end mask, top-k / top-p sampling, stop words, length criterion) on the caller's logits and
 * state -- the launch sequence the engine and the continuous batcher run per token, with the same routing of the runtime
 * arguments.  Device buffers of the caller: logits [B, V] fp32 (modified in place), output_ids time-major [rows, B] int32 with
 * rows >= max(total_len, step + 1): the token goes to row `step` (row row_len[b] + 1 with row_len), rows [0, step) are the
 * history the repetition penalty and the stop words read; finished [B] uint8, seq_len [B] int32, cum_log_probs [B] fp32 or
 * NULL, output_log_probs time-major [total_len - max_input_len, B] fp32 or NULL (the value this step adds to cum_log_probs, at
 * row step - max_input_len; row 0 with row_len; it switches the soft-max statistics on as return_cum_log_probs does), draw_counter [B] uint64, pad_count [B] int32 or NULL, input_lengths [B] int32, stop_words [B, 2, stop_len]
 * or NULL, optional_last_tokens [B, optional_count] (-1 padded) or NULL, row_len [B] int32 or NULL (every row at its own step).
 * Runtime arguments: host arrays of 1 or B entries as in ftcf_forward_args, n == 0 "not given".  finish != 0: the step's
 * bookkeeping (stop words, length criterion, padding count) follows, and *all_finished / *next_step (host, may be NULL) receive
 * the state it leaves; finish == 0 is the batcher's form (no bookkeeping: *all_finished 0, *next_step = step).  *form (host,
 * may be NULL): 0 the general four launches, 1 the one-launch top-k step, 2 the one-launch greedy step.  Synchronises the
 * stream.  V > 122880 on the general path and a repetition penalty with total_len > 7680 are FTCF_ERR_INVALID_ARG.
 * top_logprobs = N in 1..20 (appended; 0 = off): top_ids / top_log_probs, time-major [total_len - max_input_len, B, N] int32 / fp32,
 * receive at row step - max_input_len (row 0 with row_len) the N best (id, log-probability) pairs of every row that was not
 * finished before the step, as top_logprobs of ftcf_forward_args defines them; the pairs of a finished row are not written.  The
 * step then takes the general form and the soft-max statistics are on.  N outside 0..20, or N > 0 with a NULL buffer, is
 * FTCF_ERR_INVALID_ARG. */
typedef struct {
    float*          logits;
    int*            output_ids;
    uint8_t*        finished;
    int*            seq_len;
    float*          cum_log_probs;
    float*          output_log_probs;
    uint64_t*       draw_counter;
    int*            pad_count;
    const int*      input_lengths;
    const int*      stop_words;
    const int*      optional_last_tokens;
    const int*      row_len;
    const int*      top_k;
    const float*    top_p;
    const float*    temperature;
    const float*    repetition_penalty;
    const int*      min_length;
    const uint64_t* random_seed;
    int*            all_finished;
    int*            next_step;
    int*            form;
    int n_top_k, n_top_p, n_temperature, n_repetition_penalty, n_min_length, n_random_seed;
    int stop_len, optional_count;
    int B, V, step, max_input_len, total_len, end_id, return_cum_log_probs, finish;
    int    top_logprobs;
    int*   top_ids;
    float* top_log_probs;
} ftcf_dynamic_decode_args;
int ftcf_dynamic_decode_step(const ftcf_dynamic_decode_args* args, void* stream);
/* ONE step of the beam-search layer (OnlineBeamSearchLayer without beam hypotheses: penalties, per-row top K of log-softmax +
 * cum_log_probs, the K best of a batch entry's K * K candidates, parents, lengths, cache indirection, stop words along the
 * parent chain; not the length criterion).  Rows bb = batch * K + beam.  Device buffers of the caller: logits [B * K, V] fp32
 * (modified in place), output_ids / parent_ids time-major [total_len, B * K] int32, finished [B * K] uint8, seq_len [B * K]
 * int32, cum_log_probs [B * K] fp32, cache_indir [2, B * K, s_max] int32 (plane (step - max_input_len) % 2 is read, the other
 * one written), input_lengths [B * K] int32 (tiled), stop_words [B, 2, stop_len] or NULL, optional_last_tokens [B,
 * optional_count] or NULL.  Runtime arguments: host arrays of 1 or B entries, n == 0 "not given".  2 <= K <= 64, V >= K,
 * max(1, max_input_len) <= step < total_len.  Synchronises the stream. */
typedef struct {
    float*       logits;
    int*         output_ids;
    int*         parent_ids;
    uint8_t*     finished;
    int*         seq_len;
    float*       cum_log_probs;
    int*         cache_indir;
    const int*   input_lengths;
    const int*   stop_words;
    const int*   optional_last_tokens;
    const float* temperature;
    const float* repetition_penalty;
    const float* beam_search_diversity_rate;
    const float* len_penalty;
    const int*   min_length;
    int n_temperature, n_repetition_penalty, n_beam_search_diversity_rate, n_len_penalty, n_min_length;
    int stop_len, optional_count;
    int B, K, V, step, max_input_len, total_len, s_max, end_id;
    /* appended: the step's log-probability of every row's token (online_softmax_beamsearch_kernels.cu:241-243: the new
     * cumulative score minus the PARENT's old one, one fp32 subtraction; exactly +0 for a beam that had finished before the
     * step), device, time-major [total_len, B * K] fp32 like output_ids; row `step` is written.  NULL: off, and every other
     * output is bit for bit what it is with the pointer set. */
    float* step_log_probs;
} ftcf_beam_search_args;
int ftcf_beam_search_step(const ftcf_beam_search_args* args, void* stream);
/* Per-request LOGIT PROCESSORS: one stage over logits [batch_size, vocab_size] fp32 (device, modified in place), to run between
 * the LM head and ftcf_dynamic_decode_step (the continuous batcher runs it there: ftcf_batcher_submit_opts /
 * ftcf_batcher_set_token_mask).  A row is processed when row_on[b] != 0 (row_on NULL: every row), finished[b] == 0 (NULL: no row
 * is finished) and at least one option below is set for it; every other row keeps its bits.  For a processed row, in this order:
 *   1. penalties over the GENERATED tokens only (the prompt is the business of the multiplicative repetition_penalty of the
 *      dynamic decode, which runs afterwards): c[t] = occurrences of t among the row's history positions [gen_start[b], len_b),
 *      logit[t] -= presence_penalty[b] * (c[t] > 0) + frequency_penalty[b] * c[t]
 *      (the additive form of kernels/sampling_penalty_kernels.cu);
 *   2. logit[bias_ids[b][i]] += bias_values[b][i] for i < n_bias[b] <= 1024; -INFINITY bans the token.  The ids of a row are
 *      distinct and in [0, vocab_size): the CALLER checks that (ids outside the vocabulary are ignored, a repeated id takes one
 *      of its values);
 *   3. while len_b - gen_start[b] < min_new_tokens[b]: logit[end_id] = -inf;
 *   4. bad words, the reference's word list [2][bad_words_len] per row (ids back to back, then cumulative end offsets, -1
 *      padded; bad_words_len <= 256): a one-token word is banned, an n-token word bans its last token when its first n - 1 are
 *      the last n - 1 tokens of the history, prompt and generated alike (kernels/ban_bad_words.cu:42-85; unlike there token 0
 *      can be banned);
 *   5. mask[b] = ceil(vocab_size / 32) words, bit t clear: logit[t] = -inf (rows with mask_on[b] != 0; mask_on NULL: every row);
 *   6. the guard: a row left without one finite logit gets logit[end_id] = 0 (the sampling kernels never see an all -inf row).
 * History: token t of row b is hist[t * stride_t + b * stride_b] (elements), len_b = hist_len[b] + hist_len_add, gen_start[b]
 * is clamped to [0, len_b]; hist NULL: every history is empty.  All pointers are device pointers; presence_penalty /
 * frequency_penalty / min_new_tokens / n_bias [batch_size] or NULL, bias_ids / bias_values [batch_size, bias_stride].
 * A penalised or biased logit is the exact sum rounded to fp32 once (fp64 inside); banned and masked logits are exactly -inf,
 * every other logit keeps its bits.  Every logit is written by one workgroup: the result does not depend on `slice` (logits per
 * workgroup, a multiple of 32 in [32, 4096]; 0 = the default), and two runs are bit-identical.  Enqueues two launches on
 * `stream` and does not synchronise.  struct_size != sizeof(ftcf_logit_process_args), end_id outside the vocabulary, a bad
 * slice or bad_words_len: FTCF_ERR_INVALID_ARG. */
typedef struct {
    int             struct_size;
    int             batch_size, vocab_size, end_id;
    float*          logits;
    const uint8_t*  finished;
    const uint8_t*  row_on;
    const int*      hist;
    long long       stride_t, stride_b;
    const int*      hist_len;
    const int*      gen_start;
    int             hist_len_add;
    int             bias_stride;
    const float*    presence_penalty;
    const float*    frequency_penalty;
    const int*      min_new_tokens;
    const int*      bias_ids;
    const float*    bias_values;
    const int*      n_bias;
    const int*      bad_words;
    int             bad_words_len;
    int             slice;
    const unsigned* mask;
    const uint8_t*  mask_on;
} ftcf_logit_process_args;
int ftcf_logit_process(const ftcf_logit_process_args* args, void* stream);

/* ================================================================================================
 * libth_gptneox counterpart -- the engine behind GptNeoXOp
 *   replaces: th_op/gptneox/GptNeoXOp.h:69-231 (FTGptNeoX ctor), :246-381 (forward),
 *             models/gptneox/GptNeoX.cc:386-1052 (GptNeoX<T>::forward)
 * ================================================================================================ */
typedef struct ftcf_gptneox* ftcf_gptneox_t;
typedef struct ftcf_comm*    ftcf_comm_t;

/* ---- tensor-parallel communicator (utils/nccl_utils.cc:56-435, th_op/gptneox/utils/nccl_inherit_utils.cc:25-68) ---- */
#define FTCF_UNIQUE_ID_BYTES 128
/* rank 0 creates the id, the caller broadcasts the bytes (e.g. torch.distributed), every rank inits. */
int ftcf_comm_get_unique_id(uint8_t id[FTCF_UNIQUE_ID_BYTES]);
int ftcf_comm_init(const uint8_t id[FTCF_UNIQUE_ID_BYTES], int world_size, int rank, int device, ftcf_comm_t* comm);
int ftcf_comm_destroy(ftcf_comm_t comm);
/* LOCAL GROUP (test infrastructure): the ranks of a tensor-parallel job inside ONE process on ONE device, each driven by
 * its own host thread.  Same engine code path as RCCL ranks (sharding, per-layer all-reduce, vocabulary split, in-kernel
 * exchange); the collectives are host-synchronous.  Lets a single-GPU box execute and check tensor_para_size > 1. */
/* HOST-EXCHANGE communicator: one process per rank as with ftcf_comm_init, but every exchange between the ranks -- the
 * bootstrap, the hipIpc handles of the exchange windows, agreements, barriers, and (staged through host memory) the
 * all-reduce / all-gather of device buffers -- travels through ONE callback of the caller: an all-gather of host bytes
 * over the caller's own process group (e.g. torch.distributed with gloo).  This is what nccl_inherit_utils.cc:25-68 does
 * with the caller's ProcessGroup for the bootstrap, taken one step further: no RCCL communicator is created at all, so the
 * ranks may share one device (the inter-PROCESS path of the in-kernel exchange -- IPC-mapped windows, hand-shake, system
 * scope stores -- runs on a single-GPU box), and a box whose RCCL cannot initialise still gets tensor parallelism.  The
 * decode all-reduce is in the persistent kernel's exchange windows as usual; prefill collectives are host staged (slow).
 * allgather(user, send, recv, bytes): recv[r * bytes .. ] = rank r's send; returns 0 on success. */
typedef int (*ftcf_host_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
int ftcf_comm_init_host_exchange(int world_size, int rank, int device, ftcf_host_allgather_fn allgather, void* user,
                                 ftcf_comm_t* comm);
int ftcf_comm_local_unique_id(uint8_t id[FTCF_UNIQUE_ID_BYTES]);
int ftcf_comm_init_local(const uint8_t id[FTCF_UNIQUE_ID_BYTES], int world_size, int rank, int device, ftcf_comm_t* comm);
/* ftNcclAllReduceSum / ftNcclAllGather (in place, fp16 / fp32) exposed for tests */
int ftcf_comm_allreduce_sum(ftcf_comm_t comm, void* buf, size_t count, ftcf_dtype dtype, void* stream);
int ftcf_comm_allgather(ftcf_comm_t comm, void* buf, size_t count_per_rank, ftcf_dtype dtype, void* stream);

typedef struct {
    int head_num, size_per_head, inter_size, num_layer, vocab_size, rotary_embedding_dim;
    int start_id, end_id;
    int tensor_para_size, tensor_para_rank, pipeline_para_size; /* pipeline_para_size must be 1 */
    int int8_mode;                                               /* 0, or 1 = weight only */
    int dtype; /* ftcf_dtype of `weights` = the engine instantiated, as GptNeoXOp.cc:56-105 selects it from weights[0]:
                * FTCF_FP16 (every decode path, int8_mode 0 / 1) or FTCF_FP32 (FTGptNeoX<float>: fp32 weights, activations and
                * K/V cache, general path, int8_mode 0 only -- the validation instantiation, not tuned) */
    int use_gptj_residual;
    int device;        /* HIP device ordinal */
    void* stream;      /* hipStream_t all work is enqueued on (GptNeoXOp.h:180-185) */
    ftcf_comm_t comm;  /* NULL when tensor_para_size == 1 */
    int use_hip_graph; /* 1: capture the per-token step in a hipGraph when possible */
} ftcf_gptneox_config;

/* Weight contract of GptNeoXOp (GptNeoXOp.h:121-174): `weights` = 12*L+4 device pointers in the order
 * [ln1.beta xL, ln1.gamma xL, qkv.kernel xL, qkv.bias xL, attn_out.kernel xL, attn_out.bias xL, ffn1.kernel xL,
 *  ffn1.bias xL, ffn2.kernel xL, ffn2.bias xL, ln2.beta xL, ln2.gamma xL, wte, final_ln.gamma, final_ln.beta, lm_head];
 * kernels are [K, N/TP] row major; a pointer may be NULL where the reference passes an empty tensor.
 * `int8_weights` = 4*L tiled int8 tensors [qkv xL, attn_out xL, ffn1 xL, ffn2 xL], `scales` = 4*L fp16 vectors.
 * The engine keeps the pointers (the binding keeps the tensors alive, GptNeoXOp.h:402-404). */
typedef struct {
    const void* const* weights;
    int                n_weights;
    const void* const* int8_weights;
    int                n_int8_weights;
    const void* const* scales;
    int                n_scales;
} ftcf_gptneox_weights;

/* per-step streaming callback (th_op/gptneox/utils/pybind_callback_utils.cc:22-103): called on rank 0 after every
 * step but the last with host arrays last_tokens[B*beam] and idxs[B*beam]. */
typedef void (*ftcf_token_callback)(const int* last_tokens, const int* idxs, int batch, int beam, void* user);

typedef struct {
    /* inputs (GptNeoXOp.cc:113-185) */
    const int* input_ids;     /* device [B, max_input_len] */
    const int* input_lengths; /* device [B] */
    int        batch_size, max_input_len, output_len, beam_width;
    /* runtime args: host arrays of size 1 or B; n == 0 means "not given" */
    const int*      top_k;                      int n_top_k;
    const float*    top_p;                      int n_top_p;
    const float*    beam_search_diversity_rate; int n_beam_search_diversity_rate;
    const float*    temperature;                int n_temperature;
    const float*    len_penalty;                int n_len_penalty;
    const float*    repetition_penalty;         int n_repetition_penalty;
    const uint64_t* random_seed;                int n_random_seed;
    const int*      min_length;                 int n_min_length; /* not reachable through GptNeoXOp; kept for parity */
    const int* stop_words_list;      /* device [B, 2, stop_words_len] or NULL */
    int        stop_words_len;
    const int* optional_last_tokens; /* device [B, optional_last_tokens_count] (-1 padded) or NULL */
    int        optional_last_tokens_count;
    int        return_cum_log_probs;
    ftcf_token_callback callback;
    void*               callback_user;
    /* outputs (device) */
    int*   output_ids;       /* [B, beam, max_input_len + output_len] */
    int*   sequence_lengths; /* [B, beam] */
    float* cum_log_probs;    /* [B, beam] or NULL */
    /* optional debug taps (device, may be NULL): raw fp32 logits of every step [output_len, B, V] */
    float* debug_logits;
    /* per-token log-probabilities (device, may be NULL; appended last so that zero-initialised callers are unchanged).
     * output_log_probs [B, beam, output_len] (GptNeoX.cc:418, 967-987): [b, 0, i] is the log-probability of the i-th generated
     *   token, exactly the value that step adds to cum_log_probs -- logf(prob) under the row's soft-max after temperature,
     *   penalties and the min-length / optional-token masks, before top-k / top-p truncation (the reference's top-p definition).
     *   Deliberate difference: the reference's TOP-K kernel stores log P(i | i in top-k) (sampling_topk_kernels.cu:289-301),
     *   which is always 0 for greedy; here top-k rows store the full-soft-max value as top-p rows do.  Steps after a row has
     *   finished hold 0, so a sequential fp32 sum over i reproduces cum_log_probs bit for bit.  Asking for it switches the
     *   soft-max statistics on exactly as return_cum_log_probs = 1 does: tokens are those of that request.  beam_width > 1 is
     *   refused (FTCF_ERR_INVALID_ARG).
     * context_log_probs [B, max_input_len] (ParallelGpt.cc:403-470 is_return_context_cum_log_probs): [b, t] for
     *   1 <= t < input_lengths[b] is log P(input_ids[b, t] | input_ids[b, < t]); [b, 0] and the padding hold 0.  The index is the
     *   token's own position (FT's log_probs[t] holds token t + 1).  Computed once per request by a fused LM-head kernel (the
     *   logits never reach memory; ftcf_lm_head_log_probs); beam requests score the prompt once, the values equal beam_width 1's.
     *   fp32 engines are refused. */
    float* output_log_probs;
    /* The top-N alternative tokens of every step (0 / NULL = off: no kernel is launched and every bit is as before).  The three
     * fields sit with the log-probability outputs, in front of context_log_probs: the speculative fields stay the struct's last
     * ones, so a caller built against an earlier header is rebuilt (callers that zero-initialise and set fields by name are
     * unchanged).
     * With top_logprobs = N in 1..20, top_logprob_ids (int32) and top_logprob_values (fp32), both device [B, 1, output_len, N],
     * receive for every generated position the N best (id, log-probability) pairs of the distribution output_log_probs is
     * defined under: the row after the optional-token mask, temperature, repetition penalty and min-length mask, before top-k /
     * top-p truncation.  Order: log-probability descending, equal values by id ascending (+0.0 and -0.0 are one value).  Value:
     * (v - row_max) - logf(sum of exp(v - row_max) + 1e-6f); for a row of the top-p layer logf of the fp32 probability its
     * soft-max left, which is what output_log_probs holds for the emitted token.  Masked entries (a processed logit of -inf or
     * <= -FLT_MAX, a probability of 0) come after every other entry, by id ascending, with -inf.  With fewer than N tokens in the
     * vocabulary the trailing pairs are (-1, -inf).  Positions after a row has finished hold (-1, 0.0f).  Asking for it switches
     * the soft-max statistics on exactly as return_cum_log_probs = 1 does and changes nothing else: tokens are those of the
     * request with output_log_probs alone.  A greedy row's pair 0 is the emitted token; a top_k = k row's token is among the
     * pairs when N >= k.  Every step takes the general decode form (the one-launch greedy / top-k steps do not produce the
     * pairs): cum_log_probs and output_log_probs are bit for bit those of that form, which may differ in the last bit from the
     * one-launch steps' (another summation order of the soft-max statistics).  beam_width > 1, N outside 0..20 and N > 0 with a NULL buffer are
     * FTCF_ERR_INVALID_ARG; a speculative request that asks for it runs unspeculated. */
    int    top_logprobs;
    int*   top_logprob_ids;
    float* top_logprob_values;
    float* context_log_probs;
    /* Speculative greedy decoding (appended, 0 / NULL = off and every bit as before).  With
     * speculative_tokens = K in 1..15 a step drafts up to K tokens -- the continuation of the most recent earlier occurrence of
     * the last speculative_ngram tokens (N in 1..8, 0 = 3; shorter matches down to one token are tried), or, with draft_ids
     * (device [output_len]), draft_ids[j .. j + K) for a step that starts at generated index j (cut at the first negative id) --
     * and verifies them in ONE decoder pass over drafts + 1 rows; the accepted drafts and the model's own next token are emitted,
     * exactly the tokens plain greedy decoding produces one at a time.  A step with no draft is the plain step; the first step
     * of a request never drafts.  Eligible:
     * batch 1 with input_lengths[0] == max_input_len, beam_width 1, greedy (top_k <= 1 and top_p 0), repetition_penalty 1, no
     * min_length / top_logprobs / debug_logits, fp16 engine (int8_mode 0 / 1), parallel residual, tensor_para_size 1,
     * size_per_head 64 / 128, hidden and inter sizes multiples of 64, at most ~32000 positions -- and, at the engine's default
     * speculative scope 0, no optional_last_tokens / stop words / callback / return_cum_log_probs / output_log_probs.  Under
     * ftcf_gptneox_set_speculative_scope(h, 1) those five no longer exclude a request (a temperature other than 1 together with
     * return_cum_log_probs or output_log_probs still does: it changes the soft-max, not the arg max): tokens and sequence
     * lengths are those of the request without the fields, the callback is invoked once per emitted token with the arguments of
     * the unspeculated request, in its order, cum_log_probs is the sequential fp32 sum of output_log_probs, and both agree with
     * the unspeculated request's as two GEMM forms do (a pass runs the burst GEMMs).
     * An ineligible request is not an error: it runs as without the fields and ftcf_forward_stats.spec_active says so.
     * speculative_tokens outside 0..15 or speculative_ngram outside 0..8: FTCF_ERR_INVALID_ARG. */
    int        speculative_tokens;
    int        speculative_ngram;
    const int* draft_ids;
} ftcf_forward_args;

typedef struct {
    float prefill_ms;      /* HIP-event time of the context phase of the last forward */
    float decode_ms;       /* HIP-event time of the token loop of the last forward */
    int   decode_steps;    /* executed loop iterations */
    float gemv_ms_sum;     /* sum over timed weight-streaming launches (only when profiling is enabled) */
    long  gemv_launches;
    double gemv_bytes;     /* algorithmic weight bytes those launches streamed */
    int   gemv_kind;       /* which launch kind those three describe: 0 LN->QKV, 1 out-proj+FFN2, 2 LM head,
                              3 MMHA||FFN1, 4 persistent decode layers, 5 batched-decode burst GEMM pair */
    int   decode_path;     /* decoder of the last request: 0 per-stage launches, 1 persistent layers (one launch per
                              token, or per layer with tensor parallelism), 2 general (batched GEMM) path */
    /* tensor parallel, prompt phase: did the last request run its per-layer all-reduce on the side stream under the other
     * micro-batch's GEMMs (FTCF_PREFILL_OVERLAP = 1, or chosen by the auto mode), and what the auto mode's two timed trials
     * took (plain / overlapped, ms, the slowest rank's; 0 until that trial has run) */
    int   prefill_overlap;
    float prefill_ms_plain, prefill_ms_overlapped;
    /* all-reduces of the last request that went through the peer-mapped exchange windows instead of RCCL (the two-shot kernel
     * for prompt-phase messages; FTCF_TP_WINAR=0 switches it off, FTCF_TP_WINAR_MB sizes its buffers: 16) */
    int   window_allreduces;
    /* tensor parallel, batched decode (4..32 rows on the general path): did the last request run the layer's all-reduce on the
     * side stream under the other micro-batch's launches (FTCF_DECODE_OVERLAP = 1, or chosen by the auto mode), and the auto
     * mode's two trials (ms per decode step, plain / overlapped, the slowest rank's; 0 until that trial has run) */
    int   decode_overlap;
    float decode_step_ms_plain, decode_step_ms_overlapped;
    /* decode_path 1: how the one- / two-row kernel ran its out-proj / FFN2 stage: 0 K pieces merged by an owner (two hops at the
     * layer boundary), 1 own-group layout (one hop; FTCF_PERSIST_OWN) */
    int   persist_layout;
    /* speculative decoding (appended): did the last request speculate, its verify passes, the draft tokens proposed to them and
     * the draft tokens accepted (decode_steps keeps counting generated tokens) */
    int   spec_active, spec_steps, spec_drafted, spec_accepted;
} ftcf_forward_stats;

int ftcf_gptneox_create(const ftcf_gptneox_config* cfg, const ftcf_gptneox_weights* w, ftcf_gptneox_t* out);
int ftcf_gptneox_forward(ftcf_gptneox_t h, const ftcf_forward_args* args);
/* The same request split in three so that a caller can stream or time the token loop:
 * forward(args) == begin(args) [buffers, runtime args, prefill] ; step(output_len) [token loop, stops early when every
 * row finished] ; finish() [gatherTree + outputs].  `args` pointers must stay valid until finish(). */
int ftcf_gptneox_begin(ftcf_gptneox_t h, const ftcf_forward_args* args);
int ftcf_gptneox_step(ftcf_gptneox_t h, int max_steps, int* steps_done);
int ftcf_gptneox_finish(ftcf_gptneox_t h);
/* Per-token log-probabilities of the hypotheses of the LAST request, which must have run with beam_width > 1 (the reference's
 * output_log_probs [batch, beam, output_len], GptNeoX.cc:418; ftcf_forward_args.output_log_probs stays refused for beams).
 * Every beam step records new cum_log_probs - the parent's old cum_log_probs (online_softmax_beamsearch_kernels.cu:241-243);
 * log_probs[b, k, i] is the recorded value of the cell the gather tree (decoding_kernels.cu:452-583) read the i-th generated
 * token of hypothesis (b, k) from -- output_ids[b, k, input_lengths[b] + i] -- and 0 where the tree takes no token from a cell:
 * the end_id fill past the longest beam and everything behind the hypothesis' first end token.  log_probs: device,
 * capacity >= batch * beam_width * output_len floats.  Valid after forward / finish until the next begin; runs on the engine's
 * stream and synchronises; changes nothing a later call would see.  FTCF_ERR_INVALID_ARG: no request has run, the last one
 * was not a beam request or has not finished, capacity too small, NULL. */
int ftcf_gptneox_beam_log_probs(ftcf_gptneox_t h, float* log_probs, size_t capacity);
int ftcf_gptneox_get_stats(ftcf_gptneox_t h, ftcf_forward_stats* stats);
/* enable HIP-event timing around every weight-streaming launch of the decode loop (bench.py roofline leg) */
int ftcf_gptneox_set_profiling(ftcf_gptneox_t h, int enabled);
/* Which requests with speculative_tokens > 0 may speculate (a switch of the engine, not a request field: ftcf_forward_args keeps
 * its layout).  0, the default: the bare greedy request, as before the switch existed -- the same tokens, bits and spec_active.
 * 1: also a request with stop words, return_cum_log_probs, output_log_probs, a streaming callback or optional_last_tokens (see
 * speculative_tokens of ftcf_forward_args).  At either scope every greedy verify pass closes with the two launches of
 * ftcf_verify_accept.  Holds for requests begun after the call.  Any other value: FTCF_ERR_INVALID_ARG. */
int ftcf_gptneox_set_speculative_scope(ftcf_gptneox_t h, int scope);
/* Whether a TOP-K SAMPLED request with speculative_tokens > 0 may speculate (a switch of the engine like the scope, and
 * independent of it).  0, the default: as before the switch existed -- the same launches, bits and spec_active.  1: top_k in
 * 2..64 no longer excludes a request, with any temperature (also together with log-probability outputs: the pass's tail applies
 * it) and with a top_p next to the top_k (the p of the top-k layer); every verify pass of such a request closes with the three
 * launches of ftcf_verify_sample on the engine's draw counter, so the tokens, sequence lengths and callback invocations are
 * those of the unspeculated request for the same random_seed.  What the scope decides (stop words, log-probabilities, callback,
 * optional_last_tokens) it still decides; pure top-p (top_k 0 with a top_p), top_k > 64, a vocabulary above 131072 and
 * everything speculative_tokens of ftcf_forward_args excludes besides stay excluded.  Greedy requests are not affected.  Holds for
 * requests begun after the call.  Any other value: FTCF_ERR_INVALID_ARG. */
int ftcf_gptneox_set_speculative_sampling(ftcf_gptneox_t h, int enabled);
int ftcf_gptneox_destroy(ftcf_gptneox_t h);


/* ---- continuous batching over a paged K/V cache (no counterpart in the reference, whose serving layer
 * triton_backend/gptneox/ allocates the cache per request, models/gptneox/GptNeoX.cc:84-156) --------------------------------
 * A batcher borrows an engine (which must outlive it and must not run a request of its own while a batcher call is in
 * progress).  K/V live in `num_pages` pages of `page_tokens` tokens shared by all sequences; up to `max_batch` sequences
 * decode together; waiting requests are admitted, in order, as soon as a slot and the pages for prompt + max_new_tokens are
 * free.  fp16 / int8 engines, parallel residual, any tensor_para_size (one batcher per rank, fed the same requests in the same
 * order); sampling: top_k / top_p / temperature / repetition penalty / stop words, and beam search (ftcf_batcher_submit_beam). */
typedef struct ftcf_batcher* ftcf_batcher_t;
int ftcf_batcher_create(ftcf_gptneox_t engine, int max_batch, int page_tokens, int num_pages, int max_seq_len,
                        ftcf_batcher_t* out);
/* The same with a PREFIX CACHE (prefix_cache = 1; 0 is ftcf_batcher_create): the pages that hold a finished admission's full
 * prompt blocks (page_tokens tokens each) stay cached, keyed by their tokens; a later request whose prompt starts with
 * cached blocks reuses their K/V -- at most floor((prompt_len - 1) / page_tokens) of them, the last prompt token is always
 * computed -- and its prompt phase computes only the rest.  Cached pages nobody uses are evicted, least recently used and
 * leaves first, only when an allocation cannot be served from the free list; ftcf_batcher_status's free_pages counts the
 * free list only.  Streams equal those of a cold admission up to fp16 rounding of the prompt phase (token exact unless a
 * near tie).  Requests admitted in the same batch do not share with each other (n samples of ONE prompt do, with or without
 * the cache: ftcf_batcher_submit_n); beam requests neither read nor populate
 * the cache.  Refused (an error, not a silent no-op) for tensor_para_size > 1, fp32 engines, sequential residual and
 * hidden sizes without the dual LayerNorm. */
int ftcf_batcher_create_ex(ftcf_gptneox_t engine, int max_batch, int page_tokens, int num_pages, int max_seq_len, int prefix_cache,
                           ftcf_batcher_t* out);
/* The general form.  struct_size must be sizeof(ftcf_batcher_options); max_batch .. prefix_cache as above.
 * OVERCOMMIT (overcommit = 1; 0 is exactly ftcf_batcher_create_ex): an ordinary request no longer reserves the pages of
 * prompt + max_new_tokens at admission.  It takes ceil((prompt_len + 1) / page_tokens) pages (less its prefix hit) and is
 * admitted when the pool has them plus one page per running ordinary request (waived when none runs); a running request takes
 * one page more each time its sequence crosses a page boundary, before the decode step.  When the pool cannot give that page
 * (cached prefix pages nobody uses are evicted first) the running ordinary request that arrived LAST is swapped out: its K/V
 * pages are copied to pinned host memory, bit for bit, its slot is freed.  Swapped-out requests resume, oldest first and before
 * anybody waiting is admitted, when a slot and their pages (plus the same watermark) are free -- in any slot, on fresh pages,
 * with their sampling state (draw counter, cumulative log-probability, history, logit processors, token mask) as it was: every
 * request still produces exactly the tokens it produces alone.  A resume produces no event.  A swapped-out request counts as
 * `waiting` in ftcf_batcher_status; ftcf_batcher_cancel (its host pages return) and ftcf_batcher_set_token_mask find it by id.
 * Beam requests keep reserving
 * their whole budget and are never swapped.  swap_pages: host pages of 2 * num_layer * page bytes (0: num_pages);
 * max_batch * ceil(max_seq_len / page_tokens) can never fill.  When no victim fits the free host pages ftcf_batcher_step
 * fails with -2 "swap space exhausted" before the step enqueues anything; the batcher stays consistent, cancel a
 * request and call again.  swap_stage_bytes: the device staging buffer the copies go through (0: 64 MiB).  It is
 * rounded to whole pages of all layers: at least one, and at most ceil(max_seq_len / page_tokens) -- one request's pages, more
 * is never in flight -- so a larger value allocates no more than that.  A request must still fit the pool alone at full
 * length.  Refused for tensor_para_size > 1. */
typedef struct {
    int    struct_size;
    int    max_batch, page_tokens, num_pages, max_seq_len;
    int    prefix_cache;
    int    overcommit;
    int    swap_pages;
    size_t swap_stage_bytes;
} ftcf_batcher_options;
int ftcf_batcher_create_opts(ftcf_gptneox_t engine, const ftcf_batcher_options* options, ftcf_batcher_t* out);
/* Overcommit counters (any pointer may be NULL): enabled, requests swapped out now, host pages in use and in all, then since
 * creation: preemptions, resumes, pages copied out and in.  Without overcommit: enabled = 0 and zeros. */
int ftcf_batcher_preempt_stats(ftcf_batcher_t b, int* enabled, int* swapped_requests, int* swap_pages_used, int* swap_pages_total,
                               long* preemptions, long* resumes, long* pages_out, long* pages_in);
/* Prefix-cache counters (any pointer may be NULL): enabled, cached pages, cached pages eviction could free now, admissions
 * looked up, their prompt tokens, the tokens served from the cache, the prompt tokens actually computed, pages evicted to make
 * room.  A batcher without the cache reports enabled = 0 and zeros. */
int ftcf_batcher_prefix_stats(ftcf_batcher_t b, int* enabled, int* cached_pages, int* evictable_pages, long* lookups,
                              long* prompt_tokens, long* hit_tokens, long* computed_tokens, long* evictions);
/* drops every cached page no request is using */
int ftcf_batcher_clear_prefix_cache(ftcf_batcher_t b);
/* prompt_ids: HOST array.  (top_k, top_p) = (0, 0) is greedy, as in the reference's sampling layer. */
int ftcf_batcher_submit(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k, float top_p,
                        float temperature, unsigned long long seed, long* request_id);
/* The same with the request's repetition penalty (sampling_penalty_kernels.cu:367-425: every token of prompt + output so
 * far, once) and stop words: `stop_words` is a HOST int array [2][stop_len] in the reference's to_word_list_format layout
 * (codefuse_example.py:26-53: row 0 the words' ids back to back, row 1 their cumulative end offsets, -1 padded), or NULL.
 * A request ends AFTER a stop sequence has been emitted (stop_criteria_kernels.cu:24-83): the event of its last token
 * carries finished = 1.  stop_len <= 64. */
int ftcf_batcher_submit_ex(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k, float top_p,
                           float temperature, float repetition_penalty, unsigned long long seed, const int* stop_words,
                           int stop_len, long* request_id);
/* The same with per-request LOGIT PROCESSORS (ftcf_logit_process above defines each of them and their order; they apply to
 * every token of the request, the first one included, before the sampling parameters do -- log_probs and top_logprobs of the
 * step calls are those of the processed distribution).  All arrays are HOST arrays, copied by the call.
 *   presence_penalty / frequency_penalty  over the request's generated tokens (finite);
 *   min_new_tokens                        the end token is held back for that many new tokens (>= 0);
 *   bias_ids / bias_values [n_bias]       the sparse logit bias, n_bias <= 1024, distinct ids in [0, V), values not NaN and not +inf;
 *   bad_words [2][bad_words_len]          banned words in the layout of stop_words, bad_words_len <= 256.
 * opts == NULL, or options that are all zero, is exactly ftcf_batcher_submit_ex.  struct_size must be
 * sizeof(ftcf_logit_options); anything outside the ranges above is FTCF_ERR_INVALID_ARG and nothing is queued.  Beam requests
 * take no options. */
typedef struct {
    int          struct_size;
    float        presence_penalty;
    float        frequency_penalty;
    int          min_new_tokens;
    const int*   bias_ids;
    const float* bias_values;
    int          n_bias;
    const int*   bad_words;
    int          bad_words_len;
} ftcf_logit_options;
int ftcf_batcher_submit_opts(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k, float top_p,
                             float temperature, float repetition_penalty, unsigned long long seed, const int* stop_words,
                             int stop_len, const ftcf_logit_options* opts, long* request_id);
/* The ALLOWED-TOKEN MASK of a waiting or running request (the hook of grammar-constrained decoding): allowed_bits is a HOST
 * array of n_words = ceil(V / 32) words, bit t set: token t may be sampled.  It applies to every token sampled for the request
 * from the next one on -- set on a waiting request it governs the first token -- until it is replaced; allowed_bits == NULL
 * clears it.  May be called from inside the token callback.  A mask is copied to the device before the next step only when it
 * changed.  A mask without a bit in [0, V), a wrong n_words, an unknown or finished request and a beam request are
 * FTCF_ERR_INVALID_ARG.  A request whose options and mask leave no token ends with end_id. */
int ftcf_batcher_set_token_mask(ftcf_batcher_t b, long request_id, const unsigned* allowed_bits, int n_words);
/* n SAMPLES OF ONE PROMPT (OpenAI's `n`, self-consistency, pass@k): the arguments of ftcf_batcher_submit_opts (opts may be NULL)
 * queue ONE fork request and return n_samples consecutive ids in request_ids [n_samples].  Sibling i is the request a plain
 * submission of the same prompt and options with seed + i (mod 2^64) would be -- its draw counter starts at 0, draw 0 gives its
 * first token -- and produces exactly the tokens that submission produces alone; greedy siblings are identical streams.  The
 * prompt runs through the model ONCE (one prompt phase of one row, from the hit offset with the prefix cache on); its
 * floor(prompt_len / page_tokens) full pages are held once and shared by all siblings, each sibling owns the rest of what the
 * plain request holds (reservation: up to full length; overcommit: one page), the first of which receives the prompt's
 * prompt_len % page_tokens last rows.  The request is admitted alone, into any n_samples free slots; with sequences running, a
 * long prompt is prefilled in chunks as a single request's is.  From the admission on a sibling is an ordinary request in every
 * respect: own events and callback calls (the admission reports n_samples events in sibling order), cancel, token mask, stop
 * words, logit processors, log-probabilities, swap-out and resume.  While the request waits the ids are valid already:
 * ftcf_batcher_cancel of one shrinks the fork (the last one removes it), ftcf_batcher_set_token_mask sets that sibling's own mask,
 * which governs its first token.  n_samples == 1 is exactly ftcf_batcher_submit_opts.  FTCF_ERR_INVALID_ARG, nothing queued:
 * n_samples < 1 or > max_batch, or a fork that cannot fit the pool alone -- shared + n_samples * own pages at full length
 * (overcommit: its admission's pages and watermark, shared + 2 n_samples - 1, and one sibling at full length). */
int ftcf_batcher_submit_n(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k, float top_p,
                          float temperature, float repetition_penalty, unsigned long long seed, const int* stop_words, int stop_len,
                          const ftcf_logit_options* opts, int n_samples, long* request_ids);
/* Fork counters since creation (any pointer may be NULL): fork admissions, the siblings they opened, the page allocations
 * sharing saved (n_samples - 1 per shared page) and the prompt tokens their prompt phases computed (one prompt's, less its hit). */
int ftcf_batcher_fork_stats(ftcf_batcher_t b, long* requests, long* siblings, long* shared_pages, long* prompt_tokens_computed);
/* A beam-search request (GptNeoXOp.forward with beam_width > 1: OnlineBeamSearchLayer semantics, the engine's own beam kernels):
 * it occupies `beam_width` consecutive slots, its beams share the prompt's pages and every page they have in common (copy on
 * write).  ftcf_batcher_step reports ONE event for it, when it has finished: token = -1, finished = 1; the hypotheses are
 * then fetched ONCE with ftcf_batcher_beam_result: output_ids [beam_width][total_len] (prompt, then the beam's tokens, end_id
 * padded: total_len = prompt_len + max_new_tokens), sequence_lengths [beam_width], cum_log_probs [beam_width] -- the arrays
 * GptNeoXOp.forward returns.  output_ids == NULL: only *beam_width / *total_len are set (0 / 0: unknown id or still running).
 * 2 <= beam_width <= min(64, max_batch).  Up to 256 finished results wait to be fetched (the oldest are dropped beyond
 * that); ftcf_batcher_cancel of a finished request drops its result. */
int ftcf_batcher_submit_beam(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int beam_width,
                             float beam_search_diversity_rate, float len_penalty, float temperature, float repetition_penalty,
                             long* request_id);
/* The same with min_length (the end token is held back for that many new tokens: beam_search_penalty_kernels.cu:155-169; 0 = none)
 * and stop words in the layout of ftcf_batcher_submit_ex (checked along a beam's parent chain: a beam that has emitted a stop
 * sequence is finished). */
int ftcf_batcher_submit_beam_ex(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int beam_width,
                                float beam_search_diversity_rate, float len_penalty, float temperature, float repetition_penalty,
                                int min_length, const int* stop_words, int stop_len, long* request_id);
int ftcf_batcher_beam_result(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths, float* cum_log_probs,
                             int capacity, int* beam_width, int* total_len);
/* The general form of a beam request.  struct_size must be sizeof(ftcf_beam_options) (anything else is FTCF_ERR_INVALID_ARG
 * and nothing is queued); beam_width .. stop_len as in ftcf_batcher_submit_beam_ex.  token_log_probs != 0: the request also
 * returns the log-probability of every generated token of every hypothesis (ftcf_gptneox_beam_log_probs: the step's new
 * cumulative score minus the parent's old one, online_softmax_beamsearch_kernels.cu:241-243, carried along the gather tree's
 * parent chain), fetched with ftcf_batcher_beam_result_ex.  With token_log_probs == 0 it is exactly ftcf_batcher_submit_beam_ex. */
typedef struct {
    int        struct_size;
    int        beam_width;
    float      beam_search_diversity_rate, len_penalty, temperature, repetition_penalty;
    int        min_length;
    const int* stop_words;
    int        stop_len;
    int        token_log_probs;
} ftcf_beam_options;
int ftcf_batcher_submit_beam_opts(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens,
                                  const ftcf_beam_options* options, long* request_id);
/* ftcf_batcher_beam_result plus token_log_probs [beam_width][max_new_tokens] (entry i: the i-th generated token, 0 behind the
 * hypothesis' first end token and in the end_id padding).  NULL is allowed (then it is ftcf_batcher_beam_result); non-NULL for
 * a request that was not submitted with token_log_probs is FTCF_ERR_INVALID_ARG and the result stays parked. */
int ftcf_batcher_beam_result_ex(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths, float* cum_log_probs,
                                float* token_log_probs, int capacity, int* beam_width, int* total_len);
/* One scheduler iteration: one decode step for the running sequences, then admissions (prefill + first token).  Returns one
 * event per token produced: request id, token, finished (end_id emitted or max_new_tokens reached).  capacity >= 2 * max_batch.
 * With sequences running, a prompt longer than FTCF_BATCHER_PREFILL_CHUNK tokens (default 512; 0 = never) is admitted alone and
 * prefilled in chunks of that many tokens, with one decode step of the running sequences after every chunk but the last: the
 * iteration then produces several tokens per running sequence.  Events that do not fit `capacity` are returned by the next
 * calls, before a new iteration runs (`running` of ftcf_batcher_status counts 1 for them). */
int ftcf_batcher_step(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, int capacity, int* n_events);
/* The same with each event's log-probability: log_probs[i] is the event token's log-probability as output_log_probs of
 * ftcf_forward_args defines it (the value the step adds to the request's cumulative log-probability), NaN for a beam request's
 * token = -1 event.  An admission inside this call scores its first token too (the engine's prompt phase then runs the soft-max
 * statistics, as every decode step of the batcher does); events of admissions made by ftcf_batcher_step and fetched here carry
 * NaN.  log_probs holds `capacity` floats. */
int ftcf_batcher_step_ex(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int capacity,
                         int* n_events);
/* The same with each event's top_n (1..20) alternatives: top_ids / top_log_probs hold capacity * top_n entries, event i's pairs at
 * [i * top_n, (i + 1) * top_n), as top_logprobs of ftcf_forward_args defines them (the distribution the event's token was drawn
 * from).  Per call, like log_probs: an admission inside this call reports the pairs of its first token; a beam request's event
 * and events of admissions made by another step call carry (-1, NaN) pairs.  log_probs may be NULL. */
int ftcf_batcher_step_top(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int top_n, int* top_ids,
                          float* top_log_probs, int capacity, int* n_events);
/* Streaming (the reference's token callback, GptNeoX.cc:362-375, 1023 `token_generated_cb_`, per request here): `fn` is called
 * from inside ftcf_batcher_step, on the calling thread, for every event the moment its token is on the host -- i.e. between
 * the chunks of a long admission as well -- and the same events are returned by the step call afterwards.  NULL unsets. */
typedef void (*ftcf_token_callback_fn)(void* user, long request_id, int token, int finished);
int ftcf_batcher_set_token_callback(ftcf_batcher_t b, ftcf_token_callback_fn fn, void* user);
int ftcf_batcher_status(ftcf_batcher_t b, int* waiting, int* running, int* free_pages);
/* drop a waiting or running request (its pages return to the pool at once); *found = 0 when the id is unknown or already done */
int ftcf_batcher_cancel(ftcf_batcher_t b, long request_id, int* found);
int ftcf_batcher_destroy(ftcf_batcher_t b);

#ifdef __cplusplus
}
#endif
#endif /* FTCF_H */
