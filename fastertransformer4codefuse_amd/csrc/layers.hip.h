// Host-side layer units of the GPT-NeoX decode path: what the reference's layer classes do, as sequences of this library's
// HIP launches on a caller-given stream.  No layer owns memory (the reference's allocateBuffer / freeBuffer per call,
// DecoderSelfAttentionLayer.cc:148-187, FfnLayer.cc:455-530, are the engine's one arena: engine.hip plan()), no layer
// synchronises, and none calls a collective itself: a parallel-residual layer reduces x' ONCE, after the residual
// (GptNeoXDecoder.cc:342-359), which is the decoder's business -- the two walks are handed the all-reduce by their caller.
//
//   DecoderSelfAttentionLayer  <- layers/attention_layers/DecoderSelfAttentionLayer.cc:459-686 (+ TensorParallel wrapper :190-226)
//   GptContextAttentionLayer   <- layers/attention_layers/GptContextAttentionLayer.cc:25-403
//   FfnLayer (GeluFfnLayer)    <- layers/FfnLayer.cc:34-380, TensorParallelGeluFfnLayer.cc:33-63
//   ParallelResidualDecoder    <- models/gptneox/GptNeoXDecoder.cc:245-384 (use_gptj_residual), the batched decode rows
//   ParallelResidualContextDecoder <- models/gptneox/GptNeoXContextDecoder.cc:283-507 (use_gptj_residual), the prompt rows
//   DynamicDecodeLayer         <- layers/DynamicDecodeLayer.cc:192-497 (sampling layers, online beam search)
//
// ParallelResidualDecoder is the ONE walk over the layers of a batched decode step: the engine's general path and its overlapped
// form, the speculative verify pass and the continuous batcher (plain and overlapped) run it with their own attention launch,
// buffers and GEMM binding.  ParallelResidualContextDecoder is the ONE walk over the layers of the prompt phase: the whole batch,
// the token ranges of a chunked admission or of a prefix hit's tail, and the two micro-batches of the overlapped form are spans
// (PromptSpan) of the same per-layer body.  The fused forms -- the persistent decode kernel (persist_device.hip.h), the rows
// kernel, the per-stage GEMV launches -- cut ACROSS these units on purpose and stay in engine.hip; so do the sequential-residual
// loops and the fp32 instantiation.
#pragma once
#include <functional>
#include <vector>

#include "kernels.h"

namespace ftcf {

struct DenseWeight {  // layers/DenseWeight.h:29-66
    const void* kernel = nullptr;  // tiled (int8 or fp16)
    const f16*  scale  = nullptr;  // weight_only_quant_scale
    const f16*  bias   = nullptr;
};
struct LayerWeights {  // models/gptneox/GptNeoXDecoderLayerWeight.h
    const f16 *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    DenseWeight qkv, attn_out, ffn1, ffn2;
};
// the layers as the persistent / rows kernels read them; layer l's K/V at k_base / v_base + l * layer_stride
inline std::vector<PersistLayer> persist_layer_table(const std::vector<LayerWeights>& layers, f16* k_base, f16* v_base,
                                                     size_t layer_stride)
{
    std::vector<PersistLayer> pl(layers.size());
    for (size_t l = 0; l < layers.size(); l++) {
        const LayerWeights& w = layers[l];
        PersistLayer&       r = pl[l];
        r.ln1_g = w.ln1_g;
        r.ln1_b = w.ln1_b;
        r.ln2_g = w.ln2_g;
        r.ln2_b = w.ln2_b;
        r.w_qkv = w.qkv.kernel;
        r.w_ffn1 = w.ffn1.kernel;
        r.w_out = w.attn_out.kernel;
        r.w_ffn2 = w.ffn2.kernel;
        r.s_qkv = w.qkv.scale;
        r.s_ffn1 = w.ffn1.scale;
        r.s_out = w.attn_out.scale;
        r.s_ffn2 = w.ffn2.scale;
        r.b_qkv = w.qkv.bias;
        r.b_ffn1 = w.ffn1.bias;
        r.b_res = w.ffn2.bias;
        r.k_cache = k_base + l * layer_stride;
        r.v_cache = v_base + l * layer_stride;
    }
    return pl;
}

// C[m, n] = epilogue(A[m, k] x W) on stream s; `slot` names the workspace region of the burst GEMM this call may use
// (0 QKV, 1 FFN1, 2 out-proj, 3 FFN2: the four GEMMs of a layer may be in flight together on two streams).  The engine
// and the batcher bind it to their dispatch (GEMV / burst / tiled MFMA kernels by row count).
using GemmFn = std::function<void(const f16* A, const DenseWeight& w, const f16* bias, int act, f16* C, int m, int n, int k,
                                  hipStream_t s, int slot)>;

struct DecoderSelfAttentionLayer {
    GemmFn gemm;
    int    H = 0, hl = 0;  // hidden size, local hidden size (heads of this rank x size_per_head)
    // in [m, H] (LayerNorm'd) -> qkv_buf [m, 3 hl] -> masked multi-head attention over the K/V cache (appends this step's
    // key / value; qkv bias and NeoX rotary inside the kernel like the reference's) -> ctx [m, hl] -> out [m, H] (no bias:
    // it rides on the residual kernel).  attention(): the caller's launch over its K/V cache -- contiguous, paged, the verify pass's
    template<typename Attention>
    void forward(const f16* in, f16* qkv_buf, const f16* ctx_buf, f16* out, const LayerWeights& w, Attention&& attention, int m,
                 hipStream_t s) const
    {
        gemm(in, w.qkv, nullptr, 0, qkv_buf, m, 3 * hl, H, s, 0);
        attention();
        gemm(ctx_buf, w.attn_out, nullptr, 0, out, m, H, hl, s, 2);
    }
};

struct GptContextAttentionLayer {
    GemmFn gemm;
    int    H = 0, hl = 0, nh = 0, dh = 0, rot = 0;
    // rows = sequences x tokens of (a micro-batch of) the prompt: QKV GEMM, bias + rotary + K/V -> cache, causal attention on
    // MFMA tiles (the reference's UNFUSED_MHA with padding removal), output projection.  [s_lo, s_hi): the token range of a
    // chunked prompt phase whose earlier tokens' K/V are in the cache already (default: the whole prompt)
    void forward(const f16* in, f16* qkv_buf, f16* ctx_buf, f16* out, const LayerWeights& w, const int* input_lengths, f16* k_cache,
                 f16* v_cache, int B, int S, int s_max, int cache_row_mult, hipStream_t s, int s_lo = 0, int s_hi = -1) const
    {
        const int    e   = s_hi < 0 ? S : s_hi;
        const size_t r0  = (B == 1) ? (size_t)s_lo : 0;  // (a token range is only cut out of a single sequence)
        const int    m   = (B == 1) ? e - s_lo : B * S;
        gemm(in + r0 * H, w.qkv, nullptr, 0, qkv_buf + r0 * 3 * hl, m, 3 * hl, H, s, 0);
        launch_context_attention(qkv_buf, w.qkv.bias, input_lengths, k_cache, v_cache, B, S, nh, dh, rot, s_max, ctx_buf, s,
                                 cache_row_mult, s_lo, e);
        gemm(ctx_buf + r0 * hl, w.attn_out, nullptr, 0, out + r0 * H, m, H, hl, s, 2);
    }
};

struct FfnLayer {
    GemmFn gemm;
    int    H = 0, il = 0;  // hidden size, local intermediate size
    // out = gelu_tanh(in W1 + b1) W2 ; bias 2 is deferred to the residual kernel (FfnLayer.cc:203-217 gemm_bias_act)
    void forward(const f16* in, f16* mid_buf, f16* out, const LayerWeights& w, int m, hipStream_t s) const
    {
        gemm(in, w.ffn1, w.ffn1.bias, 1, mid_buf, m, il, H, s, 1);
        gemm(mid_buf, w.ffn2, nullptr, 0, out, m, H, il, s, 3);
    }
};

// How a batched decode layer's four GEMMs are launched (the caller decides by its own eligibility rules):
//   branches: [QKV -> attention -> out-proj] on `stream`, [FFN1 -> FFN2] on `side`, one burst launch per GEMM per 16 rows
//   grouped:  independent GEMMs share a launch, [QKV, FFN1] -> attention -> [out-proj, FFN2] (<= 16 rows)
//   plain:    the caller's row-count dispatch, one GEMM after the other
enum class DecodeGemms { branches, grouped, plain };

struct Untimed {  // (the timing hook of a caller that keeps no profiling records)
    template<typename F>
    void operator()(double, F&& f, hipStream_t) const
    {
        f();
    }
};

// The layers of one batched decode step of a parallel-residual model (GptNeoXDecoder.cc:245-384): per layer the entry LayerNorms
// (one dual-LN pass over x), [QKV, FFN1], attention, [out-proj, FFN2] and the closing residual -- fused into the next layer's
// LayerNorm pass where no all-reduce of x' stands in between.  The callers pass
//   attention(l, w, r0, M, s):       their attention launch for rows [r0, r0 + M) of layer l on stream s
//   allreduce(buf, count, s, scaled): the layer's all-reduce (scaled: the kernel that reads the sum applies fake_mul itself)
//   timed(bytes, launch, s):          their profiling bracket around a burst GEMM launch
struct ParallelResidualDecoder {
    const LayerWeights* layers = nullptr;
    int                 L = 0, H = 0, hl = 0, il = 0;
    bool                int8 = false;
    int                 tp = 1, fake_mul = 1;  // tensor-parallel size, fake-peer multiplier of the summed attn | ffn
    // tp > 1: attn | ffn all-reduced as ONE message and the residual inside the next layer's LayerNorm pass, as at tp = 1: two
    // launches where the reference's residual -> all-reduce -> LayerNorms (GptNeoXDecoder.cc:342-359) are three
    bool                pair_ar = false;
    // the buffer view, row-major: x [rows, H], nrm / nrm2 [rows, H], qkv [rows, 3 hl], ctx [rows, hl], att / ffn [rows, H], mid [rows, il]
    f16 *x = nullptr, *nrm = nullptr, *nrm2 = nullptr, *qkv = nullptr, *ctx = nullptr, *att = nullptr, *ffn = nullptr, *mid = nullptr;
    // the burst GEMM's workspace ([partial bytes of split-K sums][tickets]), device step pointer and host launch counter (its
    // granule tags); region: the bytes one micro-batch's GEMMs use
    float*          ws = nullptr;
    size_t          partial = 0, region = 0;
    const int*      d_step = nullptr;
    unsigned*       seq = nullptr;
    GemmFn          plain;  // DecodeGemms::plain
    hipStream_t     stream = nullptr, side = nullptr, side2 = nullptr;  // side: FFN branch / the reductions; side2: second micro-batch
    hipEvent_t      ev_fork = nullptr, ev_join = nullptr;
    const hipEvent_t *dv_fork = nullptr, *dv_done = nullptr, *dv_red = nullptr;  // [2] each, forward_overlapped

    bool pair() const { return tp > 1 && pair_ar && residual_dual_ln_supported(H); }

    // the whole batch on `stream`
    template<typename Attention, typename AllReduce, typename Timed = Untimed>
    void forward(int B, DecodeGemms gemms, Attention&& attention, AllReduce&& allreduce, Timed&& timed = Timed{}) const
    {
        FTCF_CHECK_ARG(!pair() || ffn == att + (size_t)B * H, "the pair all-reduce needs ffn directly behind att");
        DecoderSelfAttentionLayer attn_u{plain, H, hl};
        FfnLayer                  ffn_u{plain, H, il};
        if (gemms == DecodeGemms::branches) {
            // The attention branch [QKV -> MMHA -> out-proj] (78.6 + K/V + 26.2 MB at 13B int8) and the FFN branch
            // [FFN1 -> FFN2] (2 x 104.9 MB) of a parallel-residual layer are independent: two streams.  Every one
            // of these launches is a short burst -- the whole matrix requested at once, gone in ~30 us -- whose
            // ramp-up and drain leave the HBM idle; the other branch's launch fills those gaps.  The same two layer units,
            // their GEMMs bound to the burst kernel with one workspace region per GEMM of the layer.
            const int    bc      = std::min(B, 16);
            const size_t o_f1    = gemm_smallm_workspace_bytes(bc, 3 * hl, H, int8);
            const size_t o_out   = o_f1 + gemm_smallm_workspace_bytes(bc, il, H, int8);
            const size_t offs[4] = {0, o_f1, o_out, o_out + gemm_smallm_workspace_bytes(bc, H, hl, int8)};
            const double wbytes  = int8 ? 1.0 : 2.0;
            attn_u.gemm = [this, &timed, wbytes, offs](const f16* A, const DenseWeight& dw, const f16* bias, int act, f16* C, int m,
                                                       int n, int k, hipStream_t s, int slot) {
                // (one launch that keeps the weights in registers and passes the rows 16 at a time through the x tile
                // was measured: 256 VGPRs, one workgroup per CU -- 8.2 / 8.3 / 13.0 ms at 24 / 32 / 64 rows, i.e.
                // slower than re-reading the weights per 16 rows except at 64)
                for (int r0 = 0; r0 < m; r0 += 16) {  // 16 rows per launch (launches of one GEMM are in stream order)
                    const SmallmDesc d{A + (size_t)r0 * k, dw.kernel, dw.scale, bias, act, C + (size_t)r0 * n, n, k};
                    timed(wbytes * (double)n * k, [&] {
                        launch_gemm_smallm_group(&d, 1, ws, partial, std::min(16, m - r0), int8, s, d_step, seq, offs[slot]);
                    }, s);
                }
            };
            ffn_u.gemm = attn_u.gemm;
        }
        for (int l = 0; l < L; l++) {
            layer(l, 0, B, att, ffn, stream, 0, gemms, attn_u, ffn_u, attention,
                  [&](f16* buf, size_t count, bool scaled) { allreduce(buf, count, stream, scaled); }, timed);
        }
    }

    // Two micro-batches, rows [0, (B + 1) / 2) on `stream` and the rest on `side2`, independent of each other from the first layer
    // to the last; their reductions on `side` in the order c = 0, 1, 0, 1, ...: micro-batch c hands its sum over by event and waits
    // for the reduced rows by event, so c's reduction runs under (1 - c)'s launches.  Grouped GEMMs, each micro-batch with its own
    // split-K region.  Needs tp > 1 and the dual LayerNorm kernel (H % 8 == 0, H <= 8192).
    template<typename Attention, typename AllReduce, typename Timed = Untimed>
    void forward_overlapped(int B, Attention&& attention, AllReduce&& allreduce, Timed&& timed = Timed{}) const
    {
        // (a micro-batch's attn | ffn rows are adjacent: [2 r0 H, 2 r0 H + M H) and the M H behind it)
        FTCF_CHECK_ARG(ffn == att + (size_t)B * H, "the micro-batches' attn | ffn need ffn directly behind att");
        const int                       r0[2] = {0, (B + 1) / 2}, r1[2] = {(B + 1) / 2, B};
        const hipStream_t               cs[2] = {stream, side2};
        const bool                      pr = pair();
        const DecoderSelfAttentionLayer no_attn{};
        const FfnLayer                  no_ffn{};
        // what is on `stream` so far (embedding rows, the step's state) happens-before both micro-batches
        FTCF_HIP_CHECK(hipEventRecord(dv_fork[0], stream));
        FTCF_HIP_CHECK(hipStreamWaitEvent(side2, dv_fork[0], 0));
        for (int l = 0; l < L; l++) {
            for (int c = 0; c < 2; c++) {
                const int         M  = r1[c] - r0[c];
                const hipStream_t st = cs[c];
                if (l > 0 && !pr) {
                    FTCF_HIP_CHECK(hipStreamWaitEvent(st, dv_red[c], 0));  // this micro-batch's x has been reduced
                }
                f16* const attc = att + 2 * (size_t)r0[c] * H;
                layer(l, r0[c], M, attc, attc + (size_t)M * H, st, (size_t)c * region, DecodeGemms::grouped, no_attn, no_ffn, attention,
                      [&](f16* buf, size_t count, bool scaled) {
                          FTCF_HIP_CHECK(hipEventRecord(dv_done[c], st));
                          FTCF_HIP_CHECK(hipStreamWaitEvent(side, dv_done[c], 0));
                          allreduce(buf, count, side, scaled);
                          FTCF_HIP_CHECK(hipEventRecord(dv_red[c], side));
                          if (pr) {  // the layer's residual inside the next layer's LayerNorm pass, behind the reduction
                              FTCF_HIP_CHECK(hipStreamWaitEvent(st, dv_red[c], 0));
                          }
                      },
                      timed);
            }
        }
        // join: both micro-batches' last reductions, and the second compute stream itself (its last wait is for dv_red[1] of layer
        // L - 2: nothing of it is left running behind dv_red[1] of the last layer, but a capture wants every fork joined)
        FTCF_HIP_CHECK(hipEventRecord(dv_fork[1], side2));
        FTCF_HIP_CHECK(hipStreamWaitEvent(stream, dv_fork[1], 0));
        for (int c = 0; c < 2; c++) {
            FTCF_HIP_CHECK(hipStreamWaitEvent(stream, dv_red[c], 0));
        }
    }

private:
    // layer l for rows [r0, r0 + M) on stream s; attc / ffnc: where these rows' attention and FFN outputs go; reduce(buf, count,
    // scaled): the layer's all-reduce as the walk mode orders it
    template<typename Attention, typename Reduce, typename Timed>
    void layer(int l, int r0, int M, f16* attc, f16* ffnc, hipStream_t s, size_t region_off, DecodeGemms gemms,
               const DecoderSelfAttentionLayer& attn_u, const FfnLayer& ffn_u, Attention& attention, Reduce&& reduce, Timed& timed) const
    {
        const LayerWeights& w  = layers[l];
        const LayerWeights* nx = l + 1 < L ? &layers[l + 1] : nullptr;
        // layer_input/output alias for 0 < l < L-1 in the reference (:249-250) -> which residual form it runs
        const int    inplace = (l > 0 && l < L - 1) ? 1 : 0;
        const bool   dual = residual_dual_ln_supported(H), tp1 = tp == 1, pr = pair();
        const size_t o  = (size_t)r0;
        f16 *const   xr = x + o * H, *const n1 = nrm + o * H, *const n2 = nrm2 + o * H, *const q = qkv + o * 3 * hl,
                     *const cx = ctx + o * hl, *const md = mid + o * il;
        // both LayerNorms of the layer come from one pass over x, fused with the previous layer's residual when there is no
        // collective in between
        if (!dual) {
            launch_layernorm(xr, w.ln1_g, w.ln1_b, n1, M, H, 1e-5f, true, s);
            launch_layernorm(xr, w.ln2_g, w.ln2_b, n2, M, H, 1e-5f, true, s);
        }
        else if (l == 0 || (!tp1 && !pr)) {
            launch_residual_dual_ln(xr, nullptr, nullptr, nullptr, 1, 0, w.ln1_g, w.ln1_b, w.ln2_g, w.ln2_b, n1, n2, M, H, 1e-5f, s);
        }
        if (gemms == DecodeGemms::grouped) {
            // independent GEMMs share a launch (a dependent launch costs ~8 us of dispatch latency, most of a layer
            // at tensor-parallel shard sizes): [QKV, FFN1] -> attention -> [out-proj, FFN2]
            const double     wbytes = int8 ? 1.0 : 2.0;
            const SmallmDesc p1[2]  = {{n1, w.qkv.kernel, w.qkv.scale, nullptr, 0, q, 3 * hl, H},
                                       {n2, w.ffn1.kernel, w.ffn1.scale, w.ffn1.bias, 1, md, il, H}};
            timed(wbytes * H * (3.0 * hl + il), [&] { launch_gemm_smallm_group(p1, 2, ws, partial, M, int8, s, d_step, seq, region_off); }, s);
            attention(l, w, r0, M, s);
            const SmallmDesc p3[2] = {{cx, w.attn_out.kernel, w.attn_out.scale, nullptr, 0, attc, H, hl},
                                      {md, w.ffn2.kernel, w.ffn2.scale, nullptr, 0, ffnc, H, il}};
            timed(wbytes * H * ((double)hl + il), [&] { launch_gemm_smallm_group(p3, 2, ws, partial, M, int8, s, d_step, seq, region_off); }, s);
        }
        else {
            const bool fork = gemms == DecodeGemms::branches;
            if (fork) {
                FTCF_HIP_CHECK(hipEventRecord(ev_fork, s));
                FTCF_HIP_CHECK(hipStreamWaitEvent(side, ev_fork, 0));
            }
            attn_u.forward(n1, q, cx, attc, w, [&] { attention(l, w, r0, M, s); }, M, s);
            ffn_u.forward(n2, md, ffnc, w, M, fork ? side : s);
            if (fork) {
                FTCF_HIP_CHECK(hipEventRecord(ev_join, side));
                FTCF_HIP_CHECK(hipStreamWaitEvent(s, ev_join, 0));
            }
        }
        if (pr) {
            // attn | ffn travel as one message of twice the size and the residual -- x + attn + ffn + TP x (bias / TP) in fp32,
            // rounded once -- runs inside the next layer's LayerNorm pass (add_residual_kernels.cu:116-152 is the reference's)
            reduce(attc, (size_t)2 * M * H, true);
            launch_residual_dual_ln(xr, ffnc, attc, w.ffn2.bias, 1, 1, nx ? nx->ln1_g : nullptr, nx ? nx->ln1_b : nullptr,
                                    nx ? nx->ln2_g : nullptr, nx ? nx->ln2_b : nullptr, n1, n2, M, H, 1e-5f, s, tp, fake_mul);
        }
        else if (dual && tp1) {
            launch_residual_dual_ln(xr, ffnc, attc, w.ffn2.bias, 1, inplace, nx ? nx->ln1_g : nullptr, nx ? nx->ln1_b : nullptr,
                                    nx ? nx->ln2_g : nullptr, nx ? nx->ln2_b : nullptr, n1, n2, M, H, 1e-5f, s);
        }
        else {
            launch_add_bias_attn_ffn_residual(xr, ffnc, attc, xr, w.ffn2.bias, M, H, tp, inplace, true, s);
            if (!tp1) {
                reduce(xr, (size_t)M * H, false);
            }
        }
    }
};

// The rows of the prompt buffers one call of the prompt-phase walk works on: whole sequences [b0, b1) of the batch, or tokens
// [s0, s1) of the ONE sequence of a batch of one (the earlier tokens' K/V are in the cache: a chunk, a prefix hit's tail, a half)
struct PromptSpan {
    int  b0 = 0, b1 = 0, s0 = 0, s1 = 0;
    bool tokens = false;
    static PromptSpan sequences(int b0, int b1) { return {b0, b1, 0, 0, false}; }
    static PromptSpan token_range(int s0, int s1) { return {0, 1, s0, s1, true}; }
};

// The layers of the prompt phase of a parallel-residual model (GptNeoXContextDecoder.cc:283-507) over the prompt buffers
// [B * S, .] and a K/V cache of B * tile rows per layer (beam search: tile = beam_width, sequence b's K/V in cache row b * tile):
// per layer the entry LayerNorms (one dual-LN pass over x), the context attention layer, the FFN and the closing residual -- fused
// into the next layer's LayerNorm pass where no all-reduce of x' stands in between, the same rule for every span.  The callers pass
//   allreduce(buf, count, s): the layer's all-reduce of x' on stream s
struct ParallelResidualContextDecoder {
    const LayerWeights* layers = nullptr;
    int                 L = 0, H = 0, hl = 0, il = 0, tp = 1;
    // the prompt buffers, row-major: px / pnrm / pnrm2 / patt / pffn [B * S, H], pqkv [B * S, 3 hl], pctx [B * S, hl], pmid [B * S, il]
    f16 *px = nullptr, *pnrm = nullptr, *pnrm2 = nullptr, *pqkv = nullptr, *pctx = nullptr, *patt = nullptr, *pmid = nullptr, *pffn = nullptr;
    f16 *                    k_cache = nullptr, *v_cache = nullptr;  // layer l's K/V at + l * layer_stride
    size_t                   layer_stride = 0;                       // B * tile * heads of this rank * s_max * size_per_head
    const int*               input_lengths = nullptr;
    int                      B = 0, S = 0, s_max = 0, tile = 1;
    GptContextAttentionLayer attention;
    FfnLayer                 ffn;
    hipStream_t              stream = nullptr, side = nullptr;      // side: the reductions of forward_overlapped
    const hipEvent_t *       ov_done = nullptr, *ov_red = nullptr;  // [2] each, forward_overlapped

    // all layers for one span on `stream`.  A token span [s0, s1) with s0 > 0 is a piece of a chunked prompt phase or the tail
    // behind a prefix whose K/V the caller has put into the cache: every GEMM / LayerNorm / residual is row wise and the span's
    // attention reads the earlier tokens' K/V from the cache, so the arithmetic per row is that of the whole prompt; the split-K
    // form of the GEMMs depends on the row count, so the pieces agree with the whole to fp16 rounding of the GEMM outputs, not bit
    // for bit.
    template<typename AllReduce>
    void forward(const PromptSpan& span, AllReduce&& allreduce) const
    {
        check(span);
        for (int l = 0; l < L; l++) {
            layer(l, span, stream, [&](f16* buf, size_t count) { allreduce(buf, count, stream); });
        }
    }

    // Two micro-batches under tensor parallelism with the per-layer all-reduce OVERLAPPED (GptNeoXContextDecoder.cc:462-465 calls
    // ftNcclAllReduceSum on the compute stream, nothing runs under it): whole sequences when there are several (their attention is
    // independent), the first and the second part of the tokens of a single sequence (the second part's attention reads the first
    // part's K/V from the cache, where the first part's attention call has put them).  A layer runs micro-batch 0, then 1, on
    // `stream`; each micro-batch's all-reduce goes to `side` behind an event, and the NEXT layer's work on that micro-batch waits
    // for it: the reduction of one runs under the GEMMs of the other.  Same arithmetic per row as forward() of the whole batch (the
    // all-reduce sums the same values): bit-identical to it as long as the GEMMs take the same form.  Needs tp > 1.
    template<typename AllReduce>
    void forward_overlapped(const PromptSpan& span0, const PromptSpan& span1, AllReduce&& allreduce) const
    {
        const PromptSpan span[2] = {span0, span1};
        check(span0);
        check(span1);
        for (int l = 0; l < L; l++) {
            for (int c = 0; c < 2; c++) {
                if (l > 0) {
                    FTCF_HIP_CHECK(hipStreamWaitEvent(stream, ov_red[c], 0));  // this micro-batch's x has been reduced
                }
                layer(l, span[c], stream, [&](f16* buf, size_t count) {
                    FTCF_HIP_CHECK(hipEventRecord(ov_done[c], stream));
                    FTCF_HIP_CHECK(hipStreamWaitEvent(side, ov_done[c], 0));
                    allreduce(buf, count, side);
                    FTCF_HIP_CHECK(hipEventRecord(ov_red[c], side));
                });
            }
        }
        for (int c = 0; c < 2; c++) {
            FTCF_HIP_CHECK(hipStreamWaitEvent(stream, ov_red[c], 0));
        }
    }

private:
    void check(const PromptSpan& sp) const
    {
        // (GptContextAttentionLayer::forward cuts a token range out of base pointers, and only for a single sequence)
        FTCF_CHECK_ARG(sp.tokens ? (B == 1 && 0 <= sp.s0 && sp.s0 < sp.s1 && sp.s1 <= S) : (0 <= sp.b0 && sp.b0 < sp.b1 && sp.b1 <= B),
                       "a prompt span is sequences [b0, b1) of the batch or a token range [s0, s1) of a batch of one sequence");
    }

    // layer l for the rows of `sp` on stream s; reduce(buf, count): the layer's all-reduce as the walk mode orders it
    template<typename Reduce>
    void layer(int l, const PromptSpan& sp, hipStream_t s, Reduce&& reduce) const
    {
        const LayerWeights& w  = layers[l];
        const LayerWeights* nx = l + 1 < L ? &layers[l + 1] : nullptr;
        const bool   dual = residual_dual_ln_supported(H), tp1 = tp == 1;
        const size_t o = sp.tokens ? (size_t)sp.s0 : (size_t)sp.b0 * S;
        const int    M = sp.tokens ? sp.s1 - sp.s0 : (sp.b1 - sp.b0) * S;
        f16 *const   xr = px + o * H, *const n1 = pnrm + o * H, *const n2 = pnrm2 + o * H, *const at = patt + o * H, *const ff = pffn + o * H;
        f16 *const   kl = k_cache + l * layer_stride, *const vl = v_cache + l * layer_stride;
        // both LayerNorms of the layer come from one pass over x, fused with the previous layer's residual when there is no
        // collective in between
        if (!dual) {
            launch_layernorm(xr, w.ln1_g, w.ln1_b, n1, M, H, 1e-5f, true, s);
            launch_layernorm(xr, w.ln2_g, w.ln2_b, n2, M, H, 1e-5f, true, s);
        }
        else if (l == 0 || !tp1) {
            launch_residual_dual_ln(xr, nullptr, nullptr, nullptr, 1, 0, w.ln1_g, w.ln1_b, w.ln2_g, w.ln2_b, n1, n2, M, H, 1e-5f, s);
        }
        if (sp.tokens) {  // base pointers + the range: the earlier tokens' K/V are in the cache
            attention.forward(pnrm, pqkv, pctx, patt, w, input_lengths, kl, vl, 1, S, s_max, tile, s, sp.s0, sp.s1);
        }
        else {  // whole sequences: the attention layer on their rows of every buffer and their rows of the cache
            const size_t cb = (size_t)sp.b0 * (layer_stride / B);
            attention.forward(n1, pqkv + o * 3 * hl, pctx + o * hl, at, w, input_lengths + sp.b0, kl + cb, vl + cb, sp.b1 - sp.b0, S,
                              s_max, tile, s);
        }
        ffn.forward(n2, pmid + o * il, ff, w, M, s);
        // layer_input == layer_output for every layer with padding removal -> fp32-sum variant of the residual
        // (GptNeoXContextDecoder.cc:311-322,:445-461), whatever l is
        if (dual && tp1) {
            launch_residual_dual_ln(xr, ff, at, w.ffn2.bias, 1, 1, nx ? nx->ln1_g : nullptr, nx ? nx->ln1_b : nullptr,
                                    nx ? nx->ln2_g : nullptr, nx ? nx->ln2_b : nullptr, n1, n2, M, H, 1e-5f, s);
        }
        else {
            launch_add_bias_attn_ffn_residual(xr, ff, at, xr, w.ffn2.bias, M, H, tp, 1, true, s);
            if (!tp1) {
                reduce(xr, (size_t)M * H);
            }
        }
    }
};

struct DynamicDecodeLayer {
    // beam_width 1: temperature / penalties / end mask, top-k and top-p sampling, stop criteria (DynamicDecodeLayer.cc:410-497)
    void forward(const SamplingParams& sp, hipStream_t s, bool with_finish = true) const { launch_dynamic_decode(sp, s, with_finish); }
    // beam_width > 1: online beam search + the shared stop criteria (:309-408)
    void forward(const BeamParams& bp, const SamplingParams& sp, hipStream_t s) const
    {
        launch_beam_search(bp, s);
        launch_decode_finish(sp, s);
    }
};

}  // namespace ftcf
