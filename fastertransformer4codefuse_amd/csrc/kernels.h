// Internal launcher declarations shared by the engine and the C ABI (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ftcf_common.h"

namespace ftcf {

constexpr int GEMV_SPLITK_MAX_WAVES = 16;
constexpr int EPI_PLAIN             = 0;
constexpr int EPI_RESIDUAL          = 1;

struct LnGemvParams {
    const f16* x;  // [M, K] layer input
    const f16 *gamma0, *beta0, *gamma1, *beta1;
    const void *W0, *W1;          // tiled weights of segment 0 (QKV) / 1 (FFN1)
    const f16 *scale0, *scale1;   // int8 only
    const f16* bias1;
    f16 *out0, *out1;             // [M, NT0*16], [M, NT1*16]
    int   K, NT0, NT1, blocks0, blocks1;
    float eps;
};

struct SplitKParams {
    const f16 *x_a, *x_b;
    const void *W_a, *W_b;
    const f16 *scale_a, *scale_b;
    const f16* bias;
    const f16* x_in;  // residual input (EPI_RESIDUAL)
    const f16* ffn_in;  // EPI_RESIDUAL with a single segment: the FFN output comes from this buffer (two-stream path)
    f16*       out;
    int        N, KT_a, KT_b;
    int        act, tp, inplace_variant;
    int        nwaves, slice_halves;
    int        wave_seg[GEMV_SPLITK_MAX_WAVES], wave_t0[GEMV_SPLITK_MAX_WAVES], wave_nt[GEMV_SPLITK_MAX_WAVES];
};

// K3 in its balanced form: every 16-column group is cut into Q chunks of the concatenated K range [x_a ; x_b]; one
// 2-wave workgroup per (group, chunk), partial sums handed to the chunk-0 workgroup as {tag,value} granules.
struct ChunkParams {
    const f16 *x_a, *x_b;
    const void *W_a, *W_b;
    const f16 *scale_a, *scale_b;
    const f16* bias;
    const f16* x_in;
    f16*       out;
    int        N, KT_a, KT_b, Q, T;  // T = tiles per chunk
    int        tp, inplace_variant;
    unsigned long long* gran;  // [N/16][Q][2][M][16]
    const int* d_step;
    int        step, salt;
};
int    chunk_pick_q(int NT, int KT_total);
size_t chunk_workspace_bytes(int N, int M, int Q);
void   launch_gemv_chunked(const ChunkParams& p, bool int8, int M, hipStream_t s);
void launch_ln_gemv(const LnGemvParams& p, bool int8, int M, hipStream_t s);
// one 16-column group per workgroup of `wpg` waves (balanced form, grid = NT0 + NT1)
void launch_ln_gemv_group(const LnGemvParams& p, bool int8, int M, int wpg, hipStream_t s);
void plan_splitk(SplitKParams& p, bool int8, int M, int max_waves);
void launch_gemv_splitk(const SplitKParams& p, bool int8, int M, int epi, hipStream_t s);
// optional fused LayerNorm of x (gamma != NULL)
void launch_lm_head(const f16* x, const f16* W, float* logits, int M, int n_rows, int K, int ldc, hipStream_t s,
                    const f16* gamma = nullptr, const f16* beta = nullptr, float eps = 1e-5f, const int* d_stop = nullptr);

// ---- MFMA GEMM (prefill / batched decode) : kernels_gemm.hip ----
// C[m,n] = A[m,k] x W(tiled)  (+bias, gelu) ; int8: fused fp32 epilogue ; fp16: half epilogue
// `workspace` (gemm_tiled_workspace_bytes(), zeroed once; NULL = none): lets m <= 256 cut the K extent of its few tiles into
// slices reduced inside the launch.  One workspace serves one stream.
size_t gemm_tiled_workspace_bytes();
size_t gemm_tiled_ticket_bytes();  // the workspace's tail
int    gemm_tiled_splitk_max_m();  // rows up to which launch_gemm_tiled uses the workspace (FTCF_GEMM_SPLITK_MAX_M)
void   launch_gemm_tiled(const f16* A, const void* W, const f16* scale, const f16* bias, int act, f16* C, int m, int n,
                         int k, bool int8, hipStream_t s, float* workspace = nullptr);
// the form launch_gemm_tiled runs (m, n, k) in: its own variables, decided on the host without a device (ftcf_gemm_plan mirrors it)
enum GemmTiledFamily {
    GEMM_TILED_SPLITK    = 0,  // tiles cut along K, the slices reduced inside the launch (needs the workspace)
    GEMM_TILED_ROWS32    = 1,  // 32 x 64 tiles on four waves, 2-D grid (no workspace, m <= 32)
    GEMM_TILED_ONE_WG    = 2,  // one workgroup of eight waves per 64- or 128-row tile
    GEMM_TILED_FOUR_WAVE = 3,  // fp16 weights from 2048 rows: 128 x 256 tiles on four waves
};
struct GemmTiledPlan {
    int family;           // GemmTiledFamily
    int tile_rows;        // 32 / 48 / 64 / 128
    int gx, gy;           // column blocks, row blocks
    int slices;           // K slices per tile (1 outside the split-K family)
    int steps_per_slice;  // k-steps of 64 per slice; the last slice may hold fewer
    int ring;             // 0 (plain loop), 2 or 4 k-steps
    int prefetch;         // A fragments of a k-step read from LDS ahead of the dequantisation (PF)
    int two_per_cu;       // register budget of two workgroups per CU (OCC2)
    int lone;             // one-workgroup-per-tile family: at most 256 tiles, one workgroup per CU anyway
    int grid;             // workgroups launched (gx rounded up to 8 where workgroups are placed by XCD)
};
GemmTiledPlan gemm_tiled_plan(int m, int n, int k, bool int8, bool has_workspace);
// batched decode GEMM for m <= 16 rows (HBM bound forms); with a `workspace` (>= gemm_smallm_workspace_bytes of this
// GEMM) the burst form runs: K slices of 20 tiles, every wave requests its whole slice at once
// at once; `workspace` = [partial_bytes of split-K partial sums][gemm_smallm_ticket_bytes(), zeroed once before the first
// launch]: the reduction runs in the workgroup that takes the last ticket of a column block (no second launch)
size_t gemm_smallm_workspace_bytes(int m, int n, int k, bool int8);
size_t gemm_smallm_ticket_bytes();
struct SmallmDesc {  // C[m, n] = epilogue(A[m, k] x W[k, n]); act 1 = bias + gelu
    const f16*  A;
    const void* W;
    const f16*  scale;
    const f16*  bias;
    int         act;
    f16*        C;
    int         n, k;
};
// one launch for up to two independent GEMMs with the same m (partial_bytes >= the SUM of their workspace bytes)
// d_step: device-resident decode step (part of the launch's granule tag, a replayed hipGraph freezes scalars) or NULL;
// seq: the workspace's launch counter (host).  The granules must be zero when a request begins.
void   launch_gemm_smallm_group(const SmallmDesc* d, int np, float* workspace, size_t partial_bytes, int m, bool int8,
                                hipStream_t s, const int* d_step, unsigned* seq, size_t partial_offset = 0);
void   launch_gemm_smallm(const f16* A, const void* W, const f16* scale, const f16* bias, int act, f16* C, float* workspace,
                          size_t partial_bytes, int m, int n, int k, bool int8, int num_cu, hipStream_t s,
                          const int* d_step = nullptr, unsigned* seq = nullptr);
// logits_f32[m, n] = A[m,k] x W[n,k]^T (row major fp16 weights, m > 4)
void launch_gemm_nk_f32out(const f16* A, const f16* W_nk, float* C, int m, int n, int k, int ldc, hipStream_t s);

// ---- misc : kernels_misc.hip ----
void launch_layernorm(const void* x, const void* gamma, const void* beta, void* out, int m, int n, float eps,
                      bool fp16, hipStream_t s);
// [x += residual of the previous layer;] out1 = LN(x; g1, b1), out2 = LN(x; g2, b2) in one pass (ffn == NULL: no
// residual; g1 == NULL: residual only)
bool residual_dual_ln_supported(int n);
void launch_residual_dual_ln(f16* x, const f16* ffn, const f16* attn, const f16* bias, int tp, int inplace_variant,
                             const f16* g1, const f16* b1, const f16* g2, const f16* b2, f16* out1, f16* out2, int m,
                             int n, float eps, hipStream_t s, int bias_mul = 1, int sum_mul = 1);
// out = (bias + a) + b in fp32, rounded once (sequential-residual layers)
void launch_add_bias_residual(f16* out, const f16* a, const f16* b, const f16* bias, int m, int n, hipStream_t s);
void launch_add_bias_attn_ffn_residual(void* out, const void* ffn, const void* attn, const void* in, const void* bias,
                                       int m, int n, int tp, int inplace_variant, bool fp16, hipStream_t s);
void launch_embedding(f16* out, const f16* table, const int* ids, int n_ids, int H, hipStream_t s);
// prompt: ids [B,S] -> out [B*S,H] and time-major output_ids[s*B+b] (gpt_kernels.cu:31-104)
void launch_prompt_embedding(f16* out, int* output_ids, const f16* table, const int* ids, int B, int S, int H,
                             hipStream_t s);
// decode step: embedding of output_ids[(step-1)*B + b] where step is read from device state (decoding_kernels.cu:145-191)
void launch_step_embedding(f16* out, const f16* table, const int* output_ids, const int* d_step, int B, int H,
                           hipStream_t s);
// out[r] = hidden[r / tile][input_lengths[r / tile] - 1] for r < B * tile (beam search: every beam starts from beam 0's state)
void launch_gather_last_token(f16* out, const f16* hidden, const int* input_lengths, int B, int S, int H,
                              hipStream_t s, int tile = 1);
// output_ids[s][b * K + k] = ids[b][s] (time-major ids of the tiled prompt)
void launch_tile_prompt_ids(int* output_ids, const int* ids, int B, int K, int S, hipStream_t s);
void launch_fp16_rowmajor_to_tiled(const f16* w, size_t K, size_t N, f16* out, hipStream_t s);

// ---- weight-only int8 quantiser on the device : kernels_quant.hip ----
// host_symmetric_quantize_int8 (host_quant.h) bit for bit: w [E, K, N] row major (dtype 0 fp32, 1 fp16, 2 bf16 raw bits) ->
// out_q [E, K, N] bytes in the int8 tile layout + out_scale [E, N] in the weight dtype.  K % 64 == 0, N % 16 == 0, every pointer
// 16-byte aligned; workspace: symmetric_quantize_int8_workspace_bytes(E, N) = E * N * 4 bytes (the fp32 column maxima), any contents.
size_t symmetric_quantize_int8_workspace_bytes(size_t E, size_t N);
void   launch_symmetric_quantize_int8(const void* w, int dtype, size_t E, size_t K, size_t N, int8_t* out_q, void* out_scale,
                                      void* workspace, hipStream_t s);

// ---- attention : kernels_attn.hip ----
struct MmhaParams {
    const f16* qkv;       // [B, 3*Hl]
    const f16* qkv_bias;  // [3*Hl]
    f16 *      k_cache, *v_cache;  // [B, nh, s_max, dh]
    const int* seq_len;            // tlength per row
    const int* pad_count;
    const uint8_t* masked_tokens;  // [B, s_max]
    const uint8_t* finished;
    const int*     d_step;  // device step counter (timestep = step - 1); if NULL `step` is used
    const float*   rot_table;  // optional [B][rot/2][2] {cos, sin} of this step's rotary position
    int            step;
    int            B, nh, dh, rot, s_max;
    f16*           ctx;  // [B, Hl]
    unsigned long long* gran;  // split-KV hand-off slab: [B][nh][nsplit][dh+2] {tag,value} granules (zero at request start)
    int            layer;      // tag salt: unique per launch within a token
    int            nsplit;
    // beam search (standalone launch_mmha only): [2][B][s_max] ping-pong planes of the cache indirection, B = batch * beam
    const int*     cache_indir;
    int            beam_width, max_input_len;
    size_t         indir_plane;  // elements per plane
};
size_t mmha_workspace_bytes(int B, int nh, int dh, int nsplit);
int    mmha_pick_nsplit(int B, int nh, int s_max);
size_t mmha_smem_bytes(int dh, int s_max, int nsplit);
void   launch_mmha(const MmhaParams& p, hipStream_t s);
bool   mmha_head_size_supported(int dh);  // the reference's list (DecoderSelfAttentionLayer.cc:280-282)
// {cos, sin}(pos * 10000^(-2j/rot)), pos = step - 1 - pad_count[b], once per token (decoder_masked_multihead_attention_utils.h:1325-1329)
void   launch_rotary_table(float* table, const int* d_step, const int* pad_count, int B, int rot, hipStream_t s);
// launch_step_embedding + launch_rotary_table in one launch
void   launch_step_prologue(f16* out, const f16* table, const int* output_ids, const int* d_step, float* rot_table,
                            const int* pad_count, int B, int H, int rot, hipStream_t s, const int* d_stop = nullptr);
// (d_stop, here and below: device flag "every row has finished" -- the kernel returns at once when it is set)
void   launch_context_attention(const f16* qkv, const f16* qkv_bias, const int* input_lengths, f16* k_cache,
                                f16* v_cache, int B, int S, int nh, int dh, int rot, int s_max, f16* ctx,
                                hipStream_t s, int cache_row_mult = 1, int s_lo = 0,
                                int s_hi = -1);  // K/V of prompt row b live in cache row b * mult

// paged decoder attention (continuous batching front end): per-slot page tables into a shared K/V pool
struct MmhaPagedParams {
    const f16*     qkv;       // [B, 3*Hl]
    const f16*     qkv_bias;  // [3*Hl]
    f16 *          kpool, *vpool;  // THIS layer's pool: [num_pages][nh][P][dh]
    const int*     page_table;     // [B][max_pages]
    const int*     len;            // [B] cached tokens of the slot (= position of the current token)
    const uint8_t* finished;       // [B] 1: slot empty or finished (skipped)
    int            B, nh, dh, rot, P, max_pages;
    f16*           ctx;  // [B, Hl]
};
size_t mmha_paged_smem_bytes(int dh, int max_pages, int max_len);
void   launch_mmha_paged(const MmhaPagedParams& p, int max_len, hipStream_t s);
void   launch_scatter_kv_to_pages(const f16* kc, const f16* vc, f16* kpool, f16* vpool, const int* pages, int L, int nh, int dh,
                                  int s_max, int S, int P, size_t pool_layer_elems, hipStream_t s, size_t src_layer_elems = 0);
// the inverse (the batcher's prefix cache): tokens [0, T) (T a multiple of P) of a sequence's pages -> a row of the engine cache
void   launch_gather_pages_to_kv(f16* kc, f16* vc, const f16* kpool, const f16* vpool, const int* pages, int L, int nh, int dh,
                                 int s_max, int T, int P, size_t pool_layer_elems, hipStream_t s, size_t dst_layer_elems = 0);
// whole pages of every layer of both pools <-> a contiguous staging buffer [n][2 (K, V)][L][page_elems] (the batcher's swap
// space: preemption under overcommit); page_elems = nh * P * dh, a multiple of 8.  Bit-exact copies, exact inverses.
void   launch_pages_pack(f16* staging, const f16* kpool, const f16* vpool, const int* pages, int n, int L, size_t page_elems,
                         size_t pool_layer_elems, hipStream_t s);
void   launch_pages_unpack(const f16* staging, f16* kpool, f16* vpool, const int* pages, int n, int L, size_t page_elems,
                           size_t pool_layer_elems, hipStream_t s);

// ---- fused attention + FFN1 weight stream : kernels_fused.hip ----
void launch_mmha_ln_gemv(const MmhaParams& ap, const LnGemvParams& gp, bool int8, int M, hipStream_t s);

// ---- persistent decode layers : kernels_persist.hip ----
// One launch runs layers [l_begin, l_end) of the m <= 2 decode step on ONE resident workgroup per CU; the stages of a
// layer hand their vectors over inside the launch (sc1 stores + counters, {tag,value} granules) and every wave already
// holds the first weight batches of the next stage while the hand-off is in flight.
struct PersistLayer {
    const f16 *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const void *w_qkv, *w_ffn1, *w_out, *w_ffn2;  // engine tile images
    const f16 *s_qkv, *s_ffn1, *s_out, *s_ffn2;   // int8 scales
    const f16 *b_qkv, *b_ffn1, *b_res;            // qkv bias (added by attention), ffn1 bias, residual-epilogue bias
    f16 *      k_cache, *v_cache;                 // [B, nh, s_max, dh] of this layer
};
struct PersistPlan {
    int    ok;        // 0: shape not eligible (caller uses the per-kernel path)
    int    NB;        // workgroups (<= CUs)
    int    nsplit;    // split-KV factor of the attention stage
    int    uk;        // K / V wave-loads per lane of the attention stage (8: <= 256 keys per split, 12: <= 384)
    int    PA, PB;    // K pieces per 16-column group of out-proj / FFN2
    int    RLa, RLb;  // tiles per piece
    int    xs_halves; // LDS x region
    int    e1, e3;    // tile-table entries per wave (P1 / P3)
    int    cs1, cs3;  // stream share of a control wave in 1/16 of a streamer wave's (P1 / P3)
    int    qrot;      // rotation of the QKV column-group split over the workgroups (which ones get the lighter P1 share)
    int    own;       // P3 in the own-group layout (whole column groups per workgroup: one hop at the layer boundary)
    long   gp_n;      // granules of the partial-sum slab (PersistParams::gp)
    size_t smem;
};
struct PersistParams {
    const PersistLayer* layers;  // device array [L]
    int                 L, l_begin, l_end;
    const f16*          x_in;        // [M][H] input of layer l_begin (plain memory)
    f16*                x_out;       // [M][H] output of layer l_end-1
    // granule slabs (pairs of halves unless noted): qkv [M][3Hl/2], mid [M][Il/2], ctx [M][Hl/2], x' [M][H/2],
    // K pieces [NG*(PA+PB)][M*16] (fp32; own-group layout: plan.gp_n granules), attention partials [B][nh][nsplit][dh+2] (fp32); zero at request start
    unsigned long long *gq, *gm, *gc, *gx, *gp, *ga;
    int*                err;              // sticky give-up flag (0 = fine)
    int                 H, Hl, Il, nh, dh, rot, s_max, B, tp;
    PersistPlan         plan;
    const int*          d_step;
    const int*          d_stop;  // optional device flag "every row has finished": the launch returns at once when it is set
    const int*          seq_len;
    const int*          pad_count;
    const uint8_t*      masked_tokens;
    const uint8_t*      finished;
    const float*        rot_table;
    float               eps;
    long long*          ts;          // optional [NB][L][8 waves][16] wall-clock stamps (100 MHz), or NULL
    // tensor parallel (tp > 1): this rank and the exchange windows of ALL ranks as this rank addresses them (own memory
    // for xw[tp_rank], peer mappings otherwise); window layout [tp source ranks][M*H/2] granules of {tag, pair of halves}
    int                 tp_rank;
    unsigned long long* xw[8];
    // the plan's run / tile tables, precomputed once per plan: [NB][persist_table_bytes(plan)] ; tab_mode 0: none (build in
    // the launch), 1: build and store (a launch over no layers), 2: load
    char*               tab;
    int                 tab_mode;
};
constexpr int PERSIST_MAX_TP = 8;
struct PersistGroupParams {  // local group launch: every rank's parameters, nb workgroups each
    PersistParams p[PERSIST_MAX_TP];
    int           world, nb;
};
PersistPlan persist_plan(int B, int H, int Hl, int Il, int nh, int dh, int s_max, bool int8, int num_cu, int force_nb,
                         int cs1, int cs3, int own = 0, int L = 0);
// every workgroup of the plan's grid resident at once on this device?  (also raises the kernel's dynamic-LDS limit there)
bool        persist_resident(const PersistPlan& pl, bool int8, int M, int dh, int num_cu, int tp = 1);
// bytes of the table region one workgroup stores / loads (PersistParams::tab holds NB of them)
size_t      persist_table_bytes(const PersistPlan& pl);
void        launch_decode_persistent(const PersistParams& p, bool int8, hipStream_t s);
// all ranks of a local group in one launch (grid = world * NB): residency of the whole group
bool        persist_group_resident(const PersistPlan& pl, bool int8, int M, int dh, int num_cu, int world);
void        launch_decode_persistent_group(const PersistGroupParams& g, bool int8, hipStream_t s);
// tensor-parallel instantiations (kernels_persist_tp.hip); nullptr when the shape has none
const void* persist_tp_kernel(bool int8, int M, int dh, int uk, bool group, int own = 0);
// own-group instantiations for one GPU (kernels_persist_own.hip)
const void* persist_own_kernel(bool int8, int M, int dh, int uk);

// ---- persistent decode layers for 3..16 rows : kernels_rows.hip ----
// One launch runs layers [l_begin, l_end) of the batched decode step (GptNeoXDecoder.cc:245-384, any B <= 16) on one resident
// 8-wave workgroup per CU.  A layer is five chip-wide streams -- QKV, FFN1, the K/V rows of the attention, FFN2, out-proj --
// in that order, so that every hand-off but the layer boundary travels under the stream that follows its producer.  Weight
// tiles are walked k-major over up to five 16-column groups per workgroup with the rows' MFMA A fragments fetched per k-step
// from L2 (sc1 loads of the producers' write-through stores); hand-offs are flags behind drained write-through stores.
struct RowsPlan {
    int    ok;
    int    NB;            // workgroups (<= CUs)
    int    g1;            // kernel instantiation: column groups per k-step of the QKV pass (4 or 5)
    int    CB, KP2, KP3;  // row-parallel GEMMs: column blocks of RW_G groups, K pieces of FFN2 / out-proj
    int    U;             // attention units of a workgroup at most: whole (row, head) pairs (pair = workgroup + u * NB) + one part
    int    FX;            // ... of a leftover pair: each of the M nh % NB leftover pairs is shared by FX workgroups
    int    CR, cw;        // the layer boundary: column ranges per row (merger = row * CR + range), columns per range
    int    wcum[8];       // K shares of the seven streamer waves: wave s streams [n wcum[s] / wcum[7], n wcum[s + 1] / wcum[7]) of a
                          // workgroup's n k-steps (equal shares; unequal ones measured no better: profiles/r05_notes.md)
    size_t smem;
};
struct RowsParams {
    const PersistLayer* layers;  // device array [L] (k_cache / v_cache: this layer's [B][nh][s_max][dh])
    int                 L, l_begin, l_end;
    const f16*          x_in;   // [M][H] input of layer l_begin (plain memory)
    f16*                x_out;  // [M][H] output of layer l_end - 1
    // the hand-off region: ONE buffer (one descriptor inside the kernel), byte offsets of its parts
    char*               ws;
    unsigned            ws_bytes;
    unsigned            o_fq, o_fm, o_fc, o_f2, o_f3;  // [NB] flags: q|k|v / mid / ctx / FFN2 piece / out-proj piece of a workgroup
    unsigned            o_xs;     // [2][M * CR] 16-byte granules {tag, sum, sum of squares, 0} of a merger's piece of x'
    unsigned            o_xb[2];  // layer inputs handed over inside the launch (layer l reads xb[l & 1]): [M][H] halves
    unsigned            o_qkv, o_mid, o_ctx;  // [M][3 Hl], [M][Il], [M][Hl] halves
    unsigned            o_p2, o_p3;           // fp32 partial sums of FFN2 / out-proj: [KP][M][H]
    unsigned            o_fa, o_pa;           // shared pairs: [NB] flags, [NB][dh + 4] {out, max, sum} of a part
    int*                err;                  // (= ws)
    int                 M, H, Hl, Il, nh, dh, rot, s_max, tp;
    RowsPlan            plan;
    const int*          d_step;
    const int*          d_stop;
    const int*          seq_len;
    const int*          pad_count;
    const int*          input_lengths;  // keys [input_lengths[b], max_input_len) of row b are padding (never attended)
    int                 max_input_len;
    const uint8_t*      finished;
    const float*        rot_table;
    float               eps;
    long long*          ts;  // optional [NB][L][8][16] stamps
    // paged K/V (continuous batching): page_table != NULL -> row b's key t lives in page page_table[b * max_pages + t / P] of
    // the layer's pool [num_pages][nh][P][dh] (k_cache / v_cache of the layer table point at the pools)
    const int*          page_table;
    int                 page_tokens, max_pages;
};
RowsPlan rows_plan(int M, int H, int Hl, int Il, int nh, int dh, int s_max, bool int8, int num_cu, int force_nb);
bool     rows_resident(const RowsPlan& pl, bool int8, int dh, int num_cu, bool paged);  // (the K/V form the caller will launch)
// bytes of the hand-off region (flags first: rows_flag_bytes() of it must be zero when a request begins) and its carve
size_t   rows_workspace_bytes(const RowsPlan& pl, int M, int H, int Hl, int Il, int nh, int dh);
size_t   rows_flag_bytes(const RowsPlan& pl, int M, int nh);
void     rows_carve(RowsParams& p, void* workspace);  // fills the buffer pointers of p (M, H, ..., plan set)
void     launch_decode_rows(const RowsParams& p, bool int8, hipStream_t s);
int      rows_paged_block(int dh);  // page_tokens of a paged K/V cache must be a multiple of this

// ---- fp32 instantiation (FTGptNeoX<float>, GptNeoXOp.cc:56-70) : kernels_fp32.hip ----
struct Mmha32Params {
    const float*   qkv;       // [B, 3*Hl]
    const float*   qkv_bias;  // [3*Hl]
    float *        k_cache, *v_cache;  // [B, nh, s_max, dh]
    const int*     seq_len;
    const int*     pad_count;
    const uint8_t* masked_tokens;  // [B, s_max]
    const uint8_t* finished;
    const int*     d_step;
    int            B, nh, dh, rot, s_max;
    float*         ctx;  // [B, Hl]
    const int*     cache_indir;  // beam search: [2][B][s_max], or NULL
    int            beam_width, max_input_len;
    size_t         indir_plane;
};
void launch32_prompt_embedding(float* out, int* output_ids, const float* table, const int* ids, int B, int S, int H,
                               hipStream_t s);
void launch32_step_prologue(float* out, const float* table, const int* output_ids, const int* d_step, float* rot_table,
                            const int* pad_count, int B, int H, int rot, hipStream_t s);
void launch32_gather_last_token(float* out, const float* hidden, const int* input_lengths, int B, int S, int H,
                                hipStream_t s, int tile = 1);
void launch32_add_bias_residual(float* out, const float* a, const float* b, const float* bias, int m, int n, hipStream_t s);
void launch32_gemm(const float* A, const float* W, const float* bias, int act, float* C, int m, int n, int k, hipStream_t s);
void launch32_lm_head(const float* A, const float* W_nk, float* logits, int m, int n, int k, int ldc, hipStream_t s);
void launch32_context_attention(float* qkv, const float* qkv_bias, const int* input_lengths, float* k_cache, float* v_cache,
                                int B, int S, int nh, int dh, int rot, int s_max, float* ctx, hipStream_t s,
                                int cache_row_mult = 1);
void launch32_mmha(const Mmha32Params& p, hipStream_t s);

// ---- fused LM head -> per-row log-probability of a target token : kernels_logprob.hip ----
// log_probs[r] = l[r, targets[r]] - logsumexp_j l[r, j], l = A[m,k] (fp16) x W[n,k]^T (fp16, fp32 accumulation); targets[r] < 0
// (or >= n) gives 0; row_lse [m] or NULL.  k % 8 == 0.  ws: lm_head_log_probs_workspace_bytes(m, n) bytes, no zeroing needed.
size_t lm_head_log_probs_workspace_bytes(int m, int n);
void   launch_lm_head_log_probs(const f16* A, const f16* W_nk, const int* targets, float* log_probs, float* row_lse, int m, int n,
                                int k, void* ws, hipStream_t s);
// a grow-only workspace of at least that size per (device, stream), kept for the life of the process
void*  lm_head_log_probs_workspace(int m, int n, hipStream_t s);
// the engine's context_log_probs [B, S] from the final-LayerNorm'd prompt rows hidden_nrm [B*S, H]: targets / lp are [B*S] scratch
void   launch_context_log_probs(float* out, const f16* hidden_nrm, const f16* W_nk, const int* ids, const int* lengths, int* targets,
                                float* lp, int B, int S, int V, int H, hipStream_t s);
// output_log_probs: the time-major [T, B] buffer of the token loop -> [B, T]
void   launch_transpose_log_probs(float* out, const float* in, int T, int B, hipStream_t s);
// top_logprobs: `pairs` {id, log-probability} pairs <- the pattern of a row that had finished before the step, (-1, 0.0f); the
// time-major buffers of the token loop [T, B, N] -> [B, T, N]
void   launch_fill_top_logprobs(int* ids, float* values, size_t pairs, hipStream_t s);
void   launch_transpose_top_logprobs(int* out_ids, float* out_values, const int* ids, const float* values, int T, int B, int N,
                                     hipStream_t s);

// ---- dynamic decode : kernels_sampling.hip ----
// the words of `h_flags`, the pinned mailbox through which the step-closing kernels tell the host how the step ended (the host
// reads it behind an event or a synchronisation of the stream, never while a launch runs)
enum HostFlag {
    FLAG_ALL_FINISHED      = 0,  // every row has finished
    FLAG_LAST_STEP         = 1,  // the last step written (the step that produced FLAG_ALL_FINISHED)
    FLAG_LM_GREEDY_GAVE_UP = 2,  // k_lm_head_greedy's finishing workgroup gave up waiting for a partial (the host clears it)
    FLAG_SPEC_EMITTED      = 3,  // tokens emitted by a verify pass
    FLAG_SPEC_NEXT_DRAFTS  = 4,  // the draft kernel's count for the next step
    FLAG_SPEC_ACCEPTED     = 5,  // drafts of the verify pass that became output tokens
    FLAG_COUNT             = 6,
    // a verify pass (k_verify_close, k_verify_sample_close): the tokens it emitted and the sequence length behind each
    FLAG_SPEC_TOKENS       = 16,  // [VERIFY_MAX_ROWS]
    FLAG_SPEC_SEQ_LEN      = 32,  // [VERIFY_MAX_ROWS]
    FLAG_WORDS             = 48   // words of the engine's mailbox
};
struct DecodeState {  // device resident, one per engine
    int step;         // current step (max_input_len .. total-1)
    int all_finished;
    int steps_done;
    int pad;          // ticket counter of k_greedy_decode (zero between launches)
};
struct SamplingParams {
    float*       logits;  // [B, V] fp32 (modified in place)
    int          B, V;
    int          max_input_len, total_len, end_id;
    const int*   input_lengths;
    const int*   top_k;        // device [B] effective k (0 => row belongs to the top-p layer)
    int          max_top_k, any_top_p;  // host view of the same: largest k of the batch, any top-p row (LDS sizing)
    const float* top_p_topk;   // device [B] p used by the top-k layer
    const float* top_p_topp;   // device [B] p used by the top-p layer
    const float* temperature;  // device [B]
    const float* repetition_penalty;  // device [B] or NULL
    const int*   min_length;          // device [B] or NULL
    const uint64_t* random_seed;      // device [B]
    uint64_t*       draw_counter;     // device [B]
    int             apply_temperature, apply_repetition;  // host decided (BaseSamplingLayer.cc:283-313 ALL_OF logic)
    const int*      stop_words;       // device [B,2,stop_len] or NULL
    int             stop_len;
    const int*      optional_last_tokens;  // device [B,M] or NULL
    int             optional_count;
    int             return_cum_log_probs;
    int*            output_ids;  // time-major [total, B]
    uint8_t*        finished;
    int*            seq_len;
    float*          cum_log_probs;
    // the log-probability each step adds to cum_log_probs, time-major [total_len - max_input_len, B] at row (step - max_input_len)
    // (row 0 with row_len: one step per launch), or NULL.  Needs return_cum_log_probs.
    float*          output_log_probs;
    int*            pad_count;
    DecodeState*    state;
    int*            h_flags;  // pinned host mirror, indexed by HostFlag: FLAG_ALL_FINISHED, FLAG_LAST_STEP, FLAG_LM_GREEDY_GAVE_UP
    void*           ws;       // workspace (see sampling_workspace_bytes)
    // continuous batching: every row has its OWN step -- row b's token history is output_ids[0 .. row_len[b]] (time-major
    // as always), the new token goes to position row_len[b] + 1.  NULL: the batch-wide state->step
    const int*      row_len;
    // k_greedy_decode only: the NEXT token's prologue (k_step_prologue: embedding row of the token just chosen + the rotary table
    // of the next step) done by the workgroup that finishes the step; next_x NULL: the engine launches k_step_prologue itself
    f16*            next_x;     // [B, H]
    const f16*      wte;        // [V, H]
    float*          rot_table;  // [B, rot / 2, 2]
    int             H, rot;
    // the top_logprobs (1..TOP_LOGPROBS_MAX) best {id, log-probability} pairs of every live row's processed distribution (the one
    // output_log_probs is defined under), time-major [total_len - max_input_len, B, top_logprobs] at row (step - max_input_len)
    // (row 0 with row_len), or 0 / NULL.  Needs return_cum_log_probs; the step then takes the general form.
    int             top_logprobs;
    int*            top_logprob_ids;
    float*          top_logprob_values;
};
constexpr int TOP_LOGPROBS_MAX = 20;
// does launch_dynamic_decode(p, s, finish) take the one-launch path of an all-greedy batch (k_greedy_decode)?
bool dynamic_decode_is_fused(const SamplingParams& p, bool finish);
// which form launch_dynamic_decode(p, s, finish) takes: 0 the general four launches, 1 k_topk_decode, 2 k_greedy_decode
int  dynamic_decode_form(const SamplingParams& p, bool finish);
// beam search (beam_width > 1): OnlineBeamSearchLayer semantics, rows bb = batch * K + beam
constexpr int BEAM_MAX_K = 64;  // online_softmax_beamsearch_kernels.cu:691-695
struct BeamParams {
    float*       logits;  // [B*K, V] fp32 (modified in place)
    int          B, K, V;
    int          max_input_len, total_len, end_id, s_max;
    const int*   input_lengths;       // device [B*K] (tiled)
    const float* temperature;         // device [B]
    const float* repetition_penalty;  // device [B] or NULL
    const float* diversity_rate;      // device [B]
    const float* len_penalty;         // device [B]
    const int*   min_length;          // device [B] or NULL
    const int*   stop_words;          // device [B,2,stop_len] or NULL
    int          stop_len;
    const int*   optional_last_tokens;  // device [B,M] or NULL
    int          optional_count;
    int *        output_ids, *parent_ids;  // time-major [total, B*K]
    uint8_t*     finished;
    int*         seq_len;
    float*       cum_log_probs;
    // the step's log-probability of every row's token, cum_new[bb] - cum_old[parent] (+0 for a beam that had finished),
    // time-major [total, B*K] like output_ids, row `step` written; or NULL
    float*       step_log_probs;
    int*         cache_indir;  // [2][B*K][s_max]: plane (step - max_input_len) % 2 is read, the other one written
    DecodeState* state;
    void*        ws;  // beam_workspace_bytes
};
size_t beam_workspace_bytes(int B, int K);
void   launch_beam_search(const BeamParams& p, hipStream_t s);  // rows + batch kernels (not the finish step)
void   launch_decode_finish(const SamplingParams& p, hipStream_t s);
void   launch_tile_inputs(int* tiled_ids, int* tiled_len, const int* ids, const int* len, int B, int K, int S,
                          hipStream_t s);
void   launch_gather_tree_beam(int* output_ids, int* sequence_lengths, const int* step_ids, const int* parent_ids,
                               const int* seq_len, const int* input_lengths, int B, int K, int max_input_len, int total,
                               int end_id, hipStream_t s);
// the log-probabilities of the hypotheses launch_gather_tree_beam returns, [B, K, total - max_input_len], from the rows
// BeamParams::step_log_probs recorded
void   launch_gather_tree_beam_log_probs(float* log_probs, const float* step_log_probs, const int* step_ids, const int* parent_ids,
                                         const int* seq_len, const int* input_lengths, int B, int K, int max_input_len, int total,
                                         int end_id, hipStream_t s);
size_t sampling_workspace_bytes(int B, int V);
void   launch_dynamic_decode(const SamplingParams& p, hipStream_t s, bool finish = true);
// LM head (final LayerNorm fused, as launch_lm_head with gamma) + the all-greedy dynamic decode of the token + the next token's
// prologue in ONE launch (k_lm_head_greedy): one GPU, <= 2 rows, a step launch_dynamic_decode would run as k_greedy_decode.
// The workgroups' partials are tagged with the step: the first lm_head_greedy_partial_bytes(B) bytes of the sampling workspace
// must be zero at the start of a request.
bool   lm_head_greedy_ok(const SamplingParams& p, int K);
size_t lm_head_greedy_partial_bytes(int B);
void   launch_lm_head_greedy(const f16* x, const f16* W, float* logits, int K, const f16* gamma, const f16* beta, float eps,
                             const SamplingParams& p, hipStream_t s);
void   launch_decode_init(uint8_t* finished, int* seq_len, float* cum_log_probs, int* pad_count, uint8_t* masked_tokens,
                          uint64_t* draw_counter, const int* input_lengths, DecodeState* st, int B, int max_input_len,
                          int s_max, hipStream_t s, int beam_width = 1);
void   launch_gather_tree(int* output_ids, int* sequence_lengths, const int* step_ids, const int* seq_len,
                          const int* input_lengths, int B, int max_input_len, int total, int end_id, hipStream_t s);

// ---- speculative greedy decoding : kernels_verify.hip ----
// Decode attention for R <= 16 consecutive new tokens of ONE sequence: qkv [R, 3 * nh * dh], the sequence's cache row
// k_cache / v_cache [nh, s_max, dh] holds positions [0, len).  Row i: bias, NeoX rotary at len + i, K / V stored at len + i,
// ctx[i] = soft-max attention over positions [0, len + i] with mmha_partial's arithmetic.  The cached keys are read once for
// all rows.  rot_table: [R, rot / 2, 2] {cos, sin} of positions len .. len + R - 1 (launch_verify_rotary) or NULL (computed
// in the kernel, the same values).  ws: verify_attention_workspace_bytes, its ticket words (the first
// verify_attention_ticket_bytes) zero before the first launch; a launch leaves them zero.
constexpr int VERIFY_MAX_ROWS = 16;
struct VerifyAttnParams {
    const f16*   qkv;
    const f16*   qkv_bias;
    f16 *        k_cache, *v_cache;  // the sequence's cache row
    const float* rot_table;
    f16*         ctx;  // [R, nh * dh]
    float*       ws;
    int          len, R, nh, dh, rot, s_max;
};
bool   verify_attention_supported(int nh, int dh, int s_max);  // head size 64 / 128, a context the merger's split table holds
size_t verify_attention_workspace_bytes(int R, int nh, int dh, int s_max);
size_t verify_attention_ticket_bytes(int nh);
void   launch_verify_attention(const VerifyAttnParams& p, hipStream_t s);
void   launch_verify_rotary(float* table, int len, int R, int rot, hipStream_t s);
// prompt-lookup drafting (one workgroup).  tokens t[0, n), n = *d_n when d_n is given: for g = min(N, n - 1) .. 1 the LARGEST
// s <= n - g - 1 with t[s, s + g) == t[n - g, n); the first g that has one wins: draft = t[s + g, min(s + g + K, n)).
// ext (a caller's own drafts, [ext_len]): draft = ext[n - ext_base, ...) instead, cut at K, at ext_len and at the first negative id.
// *n_draft (device) and, when given, *h_n_draft (pinned host) receive the count; d_stop set: nothing is drafted (count 0).
void launch_ngram_draft(const int* tokens, int n, const int* d_n, int K, int N, const int* ext, int ext_base, int ext_len,
                        int* draft, int* n_draft, int* h_n_draft, const int* d_stop, hipStream_t s);
// the input rows of a verify pass: x[0] = wte[tokens[step - 1]], x[i] = wte[draft[i - 1]]
void launch_verify_embed(f16* x, const f16* wte, const int* tokens, const int* draft, int step, int R, int H, hipStream_t s);
// The acceptance of every greedy pass -- of a bare request (stop_words, cum_log_probs, output_log_probs NULL) as of one with stop
// words, log-probabilities or a streaming callback; the stand-alone ftcf_verify_accept of include/ftcf.h is the contract -- in two
// launches.  k_verify_slices reduces every row in VERIFY_ACCEPT_SLICES vocabulary slices to {best, index, max, sum of
// exponentials}; k_verify_close merges them in slice order into a[i] = argmax of logits row i (value descending, index ascending
// on ties), takes m = the longest prefix with draft[i] == a[i] and closes the step: for i = 0 .. m in order the token a[i] goes to
// output_ids[step + i], its log-probability logf(exp(v - max) / (sum + 1e-6f)) is added to cum_log_probs[0] (sequential fp32 adds)
// and stored at output_log_probs[step + i - max_input_len], then end_id, the stop words (stop_word_ends_at at step + i, over the
// history and the tokens just written) and the length criterion are tested; nothing is written behind the first token that
// finishes the row.  seq_len[0] and the device step advance by the tokens emitted, finished / all_finished are set.
// One row of one sequence: output_ids is [total_len].  step >= max(1, max_input_len), step + R <= total_len.
// state / h_flags (the engine's, pinned, HostFlag: FLAG_ALL_FINISHED, FLAG_LAST_STEP, FLAG_SPEC_EMITTED, FLAG_SPEC_ACCEPTED,
// FLAG_SPEC_TOKENS / FLAG_SPEC_SEQ_LEN; FLAG_SPEC_NEXT_DRAFTS is the draft kernel's) and emitted / accepted / tokens [16] (device)
// may each be NULL.  ws: verify_close_workspace_bytes().
constexpr int VERIFY_ACCEPT_SLICES = 32;
struct VerifyCloseParams {
    const float* logits;  // [R, V]
    int          R, V, step, end_id, max_input_len, total_len;
    const int*   draft;  // [R - 1]
    int*         output_ids;
    const int*   stop_words;  // [2, stop_len] or NULL
    int          stop_len;
    uint8_t*     finished;
    int*         seq_len;
    float*       cum_log_probs;     // [1] or NULL
    float*       output_log_probs;  // [total_len - max_input_len] or NULL
    DecodeState* state;
    int*         h_flags;
    int *        emitted, *accepted, *tokens;
    float*       ws;
};
size_t verify_close_workspace_bytes();
void   launch_verify_close(const VerifyCloseParams& p, hipStream_t s);
// The tail of a verify pass of a TOP-K SAMPLED request (the stand-alone ftcf_verify_sample of include/ftcf.h is the contract), in
// three launches: k_verify_topk_slices (the first half of k_topk_decode per row: VERIFY_ACCEPT_SLICES slices in registers, scaled by
// the temperature on load, their k best and {max, sum of exponentials}), k_verify_pick (a workgroup per row merges the slices'
// candidate sets as k_topk_decode's finishing workgroup does and draws with uniform number draw_counter[0] + row: topk_draw_at)
// and k_verify_sample_close (the stages of k_verify_close on the sampled tokens, then draw_counter[0] += emitted).  Row i is
// reached only behind i accepted rows, i.e. behind exactly i draws: the tokens are the plain sampled run's for the same seed.
// c: as for launch_verify_close (c.ws is not used); 1 <= top_k <= 64, V <= 131072.  ws: verify_sample_workspace_bytes().
struct VerifySampleParams {
    VerifyCloseParams c;
    int               top_k;
    float             top_p_topk;         // the p of the top-k layer (1: all of the k)
    int               apply_temperature;  // logits are read as logit * (1.0f / (temperature + 1e-6f)), k_decode_prep's expression
    float             temperature;
    uint64_t          random_seed;
    uint64_t*         draw_counter;  // device [1]
    float*            ws;
};
constexpr int VERIFY_SAMPLE_MAX_K = 64;
constexpr int VERIFY_SAMPLE_MAX_V = VERIFY_ACCEPT_SLICES * 256 * 16;
size_t verify_sample_workspace_bytes();
void   launch_verify_sample(const VerifySampleParams& p, hipStream_t s);

// ---- per-request logit processors over logits [B, V] fp32, in place, BEFORE the dynamic decode : kernels_logits.hip ----
// (include/ftcf.h ftcf_logit_process_args is the contract; the fields are its fields.)  A row is processed when it is enabled
// (row_on NULL: every row), not finished and has at least one option set; every other row keeps its bits.
struct LogitProcessParams {
    float*          logits;  // [B, V]
    int             B, V, end_id;
    const uint8_t*  finished;  // [B] or NULL
    const uint8_t*  row_on;    // [B] or NULL
    // token t of row b: hist[t * stride_t + b * stride_b], t in [0, hist_len[b] + hist_len_add); generated from gen_start[b] on
    const int*      hist;
    long long       stride_t, stride_b;
    const int*      hist_len;
    const int*      gen_start;
    int             hist_len_add;
    const float*    presence;  // [B] or NULL
    const float*    frequency;
    const int*      min_new;   // [B] or NULL
    const int*      bias_ids;  // [B, bias_stride]
    const float*    bias_values;
    const int*      n_bias;    // [B] or NULL
    int             bias_stride;
    const int*      bad_words;  // [B, 2, bad_len] or NULL
    int             bad_len;
    const unsigned* mask;     // [B, ceil(V / 32)] or NULL
    const uint8_t*  mask_on;  // [B] or NULL (every row has a mask)
    int             slice;    // logits per workgroup: a multiple of 32 in [32, LOGIT_SLICE_MAX], 0 = LOGIT_SLICE_DEFAULT
};
constexpr int LOGIT_SLICE_MAX = 4096, LOGIT_SLICE_DEFAULT = 2048, LOGIT_BIAS_MAX = 1024, LOGIT_BAD_WORDS_MAX = 256;
void launch_logit_process(const LogitProcessParams& p, hipStream_t s);

}  // namespace ftcf
