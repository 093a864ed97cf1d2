// Host-side engine of the MI355X GPT-NeoX / CodeFuse decoder: the request lifecycle -- begin(), the token loop step() /
// step_speculative(), finish() and create, each a sequence of named stages defined right above it -- and its C ABI
// `ftcf_gptneox_*` (include/ftcf.h).  The stand-alone kernel-level entry points live in capi_kernels.hip.
//
// Host classes mirror the reference's layer split (layers are thin: they own no scratch of their own and never
// reMalloc per call -- one arena is planned per request shape):
//   GptNeoX               <- models/gptneox/GptNeoX.cc:386-1052 (generation loop, LM head, dynamic decode, outputs)
//   GptNeoXContextDecoder <- models/gptneox/GptNeoXContextDecoder.cc:223-512 (prefill)
//   GptNeoXDecoder        <- models/gptneox/GptNeoXDecoder.cc:197-389 (one token through L layers)
//   DecoderSelfAttentionLayer / FfnLayer / DynamicDecodeLayer are the launch helpers used by those.
#include "engine.hip.h"

// GEMM / LM-head dispatch by row count (declared in engine.hip.h): what the engine, the batcher and the stand-alone entry
// points of capi_kernels.hip all launch through
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
void lm_head_dispatch(const f16* A, const f16* W, float* logits, int m, int n, int k, int ldc, hipStream_t s)
{
    if (m <= 4) {
        launch_lm_head(A, W, logits, m, n, k, ldc, s);
    }
    else {
        launch_gemm_nk_f32out(A, W, logits, m, n, k, ldc, s);
    }
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

// ---- begin(): the stages of a request's start, in the order begin() runs them --------------------------------------------

// every argument check on the request, before anything touches the device
void ftcf_gptneox::check_request(const ftcf_forward_args& a) const
{
    const int S = a.max_input_len, K = a.beam_width, batch = a.batch_size;
    FTCF_CHECK_ARG(a.batch_size >= 1 && S >= 1 && a.output_len >= 1, "batch_size, max_input_len and output_len must be >= 1");
    FTCF_CHECK_ARG(a.input_ids && a.input_lengths && a.output_ids && a.sequence_lengths, "NULL tensor");
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
    FTCF_CHECK_ARG(a.speculative_tokens >= 0 && a.speculative_tokens <= VERIFY_MAX_ROWS - 1, "speculative_tokens must be in [0, 15]");
    FTCF_CHECK_ARG(a.speculative_ngram >= 0 && a.speculative_ngram <= 8, "speculative_ngram must be in [0, 8]");
}

// The ranks' exchange window (collective: every rank sees the same request shape), sized for the persistent kernel's decode
// exchange and, behind its granules, the message buffers of the RCCL-free prompt-phase all-reduce (k_window_allreduce).
void ftcf_gptneox::ensure_exchange_window(int B, int K)
{
    const int  tpn     = cfg.tensor_para_size;
    const bool want_tp = tpn > 1 && persist_eligible(B, K, false);
    // (read once per process)
    static const int winar_on = env_int("FTCF_TP_WINAR", 1);
    static const int winar_mb = env_int("FTCF_TP_WINAR_MB", 16);
    const bool want_ar = tpn > 1 && tpn <= 8 && winar_on && !fp32 && cfg.comm && !cfg.comm->local && !cfg.comm->ar_failed;
    if (!want_tp && !want_ar) {
        return;
    }
    // room for two rows: [tp][2 * H / 2] granules (two planes by layer parity: persist_device.hip.h ps_tp_exchange), then 16
    // flags, then four message buffers
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

// Behind plan(): the granule tags of the persistent kernel's exchange repeat from request to request, so every rank's window is
// zeroed between two barriers -- nobody is still writing into it from the previous request, nobody writes before it is clean
void ftcf_gptneox::clear_exchange_window()
{
    const int tpn = cfg.tensor_para_size;
    if (tpn == 1 || !pplan.ok) {
        return;
    }
    comm_barrier(cfg.comm, stream, tp_scratch);
    // (this rank's own window: with fake peers it is the only one, whatever the rank)
    FTCF_HIP_CHECK(hipMemsetAsync(cfg.comm->win[fake_peers() ? 0 : cfg.tensor_para_rank], 0, (size_t)2 * tpn * H * 8, stream));
    comm_barrier(cfg.comm, stream, tp_scratch);
}

// Speculative greedy decoding: a hint that cannot change a result -- a request it does not cover runs as
// it always has, and the stats say so.  No side effect but ONE host synchronisation, issued only when everything else holds.
bool ftcf_gptneox::speculation_wanted(const ftcf_forward_args& a, int total)
{
    // what the engine's scope decides (ftcf_gptneox_set_speculative_scope), here and nowhere else: at scope 0 a request with any
    // of these runs unspeculated; at scope 1 it speculates and the pass's tail (k_verify_close, which closes every greedy pass at
    // either scope) serves them.  optional_last_tokens masks the first generated step only, which never drafts.  A temperature
    // leaves the arg max alone but not the soft-max: with a log-probability output it still excludes the request.
    // A top-k sampled request (ftcf_gptneox_set_speculative_sampling): top_k in 2..64, a top_p next to it being the p of the top-k
    // layer, over a vocabulary the sampled tail holds in registers.  Its tail applies the temperature itself, so a temperature
    // excludes nothing there.
    const bool sampled = spec_sampling == 1 && a.n_top_k > 0 && a.top_k && a.top_k[0] >= 2 && a.top_k[0] <= VERIFY_SAMPLE_MAX_K
                         && V <= VERIFY_SAMPLE_MAX_V;
    const bool log_probs = a.return_cum_log_probs || a.output_log_probs;
    bool       scoped    = !a.callback && !log_probs && !a.stop_words_list && !a.optional_last_tokens;
    if (spec_scope == 1) {
        scoped = true;
        for (int i = 0; log_probs && !sampled && i < a.n_temperature; i++) {
            scoped &= a.temperature && a.temperature[i] == 1.f;
        }
    }
    const bool eligible =
        a.speculative_tokens > 0 && a.batch_size == 1 && a.beam_width == 1 && !fp32 && cfg.tensor_para_size == 1 && cfg.use_gptj_residual
        && prefill_begin == 0 && verify_attention_supported(nhl, dh, total) && H % 64 == 0 && hl % 64 == 0 && il % 64 == 0 && scoped
        && a.top_logprobs == 0 && !a.debug_logits && a.n_min_length == 0 && (a.n_top_k == 0 || (a.top_k && a.top_k[0] <= 1) || sampled)
        && (a.n_top_p == 0 || (a.top_p && (a.top_p[0] == 0.f || sampled)))
        && (a.n_repetition_penalty == 0 || (a.repetition_penalty && a.repetition_penalty[0] == 1.f)) && !logits_hook;
    if (!eligible) {
        return false;
    }
    // (the token history must be dense from position 0: a prompt as long as its row)
    int h_len = 0;
    FTCF_HIP_CHECK(hipMemcpyAsync(&h_len, a.input_lengths, sizeof(int), hipMemcpyDeviceToHost, stream));
    comm_stream_sync(cfg.comm, stream);
    return h_len == a.max_input_len;
}

// runtime args: routing of TopKSamplingLayer.cu:27-77 / TopPSamplingLayer.cu:30-110, and their device copies
SamplingRouting ftcf_gptneox::upload_sampling_args(const ftcf_forward_args& a)
{
    const int batch = a.batch_size;
    auto top_k = broadcast_arg<int>(a.top_k, a.n_top_k, batch, 0, "top_k");
    auto top_p = broadcast_arg<float>(a.top_p, a.n_top_p, batch, 0.f, "top_p");
    auto temp  = broadcast_arg<float>(a.temperature, a.n_temperature, batch, 1.f, "temperature");
    auto rep   = broadcast_arg<float>(a.repetition_penalty, a.n_repetition_penalty, batch, 1.f, "repetition_penalty");
    auto seed  = broadcast_arg<uint64_t>(a.random_seed, a.n_random_seed, batch, 0, "random_seed");
    auto minl  = broadcast_arg<int>(a.min_length, a.n_min_length, batch, 0, "min_length");
    auto divr  = broadcast_arg<float>(a.beam_search_diversity_rate, a.n_beam_search_diversity_rate, batch, 0.f,
                                      "beam_search_diversity_rate");
    auto lenp  = broadcast_arg<float>(a.len_penalty, a.n_len_penalty, batch, 0.f, "len_penalty");
    SamplingRouting route = route_sampling_args(top_k, top_p, temp, rep, minl, a.n_repetition_penalty > 0);
    FTCF_HIP_CHECK(hipMemcpyAsync(d_top_k, route.k_eff.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_p_topk, route.p_topk.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_p_topp, route.p_topp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_temp, temp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_rep, rep.data(), batch * 4, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_seed, seed.data(), batch * 8, hipMemcpyHostToDevice, stream));
    FTCF_HIP_CHECK(hipMemcpyAsync(d_min_length, minl.data(), batch * 4, hipMemcpyHostToDevice, stream));
    if (a.beam_width > 1) {
        FTCF_HIP_CHECK(hipMemcpyAsync(d_div, divr.data(), batch * 4, hipMemcpyHostToDevice, stream));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_lenpen, lenp.data(), batch * 4, hipMemcpyHostToDevice, stream));
    }
    comm_stream_sync(cfg.comm, stream);  // the host vectors die at scope exit
    return route;
}

// granules, tags and tickets that repeat from request to request: zero before the first launch that reads them
void ftcf_gptneox::reset_workspaces(int B)
{
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
}

// what the persistent kernels (one / two rows, 3..16 rows) read besides the arena: the layer table, zeroed hand-off words and,
// for the one- / two-row kernel, the run / tile tables of this plan
void ftcf_gptneox::upload_layer_tables(int B, int s_max)
{
    if (!pplan.ok && !rplan.ok) {
        return;
    }
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
void ftcf_gptneox::tile_beam_inputs(const ftcf_forward_args& a)
{
    const int K = a.beam_width, batch = a.batch_size, B = batch * K, S = a.max_input_len, total = S + a.output_len;
    launch_tile_inputs(tiled_ids, tiled_len, a.input_ids, a.input_lengths, batch, K, S, stream);
    FTCF_HIP_CHECK(hipMemsetAsync(cache_indir, 0, (size_t)2 * B * total * 4, stream));
    FTCF_HIP_CHECK(hipMemsetAsync(parent_ids, 0, (size_t)total * B * 4, stream));
    FTCF_HIP_CHECK(hipMemsetAsync(step_log_probs, 0, (size_t)total * B * 4, stream));  // (rows no step writes hold 0)
}

// context_log_probs (ParallelGpt.cc:403-470): px holds the last layer's output of every prompt row, once per request (beams
// included, tensor parallel ranks alike: the head is replicated): the final LayerNorm, then the fused LM head -> log-prob kernel
void ftcf_gptneox::score_prompt(const ftcf_forward_args& a)
{
    const int batch = a.batch_size, S = a.max_input_len;
    if (!a.context_log_probs) {
        return;
    }
    if (S > 1) {
        launch_layernorm(px, final_g, final_b, pnrm, batch * S, H, 1e-5f, true, stream);
        launch_context_log_probs(a.context_log_probs, pnrm, lm_head, a.input_ids, a.input_lengths, ctx_tgt, ctx_lp, batch, S, V, H,
                                 stream);
    }
    else {
        FTCF_HIP_CHECK(hipMemsetAsync(a.context_log_probs, 0, (size_t)batch * S * 4, stream));
    }
}

// top_logprobs of the token loop: room for `pairs` {id, log-probability} pairs, filled with the pattern that steps after a row
// finished keep
void ftcf_gptneox::ensure_top_logprob_buffers(size_t pairs)
{
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

// what the dynamic-decode kernels read for this request (in_len: the input lengths per ROW, tiled for beams)
SamplingParams ftcf_gptneox::session_sampling_params(const ftcf_forward_args& a, const SamplingRouting& route, const int* in_len) const
{
    const int K = a.beam_width, S = a.max_input_len;
    SamplingParams sp{};
    sp.logits = logits;
    sp.B = a.batch_size * K;
    sp.V = V;
    sp.max_input_len = S;
    sp.total_len = S + a.output_len;
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
    return sp;
}

// ... and the beam-search kernels (all zero without beams)
BeamParams ftcf_gptneox::session_beam_params(const ftcf_forward_args& a, const SamplingRouting& route, const int* in_len) const
{
    const int  K = a.beam_width, S = a.max_input_len;
    BeamParams bp{};
    if (K > 1) {
        bp.logits = logits;
        bp.B = a.batch_size;
        bp.K = K;
        bp.V = V;
        bp.max_input_len = S;
        bp.total_len = S + a.output_len;
        bp.end_id = cfg.end_id;
        bp.s_max = S + a.output_len;
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
        bp.step_log_probs = step_log_probs;
        bp.cache_indir = cache_indir;
        bp.state = state;
        bp.ws = beam_ws;
    }
    return bp;
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
    check_request(a);
    const int K = a.beam_width, batch = a.batch_size, B = batch * K;  // B: rows
    const int S = a.max_input_len, out_len = a.output_len;
    const int total = S + out_len;  // max_output_seq_len == max_seq_len == max_cache_seq_len (GptNeoX.cc:520-523)
    const int s_max = total;
    FTCF_HIP_CHECK(hipSetDevice(cfg.device));
    beam_request_done = false;
    abandon_session();  // (a request left open -- begin / step without finish, or a step that threw -- must not leak its graph)
    stats.window_allreduces = 0;
    // everything the caller enqueued on its stream (input tensors) happens-before the engine's work
    FTCF_HIP_CHECK(hipEventRecord(ev_user, user_stream));
    FTCF_HIP_CHECK(hipStreamWaitEvent(stream, ev_user, 0));
    ensure_exchange_window(B, K);
    spec_plan = speculation_wanted(a, total);  // (plan() carves a verify pass's buffers for a request that speculates)
    plan(B, S, total, K);
    clear_exchange_window();
    const SamplingRouting route = upload_sampling_args(a);

    hipEvent_t e0 = get_event(), e1 = get_event();  // [e0, e1]: what the stats call the prompt phase
    FTCF_HIP_CHECK(hipEventRecord(e0, stream));
    reset_workspaces(B);
    upload_layer_tables(B, s_max);
    if (K > 1) {
        tile_beam_inputs(a);
    }
    // the inputs per ROW
    const int* in_ids = K > 1 ? tiled_ids : a.input_ids;
    const int* in_len = K > 1 ? tiled_len : a.input_lengths;
    launch_decode_init(finished, seq_len, cum, pad_count, masked, draws, in_len, state, B, S, s_max, stream, K);
    if (B <= 2 && !fp32) {  // the tagged partials of k_lm_head_greedy: a tag is the step, and steps repeat from request to request
        FTCF_HIP_CHECK(hipMemsetAsync(samp_ws, 0, lm_head_greedy_partial_bytes(B), stream));
    }
    // what the stats will say of THIS request's overlapped forms: the prompt phase below and the token loop set them
    ov_ran = ov_eligible = false;
    dv_ran = dv_eligible = false;
    prompt_phase(a, in_ids, in_len);
    score_prompt(a);
    if (a.output_log_probs) {
        FTCF_HIP_CHECK(hipMemsetAsync(olp, 0, (size_t)out_len * B * 4, stream));  // (steps after a row finished hold 0)
    }
    if (a.top_logprobs > 0) {
        ensure_top_logprob_buffers((size_t)out_len * B * a.top_logprobs);
    }
    FTCF_HIP_CHECK(hipEventRecord(e1, stream));

    ses.open(a, session_sampling_params(a, route, in_len), session_beam_params(a, route, in_len), e0, e1, spec_plan);
    if (spec_plan && route.k_eff[0] >= 2) {  // (speculation_wanted admitted it: the switch is on, 2 <= top_k <= 64)
        ses.spec_sampled    = true;
        ses.spec_top_k      = route.k_eff[0];
        ses.spec_p_topk     = route.p_topk[0];
        ses.spec_apply_temp = route.apply_temperature;
        ses.spec_temp       = a.n_temperature > 0 ? a.temperature[0] : 1.f;
        ses.spec_seed       = a.n_random_seed > 0 ? a.random_seed[0] : 0;
    }
    stats.decode_ms = 0.f;
}

// ---- the token loop (GptNeoX.cc:776-1048): what one iteration enqueues on `stream` (and the side stream) -----------------------

// the step's input row(s) and the L layers (GptNeoX.cc:776-850); not for the first step behind a prompt phase, whose input the
// prompt phase has left in x
void ftcf_gptneox::enqueue_decoder(bool with_decoder)
{
    const int B = ses.B, s_max = ses.s_max;
    if (!with_decoder) {
        return;
    }
    if (fp32) {
        launch32_step_prologue(F(x), F(wte), step_ids, &state->step, rot_table, pad_count, B, H, cfg.rotary_embedding_dim,
                               stream);
        decoder32(B, s_max);
        return;
    }
    // (an all-greedy batch: the previous token's k_greedy_decode has written this token's embedding row and rotary
    // table already -- unless this is the request's first dynamic-decode step, a one-token prompt)
    if (!(ses.K == 1 && ses.sp.next_x && ses.steps > 0 && dynamic_decode_is_fused(ses.sp, true))) {
        launch_step_prologue(x, wte, step_ids, &state->step, rot_table, pad_count, B, H, cfg.rotary_embedding_dim,
                             stream, &state->all_finished);
    }
    decoder(B, s_max);
}

// final LayerNorm, LM head (vocabulary-split under tensor parallelism), the debug tap and the logits hook; returns whether the
// LM head launch closed the step itself (k_lm_head_greedy): nothing is launched behind it then
bool ftcf_gptneox::enqueue_lm_head()
{
    const ftcf_forward_args& a = ses.a;
    const int B = ses.B, S = ses.S;
    const int tp = cfg.tensor_para_size;
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
    if (a.debug_logits) {  // (here, not behind the step: the decode kernels modify the logits in place)
        FTCF_HIP_CHECK(hipMemcpyAsync(a.debug_logits + (size_t)(ses.next_step - S) * B * V, logits,
                                      (size_t)B * V * 4, hipMemcpyDeviceToDevice, stream));
    }
    if (logits_hook && ses.K == 1) {
        logits_hook(logits, B, stream);
    }
    return lm_greedy;
}

void ftcf_gptneox::enqueue_step(bool with_decoder)
{
    enqueue_decoder(with_decoder);
    const bool closed = enqueue_lm_head();
    if (ses.K > 1) {
        dynamic_decode_layer.forward(ses.bp, ses.sp, stream);
    }
    else if (!closed) {
        dynamic_decode_layer.forward(ses.sp, stream);
    }
}

// `tokens` regular decode steps captured into one executable graph (all pointers are fixed for the session, the step counter lives
// on the device): a replay has no per-kernel host launch cost, cross-stream fork / join become edges
hipGraphExec_t ftcf_gptneox::capture_steps(int tokens)
{
    hipGraph_t     g  = nullptr;
    hipGraphExec_t ge = nullptr;
    FTCF_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
        for (int t = 0; t < tokens; t++) {
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
    return ge;
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
    DecodeStopwatch  watch(*this);
    // Several tokens per graph launch (FTCF_GRAPH_TOKENS, default 8): a graph launch costs ~14 us of GPU idle time between
    // two tokens (profiles/r03_notes.md section 6), and every kernel of a persistent-path token returns at once when the
    // device-side "every row has finished" flag is set, so the tokens of a graph behind the request's last one cost a few
    // microseconds each, not a decoder pass.  (Read per call, not once per process: the tests switch it between engines.)
    const int graph_tokens = std::max(1, std::min(64, env_int("FTCF_GRAPH_TOKENS", 8)));

    // whether a step is replayed from a captured graph ...
    // (with tensor parallelism the step contains RCCL collectives or the exchange windows' spins: not captured -- a capture
    // of the RCCL form aborted inside this image's HIP runtime, profiles/r05_notes.md)
    auto graph_eligible = [&](bool with_decoder) {
        return use_graph && with_decoder && !profiling && tp == 1 && !a.debug_logits && !logits_hook;
    };
    // ... and graph_tokens of them from one: persistent decode path, no streaming callback, one GPU, that many tokens still to go
    auto multi_token = [&](int step, int done) {
        return graph_tokens > 1 && pplan.ok && ses.K == 1 && !a.callback && tp == 1 && max_steps - done >= graph_tokens
               && total - step >= graph_tokens;
    };
    // The reference synchronises once per token (stop_criteria_kernels.cu:149-156).  Without a streaming callback nothing on
    // the host needs token t before token t+1 is enqueued, so the replayed graph of the next token(s) is launched first and the
    // host only waits for the PREVIOUS launch's event: the GPU never idles for the host round trip (~25 us per token).
    // `finished` is sticky on the device and the launches behind the last token return at once; the host's counters are set
    // back to the device's when it learns of the end (follow_device_counters).
    // (tp > 1: every rank must leave the loop at the SAME token -> synchronous)
    auto pipelined = [&](bool graph_ok) { return graph_ok && !a.callback && tp == 1; };
    bool lagging  = false;  // the host has not yet seen the flags of the token launched last
    int  lag_slot = 0;      // launches of the pipelined loop so far (two events alternate)
    auto wait_for_previous_launch = [&] {
        hipEvent_t& ev = tok_ev[lag_slot & 1];
        if (!ev) {
            FTCF_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        FTCF_HIP_CHECK(hipEventRecord(ev, stream));
        if (lagging) {
            comm_event_sync(cfg.comm, tok_ev[(lag_slot - 1) & 1]);
            ses.all_finished = h_flags[FLAG_ALL_FINISHED] != 0;
        }
        lag_slot++;
        lagging = true;
    };
    // the streaming callback (pybind_callback_utils.cc:22-103): last token of every row; a row that did not advance reports end_id
    auto report_tokens = [&](int step) {
        FTCF_HIP_CHECK(hipMemcpy(h_tokens.data(), step_ids + (size_t)step * B, (size_t)B * 4, hipMemcpyDeviceToHost));
        FTCF_HIP_CHECK(hipMemcpy(h_seq.data(), seq_len, (size_t)B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++) {
            h_idx[b] = h_seq[b];
            if (h_seq[b] != step) {
                h_tokens[b] = cfg.end_id;
            }
        }
        a.callback(h_tokens.data(), h_idx.data(), ses.batch, ses.K, a.callback_user);
    };
    // launches behind the token that finished the last row did nothing on the device (every kernel of a token returns at
    // once on the flag, k_decode_finish included: the device's step counter stopped): the host's counters follow the
    // device's, so that `steps_done` is the reference's loop count (GptNeoX.cc:776-1048 leaves its loop at that token)
    auto follow_device_counters = [&](int& done) {
        const int over = ses.next_step - (h_flags[FLAG_LAST_STEP] + 1);
        if (ses.all_finished && ses.K == 1 && over > 0) {
            ses.next_step -= over;
            ses.steps -= over;
            done -= over;
        }
    };

    int done = 0;
    while (done < max_steps && ses.next_step < total && !ses.all_finished) {
        const int  step         = ses.next_step;
        const bool with_decoder = !(S > 1 && step == S);
        const bool graph_ok     = graph_eligible(with_decoder);
        const bool multi        = graph_ok && multi_token(step, done);
        const int  launched     = multi ? graph_tokens : 1;
        if (graph_ok) {
            hipGraphExec_t& ge = multi ? ses.graph_exec_n : ses.graph_exec;
            if (!ge) {
                ge = capture_steps(launched);
            }
            FTCF_HIP_CHECK(hipGraphLaunch(ge, stream));
        }
        else {
            enqueue_step(with_decoder);
        }
        ses.steps += launched;
        ses.next_step += launched;
        done += launched;
        if (pipelined(graph_ok)) {
            wait_for_previous_launch();
            continue;
        }
        lagging = false;
        comm_stream_sync(cfg.comm, stream);
        ses.all_finished = h_flags[FLAG_ALL_FINISHED] != 0;
        if (a.callback && step + 1 < total && cfg.tensor_para_rank == 0) {
            report_tokens(step);
        }
    }
    watch.stop("the prefill");
    if (lagging) {
        ses.all_finished = h_flags[FLAG_ALL_FINISHED] != 0;
    }
    follow_device_counters(done);
    watch.add_to_stats();
    return done;
}

// One verify pass: the token of position step - 1 and `drafts` drafted tokens as R = drafts + 1 rows of the
// one sequence through the batched decode layers in their grouped form (ParallelResidualDecoder, layers.hip.h: the burst GEMM pairs
// [QKV, FFN1] -> attention -> [out-proj, FFN2], residual + both LayerNorms in one pass) with the verify attention, then the final
// LayerNorm, the LM head on R rows and the acceptance kernels, which close the step as the greedy kernels do.  The K / V rows of
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
    // One close for every pass.  Stop words, log-probabilities and the callback's tokens are the tail's business; at scope 0
    // speculation_wanted admitted the request only without them (and without optional_last_tokens), so these fields are NULL there
    // -- the condition under which the close is the bare greedy acceptance: arg max, accepted prefix, cut after the first end_id.
    VerifySampleParams q{};
    VerifyCloseParams& cp = q.c;
    cp.logits           = vlogits;
    cp.R                = R;
    cp.V                = V;
    cp.step             = st;
    cp.end_id           = cfg.end_id;
    cp.max_input_len    = ses.S;
    cp.total_len        = ses.total;
    cp.draft            = spec_draft;
    cp.output_ids       = step_ids;
    cp.stop_words       = ses.sp.stop_words;
    cp.stop_len         = ses.sp.stop_len;
    cp.finished         = finished;
    cp.seq_len          = seq_len;
    cp.cum_log_probs    = ses.sp.return_cum_log_probs ? cum : nullptr;
    cp.output_log_probs = ses.sp.return_cum_log_probs ? ses.sp.output_log_probs : nullptr;
    cp.state            = state;
    cp.h_flags          = h_flags;
    cp.ws               = spec_close_ws;
    if (ses.spec_sampled) {  // every row sampled with the draw the plain step of its position would take (either scope)
        q.top_k             = ses.spec_top_k;
        q.top_p_topk        = ses.spec_p_topk;
        q.apply_temperature = ses.spec_apply_temp;
        q.temperature       = ses.spec_temp;
        q.random_seed       = ses.spec_seed;
        q.draw_counter      = draws;
        q.ws                = spec_sample_ws;
        launch_verify_sample(q, stream);
    }
    else {
        launch_verify_close(cp, stream);
    }
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
    const int       S = ses.S, total = ses.total;
    DecodeStopwatch watch(*this);
    // The streaming callback of a request that speculates (scope 1), once per emitted token in order, with what the plain loop's
    // report_tokens(step) passes for that step: the token and the sequence length behind it (a row that did not advance reports
    // end_id), not for the request's last position.  A pass left both in the pinned flags; a plain step's are copied as there.
    auto report_tokens = [&](int st, int emitted, bool pass) {
        for (int i = 0; i < emitted && st + i + 1 < total; i++) {
            int tok = 0, idx = 0;
            if (pass) {
                tok = h_flags[FLAG_SPEC_TOKENS + i];
                idx = h_flags[FLAG_SPEC_SEQ_LEN + i];
            }
            else {
                FTCF_HIP_CHECK(hipMemcpy(&tok, step_ids + st, sizeof(int), hipMemcpyDeviceToHost));
                FTCF_HIP_CHECK(hipMemcpy(&idx, seq_len, sizeof(int), hipMemcpyDeviceToHost));
            }
            if (idx != st + i) {
                tok = cfg.end_id;
            }
            a.callback(&tok, &idx, ses.batch, ses.K, a.callback_user);
        }
    };
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
                ses.graph_exec = capture_steps(1);
            }
            FTCF_HIP_CHECK(hipGraphLaunch(ses.graph_exec, stream));
        }
        else {
            enqueue_step(with_decoder);
        }
        // the next step's drafts: the caller's (draft_ids from the generated index of the device's step on) or the n-gram lookup
        // over the tokens so far
        launch_ngram_draft(step_ids, 0, &state->step, ses.spec_K, ses.spec_N, a.draft_ids, S, total - S, spec_draft, spec_ndraft,
                           h_flags + FLAG_SPEC_NEXT_DRAFTS, &state->all_finished, stream);
        comm_stream_sync(cfg.comm, stream);
        const int emitted = nd > 0 ? h_flags[FLAG_SPEC_EMITTED] : 1;
        if (nd > 0) {
            ses.spec_steps++;
            ses.spec_drafted += nd;
            ses.spec_accepted += h_flags[FLAG_SPEC_ACCEPTED];
        }
        ses.steps += emitted;
        ses.next_step += emitted;
        done += emitted;
        ses.all_finished = h_flags[FLAG_ALL_FINISHED] != 0;
        ses.spec_nd      = h_flags[FLAG_SPEC_NEXT_DRAFTS];
        if (a.callback && cfg.tensor_para_rank == 0) {
            report_tokens(st, emitted, nd > 0);
        }
    }
    watch.stop("the token loop");
    watch.add_to_stats();
    return done;
}

// ---- finish(): the stages of a request's end, in the order finish() runs them ------------------------------------------------

// setOutputTensors (GptNeoX.cc:1090-1181)
void ftcf_gptneox::write_outputs()
{
    const ftcf_forward_args& a = ses.a;
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
}

// the sticky give-up words of the kernels that ran, copied asynchronously: `w` is the CALLER's, valid once the caller has
// synchronised the stream
void ftcf_gptneox::read_error_words(ErrorWords& w)
{
    if (pplan.ok) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&w.ps, ps_err, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    if (smallm_ws) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&w.smallm, reinterpret_cast<char*>(smallm_ws) + smallm_partial, sizeof(int),
                                      hipMemcpyDeviceToHost, stream));
    }
    if (rplan.ok) {
        FTCF_HIP_CHECK(hipMemcpyAsync(&w.rows, rows_ws, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
}

// the auto modes' timed trials of the overlapped prompt phase and the overlapped decode step (every rank keeps the slowest rank's
// time: one comm_max each, in this order on every rank), and what the stats say of both
void ftcf_gptneox::close_overlap_trials(float prefill_ms)
{
    if (ov_eligible && ov_trial < 2) {
        const int us   = comm_max(cfg.comm, (int)(prefill_ms * 1000.f), stream, tp_scratch);
        ov_ms[ov_trial] = us * 1e-3f;
        ov_trial++;
        if (ov_trial == 2) {
            FT_LOG_INFO(cfg.device, "prompt-phase all-reduce overlap (auto): plain %.2f ms, overlapped %.2f ms -> %s", ov_ms[0], ov_ms[1],
                        ov_ms[1] < ov_ms[0] ? "overlapped from now on" : "plain from now on");
        }
    }
    if (dv_eligible && dv_trial < 2 && ses.steps > 0) {  // (engine.hip.h decoder_overlapped)
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
}

// FTCF_PERSIST_TS=<file>: the in-kernel stamps of the last token, [NB][L][128] words behind a header
void ftcf_gptneox::dump_timestamps(int NB, const long long* ts)
{
    std::vector<long long> h((size_t)NB * L * 128);
    FTCF_HIP_CHECK(hipMemcpy(h.data(), ts, h.size() * 8, hipMemcpyDeviceToHost));
    if (FILE* f = fopen(ps_ts_file.c_str(), "wb")) {
        const int hdr[4] = {NB, L, 8, 16};
        fwrite(hdr, 4, 4, f);
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
    }
}

// Throws for whatever gave up during the request (bounded waits that report through sticky words instead of hanging the GPU), the
// exchange-window all-reduce first; what it switches off tells forward() how to replay the request.
void ftcf_gptneox::raise_give_ups(ErrorWords w)
{
    const int tpn = cfg.tensor_para_size;
    // test hook (FTCF_PERSIST_FAIL_ONCE=1): pretend the request's persistent kernel -- the one- / two-row or the rows kernel, a
    // request plans one of them at most -- gave up once
    if ((pplan.ok || rplan.ok) && persist_fail_once) {
        persist_fail_once         = 0;
        (pplan.ok ? w.ps : w.rows) = 99;
    }
    if (pplan.ok && tpn > 1) {
        w.ps = comm_max(cfg.comm, w.ps, stream, tp_scratch);  // every rank learns of any rank's failure
    }
    if (tpn > 1 && cfg.comm && cfg.comm->ar_seq > 0 && !cfg.comm->ar_failed) {
        // the window all-reduce's sticky give-up word (a peer that never arrived: its bounded waits ran out), agreed on
        int ar_err = 0;
        FTCF_HIP_CHECK(hipMemcpy(&ar_err, cfg.comm->ar_sync + 2, sizeof(int), hipMemcpyDeviceToHost));
        ar_err = comm_max(cfg.comm, ar_err, stream, tp_scratch);
        if (ar_err != 0) {
            cfg.comm->ar_failed = true;  // this communicator keeps RCCL (or the emulation) for the prompt phase from now on
            winar_failed        = true;
            throw Error(-2, "exchange-window all-reduce gave up waiting for a peer (its kernel was not running next to this one)");
        }
    }
    if (h_flags[FLAG_LM_GREEDY_GAVE_UP] != 0) {  // k_lm_head_greedy's finishing workgroup never saw some workgroup's partial (cannot happen: bounded all the same)
        h_flags[FLAG_LM_GREEDY_GAVE_UP] = 0;
        throw Error(-2, "LM head + greedy decode: the finishing workgroup gave up waiting for the partials of the launch");
    }
    if (w.smallm != 0) {
        throw Error(-2, "batched decode GEMM: a split-K reducer gave up waiting for its sibling workgroups' partial sums");
    }
    // the kernel that gave up is switched off (`knob`): whoever drives begin / step / finish, the next request (and the replay of
    // this one) is planned off it
    auto kernel_gave_up = [&](const char* name, int code, int& knob) {
        persist_failed = true;
        knob           = 0;
        throw Error(-2, std::string(name) + " decode kernel gave up waiting for a hand-off (code " + std::to_string(code)
                            + "): not every workgroup was resident");
    };
    if (w.rows != 0) {
        kernel_gave_up("rows", w.rows, rows);
    }
    if (w.ps != 0) {
        kernel_gave_up("persistent", w.ps, persist);
    }
}

void ftcf_gptneox::finish()
{
    Range r("ftcf.finish");
    FTCF_CHECK_ARG(ses.active, "no request in flight");
    write_outputs();
    ErrorWords err;  // (filled by the stream: read behind the synchronisation below)
    read_error_words(err);
    comm_stream_sync(cfg.comm, stream);
    float ms = 0.f;
    FTCF_HIP_CHECK(hipEventElapsedTime(&ms, ses.e0, ses.e1));
    stats.prefill_ms   = ms;
    stats.decode_steps = ses.steps;
    stats.spec_active   = ses.spec ? 1 : 0;
    stats.spec_steps    = ses.spec_steps;
    stats.spec_drafted  = ses.spec_drafted;
    stats.spec_accepted = ses.spec_accepted;
    close_overlap_trials(ms);
    // the session is closed before anything below may throw
    event_pool.push_back(ses.e0);
    event_pool.push_back(ses.e1);
    ses.e0 = ses.e1 = nullptr;
    ses.active = false;
    beam_request_done = ses.K > 1;
    destroy_graphs();
    drain_events();
    if (pplan.ok && ps_ts) {
        dump_timestamps(pplan.NB, ps_ts);
    }
    if (rplan.ok && rows_ts) {
        dump_timestamps(rplan.NB, rows_ts);
    }
    raise_give_ups(err);
}

// output_log_probs [batch, beam, output_len] of a beam request (GptNeoX.cc:418), behind the request: the step values that
// k_beam_batch recorded, carried along the gather tree's parent chain.  The request's buffers live until the next begin().
void ftcf_gptneox::beam_log_probs(float* log_probs, size_t capacity)
{
    FTCF_CHECK_ARG(log_probs, "NULL argument");
    FTCF_CHECK_ARG(beam_request_done, "beam_log_probs: the last request was not a finished beam-search request");
    FTCF_CHECK_ARG(capacity >= (size_t)ses.B * (ses.total - ses.S), "beam_log_probs: capacity is below batch * beam_width * output_len");
    FTCF_HIP_CHECK(hipSetDevice(cfg.device));
    launch_gather_tree_beam_log_probs(log_probs, step_log_probs, step_ids, parent_ids, seq_len, tiled_len, ses.batch, ses.K, ses.S,
                                      ses.total, cfg.end_id, stream);
    comm_stream_sync(cfg.comm, stream);
}

// ---- create: configuration, streams and events, the weights, the knobs, the pinned flags --------------------------------------

// The layer table from the caller's lists (GptNeoXOp.h:150-175: 12 groups of L tensors, then wte, the final LayerNorm, lm_head).
// int8 kernels and fp32 kernels are read in place; reference-layout [K, N] fp16 kernels are re-tiled once on `stream`.
void ftcf_gptneox::bind_weights(const ftcf_gptneox_weights& w)
{
    if (int8) {
        FTCF_CHECK_ARG(w.n_int8_weights == 4 * L && w.n_scales == 4 * L, "int8 lists must hold 4*L tensors");
    }
    auto W = [&](int g, int l) { return w.weights[(size_t)g * L + l]; };
    // FTCF_FP16_RETILE_IN_PLACE=1: the caller's row-major kernels are OVERWRITTEN with the tiled image (through one
    // bounce buffer) instead of being kept next to a tiled copy -- the engine then holds one copy of the fp16 weights
    // (26 GB instead of 52 GB at 13B); the caller must not read those tensors as [K, N] matrices afterwards
    const bool in_place = env_int("FTCF_FP16_RETILE_IN_PLACE", 0) != 0;
    layers.resize(L);
    for (int l = 0; l < L; l++) {
        LayerWeights& lw = layers[l];
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
        FTCF_CHECK_ARG(cfg.use_gptj_residual || lw.attn_out.bias,
                       "use_gptj_residual == 0 needs the attention output bias (weights[5*L + l])");
        if (int8) {
            lw.qkv.kernel = w.int8_weights[0 * L + l];
            lw.attn_out.kernel = w.int8_weights[1 * L + l];
            lw.ffn1.kernel = w.int8_weights[2 * L + l];
            lw.ffn2.kernel = w.int8_weights[3 * L + l];
            lw.qkv.scale = (const f16*)w.scales[0 * L + l];
            lw.attn_out.scale = (const f16*)w.scales[1 * L + l];
            lw.ffn1.scale = (const f16*)w.scales[2 * L + l];
            lw.ffn2.scale = (const f16*)w.scales[3 * L + l];
            FTCF_CHECK_ARG(lw.qkv.kernel && lw.attn_out.kernel && lw.ffn1.kernel && lw.ffn2.kernel && lw.qkv.scale
                               && lw.attn_out.scale && lw.ffn1.scale && lw.ffn2.scale,
                           "missing int8 kernel / scale tensor");
        }
        else if (fp32) {
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
            for (auto& it : items) {
                const void* src = W(it.g, l);
                FTCF_CHECK_ARG(src != nullptr, "missing fp16 kernel tensor");
                const size_t bytes = it.K * it.N * 2;
                if (in_place) {
                    if (bounce_bytes < bytes) {
                        if (bounce) {
                            FTCF_HIP_CHECK(hipStreamSynchronize(stream));
                            (void)hipFree(bounce);
                        }
                        FTCF_HIP_CHECK(hipMalloc(&bounce, bytes));
                        bounce_bytes = bytes;
                    }
                    launch_fp16_rowmajor_to_tiled((const f16*)src, it.K, it.N, (f16*)bounce, stream);
                    FTCF_HIP_CHECK(hipMemcpyAsync(const_cast<void*>(src), bounce, bytes, hipMemcpyDeviceToDevice, stream));
                    it.d->kernel = src;
                    continue;
                }
                void* dst = nullptr;
                FTCF_HIP_CHECK(hipMalloc(&dst, bytes));
                owned.push_back(dst);
                launch_fp16_rowmajor_to_tiled((const f16*)src, it.K, it.N, (f16*)dst, stream);
                it.d->kernel = dst;
            }
        }
    }
    wte     = (const f16*)w.weights[12 * L];
    final_g = (const f16*)w.weights[12 * L + 1];  // GptNeoXOp.h:172-173: slot 12L+1 = gamma
    final_b = (const f16*)w.weights[12 * L + 2];
    lm_head = (const f16*)w.weights[12 * L + 3];
    FTCF_CHECK_ARG(wte && final_g && final_b && lm_head, "missing embedding / final layernorm / lm_head");
}

// The knobs an engine reads ONCE, when it is created (the members' initialisers are the defaults).  Read at other moments, each
// where it is used: FTCF_DECODE_OVERLAP per request (begin), FTCF_PREFILL_OVERLAP per prompt phase (prefill_overlap_wanted),
// FTCF_GRAPH_TOKENS per step() call, FTCF_TP_WINAR / FTCF_TP_WINAR_MB once per process (ensure_exchange_window),
// FTCF_FP16_RETILE_IN_PLACE by bind_weights.
void ftcf_gptneox::read_env_knobs()
{
    STAGE_MAX_ROWS    = std::max(0, std::min(4, env_int("FTCF_STAGE_MAX_ROWS", STAGE_MAX_ROWS)));
    SMALLM_MAX_ROWS   = std::max(16, std::min(256, env_int("FTCF_SMALLM_MAX_ROWS", SMALLM_MAX_ROWS)));
    persist           = env_int("FTCF_PERSIST", persist);
    rows              = env_int("FTCF_ROWS", rows);
    rows_nb           = env_int("FTCF_ROWS_NB", rows_nb);
    persist_fail_once = env_int("FTCF_PERSIST_FAIL_ONCE", persist_fail_once);
    persist_tp        = env_int("FTCF_TP_PERSIST", persist_tp);
    persist_nb        = env_int("FTCF_PERSIST_NB", persist_nb);
    persist_cs1       = env_int("FTCF_PERSIST_CS1", persist_cs1);
    persist_cs3       = env_int("FTCF_PERSIST_CS3", persist_cs3);
    // 0: P3 as K pieces merged by an owner (the form until round 5), 1: own-group layout wherever the shape divides, 2 (default):
    // where it measured faster
    persist_own       = env_int("FTCF_PERSIST_OWN", persist_own);
    decode_branches   = env_int("FTCF_DECODE_BRANCHES", cfg.tensor_para_size == 1 ? 1 : 0);
    tp_pair_ar        = env_int("FTCF_TP_PAIR_AR", tp_pair_ar) != 0;
    use_graph         = env_int("FTCF_USE_GRAPH", cfg.use_hip_graph != 0) != 0;
    if (const char* m = getenv("FTCF_PERSIST_TS")) {  // (a file name)
        ps_ts_file = m;
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
        // weights still being uploaded / produced on the caller's stream happen-before the re-tiling of bind_weights
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
        e->bind_weights(*w);
        e->k3_q = e->fp32 ? 1 : chunk_pick_q(e->H / 16, (e->hl + e->il) / (e->int8 ? TILE_K_I8 : TILE_K_F16));
        e->read_env_knobs();
        {
            hipDeviceProp_t prop;
            FTCF_HIP_CHECK(hipGetDeviceProperties(&prop, cfg->device));
            e->num_cu = prop.multiProcessorCount;
        }
        if (tp > 1) {
            // scratch word of the communicator helpers (comm_barrier / comm_max / comm_agree): every path of a tensor-parallel
            // engine may reach them (the prompt-phase overlap's trials, the kernels' error words), whatever it planned
            FTCF_HIP_CHECK(hipMalloc((void**)&e->tp_scratch, 256));
            FTCF_HIP_CHECK(hipMemsetAsync(e->tp_scratch, 0, 256, e->stream));
        }
        FTCF_HIP_CHECK(hipHostMalloc((void**)&e->h_flags, FLAG_WORDS * sizeof(int), hipHostMallocDefault));
        e->h_flags[FLAG_ALL_FINISHED] = e->h_flags[FLAG_LAST_STEP] = e->h_flags[FLAG_LM_GREEDY_GAVE_UP] = 0;
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

extern "C" int ftcf_gptneox_beam_log_probs(ftcf_gptneox_t h, float* log_probs, size_t capacity)
{
    return guarded([&] {
        require_device();  // (no engine exists without one)
        FTCF_CHECK_ARG(h, "NULL argument");
        h->beam_log_probs(log_probs, capacity);
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

extern "C" int ftcf_gptneox_set_speculative_scope(ftcf_gptneox_t h, int scope)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h, "NULL argument");
        FTCF_CHECK_ARG(scope == 0 || scope == 1, "speculative scope must be 0 or 1");
        h->spec_scope = scope;
    });
}

extern "C" int ftcf_gptneox_set_speculative_sampling(ftcf_gptneox_t h, int enabled)
{
    return guarded([&] {
        FTCF_CHECK_ARG(h, "NULL argument");
        FTCF_CHECK_ARG(enabled == 0 || enabled == 1, "speculative sampling must be 0 or 1");
        h->spec_sampling = enabled;
    });
}

extern "C" int ftcf_gptneox_destroy(ftcf_gptneox_t h)
{
    return guarded([&] { delete h; });
}
