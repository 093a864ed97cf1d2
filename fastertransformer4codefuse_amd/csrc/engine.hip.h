// The engine behind GptNeoXOp (models/gptneox/GptNeoX.cc:386-1052): the structure every engine translation unit sees --
// engine.hip defines the request lifecycle (begin / step / finish as named stages) and its C ABI `ftcf_gptneox_*`, batcher.hip the
// continuous-batching front end that borrows an engine, capi_kernels.hip the stand-alone kernel-level entry points.  Here: the
// arena plan, the decoder paths and what the units share (GEMM dispatch, the routing of the sampling arguments, the knobs).
#pragma once
#include "comm.hip.h"

// (engine.hip) GEMM / LM-head dispatch shared with the batcher and capi_kernels.hip
void gemm_dispatch(const f16* A, const void* W, const f16* scale, const f16* bias, int act, f16* C, int m, int n, int k, bool int8,
                   hipStream_t s, float* smallm_ws = nullptr, size_t smallm_partial = 0, int num_cu = 256, const int* d_step = nullptr,
                   unsigned* smallm_seq = nullptr, float* tiled_ws = nullptr);
void lm_head_dispatch(const f16* A, const f16* W, float* logits, int m, int n, int k, int ldc, hipStream_t s);

namespace {
// (DenseWeight / LayerWeights and the host-side layer units DecoderSelfAttentionLayer, GptContextAttentionLayer, FfnLayer,
// ParallelResidualDecoder, DynamicDecodeLayer: layers.hip.h)

struct DeviceBuffer {
    void*  ptr = nullptr;
    size_t cap = 0;
    void   reserve(size_t bytes)
    {
        if (bytes > cap) {
            if (ptr) {
                FTCF_HIP_CHECK(hipFree(ptr));
                ptr = nullptr;
                cap = 0;
            }
            FTCF_HIP_CHECK(hipMalloc(&ptr, bytes));
            cap = bytes;
        }
    }
    ~DeviceBuffer()
    {
        if (ptr) {
            (void)hipFree(ptr);
        }
    }
};

// carve helper over one arena
struct Carver {
    char*  base;
    size_t off = 0;
    explicit Carver(void* b): base((char*)b) {}
    template<typename T>
    T* take(size_t n)
    {
        off      = (off + 255) & ~(size_t)255;
        T* p     = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

enum { KIND_LN_GEMV = 0, KIND_SPLITK = 1, KIND_LM_HEAD = 2, KIND_FUSED = 3, KIND_PERSIST = 4, KIND_SMALLM = 5, KIND_COUNT = 6 };

}  // namespace

// a runtime argument given once or per request, as a vector of B (engine.hip begin(), capi_kernels.hip's one-step entries)
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

__global__ void k_transpose_gathered_logits(float* out, const float* in, int tp, int B, int vl, int src);  // (engine.hip)
template<typename T>
__global__ void k_scale_by_tp(T* buf, size_t n, float tp);  // (engine.hip)

struct ftcf_gptneox {
    ftcf_gptneox_config       cfg{};
    int                       H = 0, nhl = 0, hl = 0, il = 0, L = 0, V = 0, vl = 0, dh = 0;
    bool                      int8 = false;
    bool                      fp32 = false;  // FTGptNeoX<float> (GptNeoXOp.cc:56-70): fp32 weights, activations and K/V; general path only
    // `stream` is the engine's own work stream (capturable, unlike the legacy null stream torch usually hands over);
    // it is ordered after `user_stream` at begin() and drained before forward()/finish() return
    hipStream_t               stream = nullptr, user_stream = nullptr;
    // second stream of the batched decode layer: [QKV -> MMHA -> out-proj] on `stream`, [FFN1 -> FFN2] here (fork / join by
    // events; under capture the branch becomes a parallel branch of the token's hipGraph)
    hipStream_t               side = nullptr, side2 = nullptr;  // (side2: the second micro-batch of decoder_overlapped)
    hipEvent_t                ev_fork = nullptr, ev_join = nullptr;
    // batched decode GEMMs: 1 = the attention branch and the FFN branch on two streams, 0 = one stream, the independent GEMMs
    // paired per launch.  Default: two streams at tensor_para_size 1 (the launches are bandwidth bound and fill each other's ramps:
    // 13B int8 bs = 16, 4.31 vs 4.66 ms per step), pairs on a tensor-parallel shard (launch-latency bound: TP 8 shard 1.79 vs 2.36
    // ms, TP 4 2.16 vs 2.62, TP 2 3.13 vs 3.28; `bench.py --fake-tp`).  FTCF_DECODE_BRANCHES overrides.
    int                       decode_branches = 1;
    hipEvent_t                ev_user = nullptr;
    hipEvent_t                tok_ev[2] = {nullptr, nullptr};  // per-token events of the pipelined token loop
    bool                      tp_pair_ar = true;  // batched decode under TP: attn | ffn all-reduced as one message, residual inside the next LN pass
    int                       k1_wpg = 2;  // waves per column group of the QKV launch (0: legacy 4-groups-per-block form)
    std::vector<LayerWeights> layers;
    const f16 *               wte = nullptr, *final_g = nullptr, *final_b = nullptr, *lm_head = nullptr;
    std::vector<void*>        owned;  // tiled fp16 copies (int8_mode == 0)
    void*                     bounce = nullptr;  // FTCF_FP16_RETILE_IN_PLACE: staging of one matrix during create()
    size_t                    bounce_bytes = 0;

    DeviceBuffer arena;
    // decode / state views (valid after plan())
    f16 *x = nullptr, *nrm = nullptr, *nrm2 = nullptr, *qkv = nullptr, *ctx = nullptr, *att = nullptr, *mid = nullptr, *ffn = nullptr;
    f16 *k_cache = nullptr, *v_cache = nullptr;
    f16 *px = nullptr, *pnrm = nullptr, *pnrm2 = nullptr, *pqkv = nullptr, *pctx = nullptr, *patt = nullptr, *pmid = nullptr,
        *pffn = nullptr;
    float *      logits = nullptr, *gather = nullptr, *mmha_ws = nullptr, *rot_table = nullptr;
    unsigned long long* chunk_ws = nullptr;
    int          k3_q = 1;  // chunks per column group of the K3 launch (0: legacy one-workgroup-per-group form)
    void*        samp_ws = nullptr;
    DecodeState* state = nullptr;
    uint8_t *    finished = nullptr, *masked = nullptr;
    int *        seq_len = nullptr, *pad_count = nullptr, *step_ids = nullptr, *d_top_k = nullptr,
        *d_min_length = nullptr;
    float *   olp = nullptr;  // output_log_probs of the token loop, time-major [output_len, B]
    // top_logprobs of the token loop, time-major [output_len, B, N]: allocated by the first request that asks, grown when needed
    int*      tlp_ids = nullptr;
    float*    tlp_values = nullptr;
    size_t    tlp_pairs = 0;
    int*      ctx_tgt = nullptr;  // context_log_probs scratch: targets [B*S] ...
    float*    ctx_lp  = nullptr;  // ... and the log-probability of each hidden row's target [B*S]
    float *   cum = nullptr, *d_p_topk = nullptr, *d_p_topp = nullptr, *d_temp = nullptr, *d_rep = nullptr;
    uint64_t *draws = nullptr, *d_seed = nullptr;
    float*    smallm_ws = nullptr;  // split-K partials + tickets of the batched decode GEMM (5..16 rows)
    float*    tiled_ws  = nullptr;  // split-K partial tiles + tickets of the tiled GEMM at 17..768 rows (short prompt phases)
    size_t    smallm_partial = 0, smallm_region = 0;  // (all of the partial sums; one set of four GEMM regions)
    unsigned  smallm_seq = 0;       // launch counter: part of the granule tag of its in-launch reduction
    // beam search (beam_width K > 1; rows = batch * K everywhere above)
    int *  tiled_ids = nullptr, *tiled_len = nullptr, *parent_ids = nullptr, *cache_indir = nullptr;
    float* step_log_probs = nullptr;  // [total, B] like parent_ids: every beam step's cum - the parent's old cum (beam_log_probs)
    bool   beam_request_done = false;  // a beam request has finished and no begin() has touched its buffers since
    void*  beam_ws = nullptr;
    float *d_div = nullptr, *d_lenpen = nullptr;
    int*      h_flags = nullptr;  // pinned
    int       nsplit = 1;
    // persistent decode layers (kernels_persist.hip): on whenever the shape is eligible (FTCF_PERSIST=0: per-stage launches)
    int                 persist = 1, persist_tp = 1, persist_nb = 0, persist_cs1 = 12, persist_cs3 = 10, persist_own = 2;
    int                 decode_overlap_mode = 0;  // FTCF_DECODE_OVERLAP as read when the last request began: 0 off (default), 1 on, 2 "auto" (timed trial, RCCL ranks)
    int                 num_cu = 0;
    PersistPlan         pplan{};
    PersistLayer*       d_players = nullptr;  // device [L]
    char*               ps_tab = nullptr;     // the plan's run / tile tables, built once per request by a launch over no layers
    bool                ps_tab_ready = false;
    unsigned long long *ps_gq = nullptr, *ps_gm = nullptr, *ps_gc = nullptr, *ps_gx = nullptr, *ps_gp = nullptr,
                       *ps_ga = nullptr;
    size_t              ps_slab_n = 0;
    int*                ps_err = nullptr;
    int*                tp_scratch = nullptr;  // device int for the barrier all-reduce of the tensor-parallel windows
    long long*          ps_ts = nullptr;  // FTCF_PERSIST_TS=<file>: in-kernel stamps of the last token
    // persistent decode layers for 3..16 rows (kernels_rows.hip): on whenever the shape is eligible (FTCF_ROWS=0: general path)
    int                 rows = 1, rows_nb = 0;
    RowsPlan            rplan{};
    char*               rows_ws = nullptr;
    long long*          rows_ts = nullptr;
    std::string         ps_ts_file;

    // speculative greedy decoding: the buffers of a verify pass over <= 16 rows of the one sequence, carved
    // only for a request that speculates (spec_plan, set by begin() before plan())
    bool   spec_plan = false;
    f16 *  vx = nullptr, *vnrm = nullptr, *vnrm2 = nullptr, *vqkv = nullptr, *vctx = nullptr, *vatt = nullptr, *vffn = nullptr, *vmid = nullptr;
    float *vlogits = nullptr, *vrot = nullptr, *spec_aws = nullptr, *spec_gws = nullptr;
    size_t spec_partial = 0;  // split-K partials of the pass's burst GEMMs (a workspace of their own: [partials][tickets])
    int *  spec_draft = nullptr, *spec_ndraft = nullptr;
    float* spec_close_ws = nullptr;  // the slice partials of k_verify_close (every greedy pass, at either scope)
    // which requests may speculate (ftcf_gptneox_set_speculative_scope): 0 the bare greedy request, 1 also one with stop words,
    // log-probabilities, a streaming callback or optional_last_tokens.  Read by begin() alone (speculation_wanted): a request that
    // began is not touched by a later call.
    int    spec_scope = 0;
    // may a top-k sampled request speculate (ftcf_gptneox_set_speculative_sampling)?  Its passes close with the sampled tail
    // (launch_verify_sample) on the request's own draw counter and seed.  Read by begin(), like the scope.
    int    spec_sampling = 0;
    float* spec_sample_ws = nullptr;  // candidates, slice statistics and picks of the sampled tail

    // profiling
    bool               profiling = false;
    ftcf_forward_stats stats{};
    double             kind_ms[KIND_COUNT]{}, kind_bytes[KIND_COUNT]{};
    long               kind_n[KIND_COUNT]{};
    std::vector<std::tuple<hipEvent_t, hipEvent_t, int, double>> pending;
    std::vector<hipEvent_t>                                       event_pool;

    ~ftcf_gptneox()
    {
        for (void* p : owned) {
            (void)hipFree(p);
        }
        destroy_graphs();
        if (tp_scratch) {
            (void)hipFree(tp_scratch);
        }
        if (tlp_ids) {
            (void)hipFree(tlp_ids);
            (void)hipFree(tlp_values);
        }
        if (stream) {
            (void)hipStreamDestroy(stream);
            for (int c = 0; c < 2; c++) {
                if (ov_done[c]) {
                    (void)hipEventDestroy(ov_done[c]);
                    (void)hipEventDestroy(ov_red[c]);
                }
            }
            for (int c = 0; c < 2; c++) {
                if (dv_done[c]) {
                    (void)hipEventDestroy(dv_done[c]);
                    (void)hipEventDestroy(dv_red[c]);
                    (void)hipEventDestroy(dv_fork[c]);
                }
            }
            if (side2) {
                (void)hipStreamDestroy(side2);
            }
            if (side) {
                (void)hipStreamDestroy(side);
                (void)hipEventDestroy(ev_fork);
                (void)hipEventDestroy(ev_join);
            }
        }
        if (ev_user) {
            (void)hipEventDestroy(ev_user);
        }
        for (hipEvent_t e : tok_ev) {
            if (e) {
                (void)hipEventDestroy(e);
            }
        }
        if (h_flags) {
            (void)hipHostFree(h_flags);
        }
        for (auto e : event_pool) {
            (void)hipEventDestroy(e);
        }
    }

    hipEvent_t get_event()
    {
        if (!event_pool.empty()) {
            hipEvent_t e = event_pool.back();
            event_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        FTCF_HIP_CHECK(hipEventCreate(&e));
        return e;
    }

    template<typename F>
    void timed(int kind, double bytes, F&& f, hipStream_t on = nullptr)
    {
        if (!profiling) {
            f();
            return;
        }
        hipEvent_t a = get_event(), b = get_event();
        FTCF_HIP_CHECK(hipEventRecord(a, on ? on : stream));
        f();
        FTCF_HIP_CHECK(hipEventRecord(b, on ? on : stream));
        pending.emplace_back(a, b, kind, bytes);
    }
    void drain_events()
    {
        for (auto& t : pending) {
            float ms = 0.f;
            FTCF_HIP_CHECK(hipEventSynchronize(std::get<1>(t)));
            FTCF_HIP_CHECK(hipEventElapsedTime(&ms, std::get<0>(t), std::get<1>(t)));
            kind_ms[std::get<2>(t)] += ms;
            kind_bytes[std::get<2>(t)] += std::get<3>(t);
            kind_n[std::get<2>(t)] += 1;
            event_pool.push_back(std::get<0>(t));
            event_pool.push_back(std::get<1>(t));
        }
        pending.clear();
    }

    // ---- arena planning: everything a request of shape (B, S, total) needs, carved once ----
    // The blocks of plan() below, in the order plan() carves them; each sets its own views (and plans) from the Carver it is given
    // and is run twice, first over no memory to learn the size.

    // Whether a request of B rows x K beams may take the one- / two-row persistent kernel.  planned = false is what begin() asks
    // BEFORE the ranks' exchange window exists (is one worth building?): the knobs and the request's shape only; planned = true is
    // plan()'s question: the engine's own limits and the window as well.
    // (L <= 255: the hand-off tags carry the layer in their low byte; tpn <= 8: the exchange-window table of the kernel)
    bool persist_eligible(int B, int K, bool planned) const
    {
        const int  tpn   = cfg.tensor_para_size;
        const bool shape = persist && K == 1 && B <= 2 && cfg.use_gptj_residual && tpn <= PERSIST_MAX_TP && (tpn == 1 || persist_tp);
        return shape && (!planned || (!fp32 && L <= 255 && (tpn == 1 || (cfg.comm && cfg.comm->win_ok))));
    }
    // With tensor parallelism the per-layer all-reduce happens INSIDE the persistent launch, through the ranks'
    // exchange windows (persist_device.hip.h ps_tp_exchange); where the windows are not available (peer mapping or
    // hand-shake failed, FTCF_TP_PERSIST=0) the per-stage launches + RCCL all-reduce stay in charge.
    void plan_persistent(Carver& c, int B, int K, int s_max)
    {
        pplan = PersistPlan{};
        const int  tpn      = cfg.tensor_para_size;
        const bool tp_local = tpn > 1 && cfg.comm && cfg.comm->local;
        if (persist_eligible(B, K, true)) {
            // (a local group shares ONE device: every rank gets 1 / world of its compute units)
            const int nb = tp_local ? std::max(1, (persist_nb > 0 ? persist_nb : num_cu) / tpn) : persist_nb;
            pplan = persist_plan(B, H, hl, il, nhl, dh, s_max, int8, num_cu, nb, persist_cs1, persist_cs3, persist_own, L);
            const bool resident = !pplan.ok ? false
                                  : tp_local ? persist_group_resident(pplan, int8, B, dh, num_cu, tpn)
                                             : persist_resident(pplan, int8, B, dh, num_cu, tpn);
            if (!resident) {
                pplan = PersistPlan{};  // not every workgroup would be resident: the hand-offs could never complete
            }
        }
        if (pplan.ok) {
            ps_slab_n   = (size_t)B * 3 * hl / 2 + (size_t)B * il / 2 + (size_t)B * hl / 2 + (size_t)B * H / 2
                        + (size_t)pplan.gp_n + (size_t)B * nhl * pplan.nsplit * (dh + 2);
            ps_gq       = c.take<unsigned long long>(ps_slab_n + 8);
            ps_gm       = ps_gq ? ps_gq + (size_t)B * 3 * hl / 2 : nullptr;
            ps_gc       = ps_gq ? ps_gm + (size_t)B * il / 2 : nullptr;
            ps_gx       = ps_gq ? ps_gc + (size_t)B * hl / 2 : nullptr;
            ps_gp       = ps_gq ? ps_gx + (size_t)B * H / 2 : nullptr;
            ps_ga       = ps_gq ? ps_gp + (size_t)pplan.gp_n : nullptr;
            ps_err      = ps_gq ? reinterpret_cast<int*>(ps_gq + ps_slab_n) : nullptr;
            d_players   = c.take<PersistLayer>(L);
            ps_tab      = c.take<char>(persist_table_bytes(pplan) * pplan.NB);
            ps_tab_ready = false;
            ps_ts       = ps_ts_file.empty() ? nullptr : c.take<long long>((size_t)pplan.NB * L * 128);
        }
    }
    // 3..16 rows (and what the one- / two-row kernel does not take): the rows kernel, one launch per token.  With tensor
    // parallelism it would be one launch per layer and the all-reduce of x' between them: a rank's shard of a layer is a few
    // microseconds of HBM time behind five in-kernel hand-offs, and the paired launches of the general path are faster
    // (one rank's shard of TP 8 at bs 16: 2.67 against 1.69 ms per step): tensor_para_size 1 only
    void plan_rows(Carver& c, int B, int K, int s_max)
    {
        rplan = RowsPlan{};
        rows_ws = nullptr;
        rows_ts = nullptr;
        // One and two rows are the one- / two-row kernel's; where ITS plan declines a request (fp16 weights at two rows, more than
        // 1248 / 3072 tokens of context: its LDS) the rows kernel takes it -- 2.73 ms per token at one row against 3.2 on the
        // per-stage launches, 3.10 at two rows against 3.48 on the general path (13B int8, 1024-in / 512-out) -- but not when
        // that kernel has been switched off (FTCF_PERSIST=0, or after it gave up once): then the per-stage launches run, the path
        // of a tensor-parallel rank
        const int rmin = persist ? 1 : 3;
        if (rows && cfg.tensor_para_size == 1 && !pplan.ok && !fp32 && K == 1 && B >= rmin && B <= 16
            && cfg.use_gptj_residual && L <= 255) {
            rplan = rows_plan(B, H, hl, il, nhl, dh, s_max, int8, num_cu, rows_nb > 0 ? rows_nb : persist_nb);
            if (rplan.ok && !rows_resident(rplan, int8, dh, num_cu, false)) {
                rplan = RowsPlan{};
            }
            if (rplan.ok) {
                rows_ws   = c.take<char>(rows_workspace_bytes(rplan, B, H, hl, il, nhl, dh));
                d_players = c.take<PersistLayer>(L);  // (the persistent plan, which has a table of its own, is off here)
                rows_ts   = ps_ts_file.empty() ? nullptr : c.take<long long>((size_t)rplan.NB * L * 128);
            }
        }
    }
    // the split-K workspaces of the burst GEMM (5..16 rows per launch) and of the tiled GEMM (17..768 rows)
    void plan_gemm_workspaces(Carver& c, int B, int S, int K)
    {
        // (the four GEMMs of a layer may be in flight together: one region each)
        // (17..SMALLM_MAX_ROWS rows run the same kernel in chunks of 16 rows: sized for one chunk)
        // (a prompt phase of up to SMALLM_MAX_ROWS tokens in all is HBM bound like a decode step: it takes the same kernel)
        const int  bc         = 16;
        const long prefill_m  = S > 1 ? (long)(B / K) * S : 0;
        // (tensor parallel: up to 32 rows as two micro-batches of <= 16, each with its own regions -- decoder_overlapped)
        const bool decode_ws  = B > STAGE_MAX_ROWS && (B <= SMALLM_MAX_ROWS || (cfg.tensor_para_size > 1 && B <= 32));
        const bool prefill_ws = prefill_m > 4 && prefill_m <= SMALLM_MAX_ROWS;
        smallm_partial = gemm_smallm_workspace_bytes(bc, 3 * hl, H, int8) + gemm_smallm_workspace_bytes(bc, il, H, int8)
                         + gemm_smallm_workspace_bytes(bc, H, hl, int8) + gemm_smallm_workspace_bytes(bc, H, il, int8);
        smallm_region  = smallm_partial;
        smallm_partial *= cfg.tensor_para_size > 1 ? 2 : 1;
        smallm_ws = (!fp32 && (decode_ws || prefill_ws)) ? c.take<float>((smallm_partial + gemm_smallm_ticket_bytes()) / 4) : nullptr;
        const bool tiled_rows = prefill_m > 16 || (B > 16 && B <= gemm_tiled_splitk_max_m());
        tiled_ws              = (!fp32 && tiled_rows) ? c.take<float>(gemm_tiled_workspace_bytes() / 4) : nullptr;
    }
    // beam search (rows = batch * K)
    void plan_beams(Carver& c, int B, int S, int total, int K)
    {
        const int s_max = total;
        tiled_ids   = c.take<int>((size_t)B * S);
        tiled_len   = c.take<int>(B);
        parent_ids  = c.take<int>((size_t)total * B);
        step_log_probs = c.take<float>((size_t)total * B);
        cache_indir = c.take<int>((size_t)2 * B * s_max);
        beam_ws     = c.take<char>(beam_workspace_bytes(B / K, K));
        d_div       = c.take<float>(B);
        d_lenpen    = c.take<float>(B);
    }
    // the prompt phase's buffers over M = batch * S tokens (beam search prefills one row per request)
    void plan_prompt(Carver& c, size_t M)
    {
        px             = c.take<f16>(M * H * (fp32 ? 2 : 1));
        pnrm           = c.take<f16>(M * H * (fp32 ? 2 : 1));
        pnrm2          = c.take<f16>(M * H * (fp32 ? 2 : 1));
        pqkv           = c.take<f16>(M * 3 * hl * (fp32 ? 2 : 1));
        pctx           = c.take<f16>(M * hl * (fp32 ? 2 : 1));
        patt           = c.take<f16>(M * H * (fp32 ? 2 : 1));
        pmid           = c.take<f16>(M * il * (fp32 ? 2 : 1));
        pffn           = c.take<f16>(M * H * (fp32 ? 2 : 1));
        ctx_tgt        = c.take<int>(M);
        ctx_lp         = c.take<float>(M);
    }
    // the buffers of a verify pass (speculative decoding)
    void plan_speculative(Carver& c, int s_max)
    {
        const int R  = VERIFY_MAX_ROWS;
        vx           = c.take<f16>((size_t)R * H);
        vnrm         = c.take<f16>((size_t)R * H);
        vnrm2        = c.take<f16>((size_t)R * H);
        vqkv         = c.take<f16>((size_t)R * 3 * hl);
        vctx         = c.take<f16>((size_t)R * hl);
        vatt         = c.take<f16>((size_t)R * H);
        vffn         = c.take<f16>((size_t)R * H);
        vmid         = c.take<f16>((size_t)R * il);
        vlogits      = c.take<float>((size_t)R * V);
        vrot         = c.take<float>((size_t)R * 256);
        spec_aws     = c.take<float>(verify_attention_workspace_bytes(R, nhl, dh, s_max) / 4);
        spec_partial = gemm_smallm_workspace_bytes(R, 3 * hl, H, int8) + gemm_smallm_workspace_bytes(R, il, H, int8)
                       + gemm_smallm_workspace_bytes(R, H, hl, int8) + gemm_smallm_workspace_bytes(R, H, il, int8);
        spec_gws     = c.take<float>((spec_partial + gemm_smallm_ticket_bytes()) / 4);
        spec_draft   = c.take<int>(R);
        spec_ndraft  = c.take<int>(4);
        spec_close_ws = c.take<float>(verify_close_workspace_bytes() / 4);
        spec_sample_ws = c.take<float>(verify_sample_workspace_bytes() / 4);
    }
    // B = rows of the request (batch * beam_width)
    void plan(int B, int S, int total, int K)
    {
        const int s_max = total;
        nsplit          = mmha_pick_nsplit(B, nhl, s_max);
        for (int pass = 0; pass < 2; pass++) {
            Carver c(pass == 0 ? nullptr : arena.ptr);
            const size_t es    = fp32 ? 2 : 1;  // fp32 engine: the same views hold floats
            const size_t cache = (size_t)L * B * nhl * s_max * dh * es;
            k_cache            = c.take<f16>(cache);
            v_cache            = c.take<f16>(cache);
            x                  = c.take<f16>((size_t)B * H * es);
            nrm                = c.take<f16>((size_t)B * H * es);
            nrm2               = c.take<f16>((size_t)B * H * es);
            qkv                = c.take<f16>((size_t)B * 3 * hl * es);
            ctx                = c.take<f16>((size_t)B * hl * es);
            att                = c.take<f16>((size_t)2 * B * H * es);  // [att | ffn]: one message for the layer's all-reduce
            ffn                = att + (size_t)B * H * es;
            mid                = c.take<f16>((size_t)B * il * es);
            logits             = c.take<float>((size_t)B * V);
            gather             = c.take<float>((size_t)B * V);
            mmha_ws            = c.take<float>(mmha_workspace_bytes(B, nhl, dh, nsplit) / 4);
            samp_ws            = c.take<char>(sampling_workspace_bytes(B, V));
            rot_table          = c.take<float>((size_t)B * 256);
            chunk_ws           = c.take<unsigned long long>(chunk_workspace_bytes(H, std::min(B, 4), 8) / 8);
            plan_persistent(c, B, K, s_max);
            plan_rows(c, B, K, s_max);
            plan_gemm_workspaces(c, B, S, K);
            state              = c.take<DecodeState>(1);
            finished           = c.take<uint8_t>(B);
            masked             = c.take<uint8_t>((size_t)B * s_max);
            seq_len            = c.take<int>(B);
            pad_count          = c.take<int>(B);
            step_ids           = c.take<int>((size_t)total * B);
            d_top_k            = c.take<int>(B);
            d_min_length       = c.take<int>(B);
            cum                = c.take<float>(B);
            olp                = c.take<float>((size_t)(total - S) * B);
            d_p_topk           = c.take<float>(B);
            d_p_topp           = c.take<float>(B);
            d_temp             = c.take<float>(B);
            d_rep              = c.take<float>(B);
            draws              = c.take<uint64_t>(B);
            d_seed             = c.take<uint64_t>(B);
            if (K > 1) {
                plan_beams(c, B, S, total, K);
            }
            if (S > 1) {
                plan_prompt(c, (size_t)(B / K) * S);
            }
            if (spec_plan) {  // (behind everything else: the views of a request that does not speculate are where they were)
                plan_speculative(c, s_max);
            }
            if (pass == 0) {
                arena.reserve(c.off + 4096);
            }
        }
    }

    // ---- host-side layer units (layers.hip.h), bound to this engine's GEMM dispatch -----------------------------------
    DecoderSelfAttentionLayer self_attention_layer;
    GptContextAttentionLayer  context_attention_layer;
    FfnLayer                  ffn_layer;
    DynamicDecodeLayer        dynamic_decode_layer;
    bool                      layers_bound = false;
    void bind_layers()
    {
        if (layers_bound) {
            return;
        }
        // (row-count dispatch of gemm(); `slot` is unused here: the burst kernel's four workspace regions are only in flight
        // together on the two-stream branch form, which names its regions itself)
        GemmFn g = [this](const f16* A, const DenseWeight& w, const f16* bias, int act, f16* C, int m, int n, int k, hipStream_t s,
                          int) { gemm(A, w, bias, act, C, m, n, k, s); };
        self_attention_layer    = DecoderSelfAttentionLayer{g, H, hl};
        context_attention_layer = GptContextAttentionLayer{g, H, hl, nhl, dh, cfg.rotary_embedding_dim};
        ffn_layer               = FfnLayer{g, H, il};
        layers_bound            = true;
    }

    void gemm(const f16* A, const DenseWeight& w, const f16* bias, int act, f16* C, int m, int n, int k, hipStream_t on = nullptr)
    {
        hipStream_t stream = on ? on : this->stream;  // (the layer units pass the stream they were given)
        // 5..SMALLM_MAX_ROWS rows (batched decode steps off the branch form, short prompt phases): the burst kernel, 16 rows
        // per launch.  13B int8 prefill, ms: 17 tokens 12.5 -> 6.6, 33..48: 16.3 -> 9.6 (above that the tiled GEMM is as fast).
        if (smallm_ws && m > 4 && m <= SMALLM_MAX_ROWS && gemm_smallm_workspace_bytes(16, n, k, int8) <= smallm_partial) {
            for (int r0 = 0; r0 < m; r0 += 16) {
                launch_gemm_smallm(A + (size_t)r0 * k, w.kernel, w.scale, bias, act, C + (size_t)r0 * n, smallm_ws, smallm_partial,
                                   std::min(16, m - r0), n, k, int8, num_cu, stream, &state->step, &smallm_seq);
            }
            return;
        }
        if (m > 16) {
            launch_gemm_tiled(A, w.kernel, w.scale, bias, act, C, m, n, k, int8, stream, tiled_ws);
            return;
        }
        gemm_dispatch(A, w.kernel, w.scale, bias, act, C, m, n, k, int8, stream, nullptr, smallm_partial, num_cu, &state->step,
                      &smallm_seq);
    }

    // fake peers (FTCF_FAKE_TP, bench.py --fake-tp N): a rank of a TP = N job alone on a one-rank RCCL communicator.  It
    // plays every peer with its own shard, so an all-reduce is TP x its buffer and the gathered logits are TP copies of its
    // slice: outputs are those of a TP = N job whose every rank holds shard `rank`.
    bool fake_peers() const
    {
        return cfg.tensor_para_size > 1 && cfg.comm && cfg.comm->world == 1 && !cfg.comm->local && !cfg.comm->hx;
    }
    int fake_peers_mul() const { return fake_peers() ? cfg.tensor_para_size : 1; }
    // ranks joined by RCCL (what an all-reduce between them hides can only be measured on the node: the "auto" overlap trials)
    bool rccl_ranks() const
    {
        return cfg.tensor_para_size > 1 && cfg.comm && cfg.comm->comm && !cfg.comm->local && !cfg.comm->hx && cfg.comm->world > 1;
    }

    // (consumer_scales: the kernel that reads the result multiplies it by fake_peers_mul() itself -- no launch here)
    void allreduce(f16* buf, size_t count, hipStream_t on = nullptr, bool consumer_scales = false)
    {
        if (cfg.tensor_para_size > 1) {
            Range r("ftcf.allreduce");
            hipStream_t st = on ? on : stream;
            FTCF_CHECK_ARG(cfg.comm && (cfg.comm->comm || cfg.comm->local || cfg.comm->hx), "tensor_para_size > 1 needs a communicator");
            if (window_allreduce(cfg.comm, buf, count, st)) {
                stats.window_allreduces++;
                return;  // through the peer-mapped windows: no RCCL call (prompt-phase messages; k_window_allreduce)
            }
            if (cfg.comm->local) {
                local_allreduce(cfg.comm, buf, count, true, st);
                return;
            }
            if (cfg.comm->hx) {
                hx_allreduce(cfg.comm, buf, count, true, st);
                return;
            }
            if (fake_peers()) {
                if (consumer_scales) {
                    return;
                }
                hipLaunchKernelGGL(k_scale_by_tp<f16>, dim3(256), dim3(256), 0, st, buf, count, (float)cfg.tensor_para_size);
                return;  // TP identical partials
            }
            FTCF_NCCL_CHECK(ncclAllReduce(buf, buf, count, ncclFloat16, ncclSum, cfg.comm->comm, st));
        }
    }

    // vocabulary-split LM head (GptNeoX.cc:888-925): rank r has written its [B, V/TP] slice of `gath` ([TP][B][V/TP] fp32);
    // all-gather it and transpose into out [B, V]
    void allgather_logits(float* gath, float* out, int B, hipStream_t st)
    {
        const int tp = cfg.tensor_para_size;
        float*    mine = gath + (size_t)cfg.tensor_para_rank * B * vl;
        if (fake_peers()) {
            // every peer's slice is this rank's own: the transpose reads slot [rank] for all of them (no collective)
            hipLaunchKernelGGL(k_transpose_gathered_logits, dim3(256), dim3(256), 0, st, out, gath, tp, B, vl,
                               cfg.tensor_para_rank);
            return;
        }
        if (cfg.comm->local) {
            local_allgather(cfg.comm, gath, (size_t)B * vl, false, st);
        }
        else if (cfg.comm->hx) {
            hx_allgather_device(cfg.comm, gath, (size_t)B * vl, 4, st);
        }
        else {
            FTCF_NCCL_CHECK(ncclAllGather(mine, gath, (size_t)B * vl, ncclFloat32, cfg.comm->comm, st));
        }
        hipLaunchKernelGGL(k_transpose_gathered_logits, dim3(256), dim3(256), 0, st, out, gath, tp, B, vl, -1);
    }

    // ---------------------------------------------------------------------------------------------------------------
    // fp32 instantiation (kernels_fp32.hip): the arena views (x, nrm, qkv, ..., the caches, the prefill buffers) hold floats
    // ---------------------------------------------------------------------------------------------------------------
    static float*       F(f16* p) { return reinterpret_cast<float*>(p); }
    static const float* F(const f16* p) { return reinterpret_cast<const float*>(p); }
    static const float* F(const void* p) { return reinterpret_cast<const float*>(p); }
    void allreduce32(float* buf, size_t count)
    {
        if (cfg.tensor_para_size > 1) {
            Range r("ftcf.allreduce");
            FTCF_CHECK_ARG(cfg.comm && (cfg.comm->comm || cfg.comm->local || cfg.comm->hx), "tensor_para_size > 1 needs a communicator");
            if (cfg.comm->local) {
                local_allreduce(cfg.comm, buf, count, false, stream);
                return;
            }
            if (cfg.comm->hx) {
                hx_allreduce(cfg.comm, buf, count, false, stream);
                return;
            }
            if (fake_peers()) {
                hipLaunchKernelGGL(k_scale_by_tp<float>, dim3(256), dim3(256), 0, stream, buf, count, (float)cfg.tensor_para_size);
                return;
            }
            FTCF_NCCL_CHECK(ncclAllReduce(buf, buf, count, ncclFloat32, ncclSum, cfg.comm->comm, stream));
        }
    }
    // one layer's GEMMs / residual on M rows, shared by the context phase and the decode step
    // (GptNeoXContextDecoder.cc:283-507, GptNeoXDecoder.cc:245-384 with T = float)
    template<typename Attn>
    void layer32(const LayerWeights& w, float* X, float* N1, float* Q, float* C, float* A, float* MID, float* FF, int M,
                 bool first_or_last_inplace_variant, Attn&& attention)
    {
        launch_layernorm(X, w.ln1_g, w.ln1_b, N1, M, H, 1e-5f, false, stream);
        launch32_gemm(N1, F(w.qkv.kernel), nullptr, 0, Q, M, 3 * hl, H, stream);
        attention();
        launch32_gemm(C, F(w.attn_out.kernel), nullptr, 0, A, M, H, hl, stream);
        if (!cfg.use_gptj_residual) {
            // sequential residual (GptNeoXDecoder.cc:313-331,362-367): h = attn + bias + x ; x' = ffn(LN2(h)) + bias + h
            allreduce32(A, (size_t)M * H);
            launch32_add_bias_residual(A, X, A, F(w.attn_out.bias), M, H, stream);
            launch_layernorm(A, w.ln2_g, w.ln2_b, N1, M, H, 1e-5f, false, stream);
            launch32_gemm(N1, F(w.ffn1.kernel), F(w.ffn1.bias), 1, MID, M, il, H, stream);
            launch32_gemm(MID, F(w.ffn2.kernel), nullptr, 0, FF, M, H, il, stream);
            allreduce32(FF, (size_t)M * H);
            launch32_add_bias_residual(X, FF, A, F(w.ffn2.bias), M, H, stream);
            return;
        }
        launch_layernorm(X, w.ln2_g, w.ln2_b, N1, M, H, 1e-5f, false, stream);
        launch32_gemm(N1, F(w.ffn1.kernel), F(w.ffn1.bias), 1, MID, M, il, H, stream);
        launch32_gemm(MID, F(w.ffn2.kernel), nullptr, 0, FF, M, H, il, stream);
        launch_add_bias_attn_ffn_residual(X, FF, A, X, w.ffn2.bias, M, H, cfg.tensor_para_size,
                                          first_or_last_inplace_variant ? 0 : 1, false, stream);
        allreduce32(X, (size_t)M * H);
    }
    void context_decoder32(int B, int S, const int* input_lengths, int s_max, int tile)
    {
        Range        r("ftcf.GptNeoXContextDecoder");
        const int    M       = B * S;
        const size_t cache_l = (size_t)B * tile * nhl * s_max * dh;
        for (int l = 0; l < L; l++) {
            const LayerWeights& w = layers[l];
            // (the context decoder's layer_input == layer_output for every layer with padding removal: the fp32-sum variant)
            layer32(w, F(px), F(pnrm), F(pqkv), F(pctx), F(patt), F(pmid), F(pffn), M, false, [&] {
                launch32_context_attention(F(pqkv), F(w.qkv.bias), input_lengths, F(k_cache) + l * cache_l,
                                           F(v_cache) + l * cache_l, B, S, nhl, dh, cfg.rotary_embedding_dim, s_max, F(pctx),
                                           stream, tile);
            });
        }
    }
    void decoder32(int B, int s_max)
    {
        Range        r("ftcf.GptNeoXDecoder");
        const size_t cache_l = (size_t)B * nhl * s_max * dh;
        stats.decode_path    = 2;
        for (int l = 0; l < L; l++) {
            const LayerWeights& w = layers[l];
            // layer_input/output alias for 0 < l < L-1 in the reference (GptNeoXDecoder.cc:249-250) -> residual form
            const bool outer = !(l > 0 && l < L - 1);
            layer32(w, F(x), F(nrm), F(qkv), F(ctx), F(att), F(mid), F(ffn), B, outer, [&] {
                Mmha32Params mp{};
                mp.qkv = F(qkv);
                mp.qkv_bias = F(w.qkv.bias);
                mp.k_cache = F(k_cache) + l * cache_l;
                mp.v_cache = F(v_cache) + l * cache_l;
                mp.seq_len = seq_len;
                mp.pad_count = pad_count;
                mp.masked_tokens = masked;
                mp.finished = finished;
                mp.d_step = &state->step;
                mp.B = B;
                mp.nh = nhl;
                mp.dh = dh;
                mp.rot = cfg.rotary_embedding_dim;
                mp.s_max = s_max;
                mp.ctx = F(ctx);
                if (ses.K > 1) {
                    mp.cache_indir   = cache_indir;
                    mp.beam_width    = ses.K;
                    mp.max_input_len = ses.S;
                    mp.indir_plane   = (size_t)B * s_max;
                }
                launch32_mmha(mp, stream);
            });
        }
    }

    // ---- prompt phase: GptNeoXContextDecoder::forward (GptNeoXContextDecoder.cc:283-507) --------------------------------------
    // The batcher's handles on the prompt phase of ONE sequence (context_decoder_chunked); it sets them before the request and
    // resets them after it.
    int                   prefill_chunk = 0;  // with a hook: the prompt's tokens pass through all layers this many at a time
    std::function<void()> prefill_hook;       // ... and this runs between two chunks
    int                   prefill_begin = 0;  // the prompt phase starts at this token (the prefix cache's hit length)
    std::function<void()> prefill_prefix;     // ... after this has put the K/V of tokens [0, prefill_begin) into cache row 0
    // The batcher's logit processors on an admission's FIRST token: when set, every step of the request materialises its logits
    // [rows, V] (no one-launch LM head + greedy step, no captured graph, no speculation) and calls the hook on the engine's stream
    // between the LM head (all-gather included) and the dynamic decode -- the way top_logprobs leaves the one-launch greedy step.
    // Beam requests do not call it.  Set and reset around one forward() like the members above; unset, nothing changes.
    std::function<void(float* logits, int rows, hipStream_t stream)> logits_hook;
    // the prompt-phase layers of a parallel-residual model (layers.hip.h) over this engine's prompt buffers, cache and streams:
    // B prompt rows; their K/V go to cache rows b * tile of a cache with B * tile rows (beam search: tile = beam_width)
    ParallelResidualContextDecoder context_walk(int B, int S, const int* input_lengths, int s_max, int tile)
    {
        bind_layers();
        ParallelResidualContextDecoder d;
        d.layers = layers.data();
        d.L = L, d.H = H, d.hl = hl, d.il = il, d.tp = cfg.tensor_para_size;
        d.px = px, d.pnrm = pnrm, d.pnrm2 = pnrm2, d.pqkv = pqkv, d.pctx = pctx, d.patt = patt, d.pmid = pmid, d.pffn = pffn;
        d.k_cache = k_cache, d.v_cache = v_cache;
        d.layer_stride  = (size_t)B * tile * nhl * s_max * dh;
        d.input_lengths = input_lengths;
        d.B = B, d.S = S, d.s_max = s_max, d.tile = tile;
        d.attention = context_attention_layer, d.ffn = ffn_layer;
        d.stream = stream, d.side = side, d.ov_done = ov_done, d.ov_red = ov_red;
        return d;
    }
    auto prompt_allreduce()  // (what the walk is handed)
    {
        return [this](f16* buf, size_t count, hipStream_t st) { allreduce(buf, count, st); };
    }
    static bool chunked_supported(bool fp32_, int tp, bool gptj, int H_) { return !fp32_ && tp == 1 && gptj && residual_dual_ln_supported(H_); }
    // Chunked prompt phase of ONE sequence (the continuous-batching front end, section 4e of DESIGN.md): the prompt's tokens pass
    // through all layers `prefill_chunk` at a time, as token spans of the walk, and `prefill_hook` runs between two chunks (the
    // batcher enqueues one decode step of its running slots there: an admission delays them by one chunk, not by the whole
    // prompt).  The same from token `prefill_begin` on (the batcher's prefix cache): `prefill_prefix` runs first, the prompt phase
    // computes the tail only -- in one piece without a hook, in chunks of `prefill_chunk` with one.
    bool context_decoder_chunked(int S, const int* input_lengths, int s_max, int tile = 1)
    {
        const int sb = prefill_begin;
        if (sb > 0) {
            FTCF_CHECK_ARG(chunked_supported(fp32, cfg.tensor_para_size, cfg.use_gptj_residual, H) && tile == 1 && sb < S,
                           "a prompt phase from a token offset needs one sequence, no beams, tensor_para_size 1, parallel residual "
                           "and the dual LayerNorm");
        }
        else if (!prefill_hook || prefill_chunk <= 0 || S <= prefill_chunk
                 || !chunked_supported(fp32, cfg.tensor_para_size, cfg.use_gptj_residual, H)) {
            return false;
        }
        Range r("ftcf.GptNeoXContextDecoder.chunked");
        // (tile = beam_width: the sequence's K/V go to cache row 0 of tile rows)
        const ParallelResidualContextDecoder walk  = context_walk(1, S, input_lengths, s_max, tile);
        const int                            chunk = (prefill_hook && prefill_chunk > 0) ? prefill_chunk : S;
        if (sb > 0 && prefill_prefix) {
            prefill_prefix();
        }
        for (int s0 = sb; s0 < S; s0 += chunk) {
            const int s1 = std::min(S, s0 + chunk);
            walk.forward(PromptSpan::token_range(s0, s1), prompt_allreduce());
            if (s1 < S) {
                prefill_hook();
            }
        }
        return true;
    }

    // Prompt phase under tensor parallelism in two micro-batches, the per-layer all-reduce on the side stream
    // (ParallelResidualContextDecoder::forward_overlapped)
    hipEvent_t ov_done[2] = {nullptr, nullptr}, ov_red[2] = {nullptr, nullptr};
    int        ov_trial = 0;             // auto mode: 0 the next eligible prompt phase runs plain, 1 overlapped, 2 decided
    float      ov_ms[2] = {0.f, 0.f};    // ... what the two trials took (the slowest rank's time)
    bool       ov_ran = false, ov_eligible = false;  // this request (begin() resets them): ran overlapped / counts as a trial
    // where a single sequence's tokens are cut in two (below 64: too short to be worth two micro-batches)
    static int prefill_overlap_cut(int S) { return (S / 2) / 64 * 64; }
    // (no side effects; auto_trial: this request counts as a trial of the auto mode, whichever form it runs)
    bool prefill_overlap_wanted(int B, int S, bool* auto_trial) const
    {
        // OPT-IN (FTCF_PREFILL_OVERLAP=1; read per request, the tests flip it): on the one GPU the builder has, one rank's shard of
        // the 1024-token prompt phase takes 19.1 -> 27.6 ms (TP 2) / 10.3 -> 18.3 ms (TP 8) in two micro-batches -- GEMMs of 512
        // rows fill the chip worse than GEMMs of 1024 (profiles/r03_faketp_prefill.txt) -- and what the overlap hides (40 all-reduces
        // of 10 MiB over xGMI) cannot be measured without the peers.  Whoever has the node should measure both.
        // Round 4: DECIDED FROM DATA on the node it runs on.  FTCF_PREFILL_OVERLAP = 0 / 1 forces it; unset or "auto" (the
        // default for ranks joined by RCCL, i.e. a real multi-GPU job): the first eligible prompt phase of at least 512 tokens
        // runs plain and is timed, the second one overlapped, every rank learns the slower rank's times (comm_max) and the
        // engine keeps the faster form; ftcf_forward_stats says what ran and what the two trials took.
        const char* ev  = getenv("FTCF_PREFILL_OVERLAP");
        const bool  aut = (!ev || !strcmp(ev, "auto")) && rccl_ranks();
        const int   env = (ev && strcmp(ev, "auto")) ? atoi(ev) : 0;
        if ((!env && !aut) || cfg.tensor_para_size == 1 || !cfg.use_gptj_residual || !residual_dual_ln_supported(H) || !side) {
            return false;
        }
        const bool cut = B >= 2 || prefill_overlap_cut(S) >= 64;
        if (aut) {
            *auto_trial = (long)B * S >= 512 && cut;
            if (!*auto_trial || !(ov_trial == 1 || (ov_trial == 2 && ov_ms[1] < ov_ms[0]))) {
                return false;
            }
        }
        return cut;
    }
    void prefill_overlap_events()
    {
        for (int c = 0; c < 2; c++) {
            if (!ov_done[c]) {
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&ov_done[c], hipEventDisableTiming));
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&ov_red[c], hipEventDisableTiming));
            }
        }
    }
    // whether this prompt phase ran overlapped: the halves of the sequences when there are several, else the tokens before and
    // behind the cut of the single one
    bool context_decoder_overlapped(int B, int S, const int* input_lengths, int s_max)
    {
        bool       aut  = false;
        const bool want = prefill_overlap_wanted(B, S, &aut);
        ov_eligible     = aut;
        if (!want) {
            return false;
        }
        Range r("ftcf.GptNeoXContextDecoder.overlapped");
        ov_ran = true;
        prefill_overlap_events();
        const int        cut = prefill_overlap_cut(S);
        const PromptSpan sp0 = B >= 2 ? PromptSpan::sequences(0, B / 2) : PromptSpan::token_range(0, cut);
        const PromptSpan sp1 = B >= 2 ? PromptSpan::sequences(B / 2, B) : PromptSpan::token_range(cut, S);
        context_walk(B, S, input_lengths, s_max, 1).forward_overlapped(sp0, sp1, prompt_allreduce());
        return true;
    }

    // B prompt rows; their K/V go to cache rows b * tile of a cache with B * tile rows (beam search: tile = beam_width)
    void context_decoder(int B, int S, const int* input_lengths, int s_max, int tile)
    {
        if (B == 1 && context_decoder_chunked(S, input_lengths, s_max, tile)) {  // (tile > 1: a beam request's prompt)
            return;
        }
        FTCF_CHECK_ARG(prefill_begin == 0, "a prompt phase from a token offset needs a batch of one sequence");
        if (tile == 1 && context_decoder_overlapped(B, S, input_lengths, s_max)) {
            return;
        }
        Range r("ftcf.GptNeoXContextDecoder");
        if (cfg.use_gptj_residual) {  // the whole batch on the engine stream
            context_walk(B, S, input_lengths, s_max, tile).forward(PromptSpan::sequences(0, B), prompt_allreduce());
            return;
        }
        bind_layers();
        const int    M       = B * S;
        const size_t cache_l = (size_t)B * tile * nhl * s_max * dh;
        for (int l = 0; l < L; l++) {
            const LayerWeights& w = layers[l];
            // sequential residual (GptNeoXContextDecoder.cc:401-418,463-470): the TensorParallel layers reduce their
            // own outputs; h = attn + bias + x ; x' = ffn(LN2(h)) + bias + h
            launch_layernorm(px, w.ln1_g, w.ln1_b, pnrm, M, H, 1e-5f, true, stream);
            context_attention_layer.forward(pnrm, pqkv, pctx, patt, w, input_lengths, k_cache + l * cache_l, v_cache + l * cache_l, B, S,
                                            s_max, tile, stream);
            allreduce(patt, (size_t)M * H);
            launch_add_bias_residual(patt, px, patt, w.attn_out.bias, M, H, stream);
            launch_layernorm(patt, w.ln2_g, w.ln2_b, pnrm, M, H, 1e-5f, true, stream);
            ffn_layer.forward(pnrm, pmid, pffn, w, M, stream);
            allreduce(pffn, (size_t)M * H);
            launch_add_bias_residual(px, pffn, patt, w.ffn2.bias, M, H, stream);
        }
    }

    PersistParams persist_params(int B, int s_max)
    {
        PersistParams pp{};
        pp.layers = d_players;
        pp.L = L;
        pp.x_in = x;
        pp.x_out = x;
        pp.gq = ps_gq;
        pp.gm = ps_gm;
        pp.gc = ps_gc;
        pp.gx = ps_gx;
        pp.gp = ps_gp;
        pp.ga = ps_ga;
        pp.err = ps_err;
        pp.H = H;
        pp.Hl = hl;
        pp.Il = il;
        pp.nh = nhl;
        pp.dh = dh;
        pp.rot = cfg.rotary_embedding_dim;
        pp.s_max = s_max;
        pp.B = B;
        pp.tp = cfg.tensor_para_size;
        pp.tp_rank = cfg.tensor_para_rank;
        for (int r = 0; r < PERSIST_MAX_TP; r++) {
            pp.xw[r] = (cfg.tensor_para_size > 1 && cfg.comm && r < (int)cfg.comm->win.size())
                           ? static_cast<unsigned long long*>(cfg.comm->win[r]) : nullptr;
        }
        if (fake_peers() && !cfg.comm->win.empty()) {
            // fake peers (bench.py --fake-tp N: ONE rank of a TP = N job without its peers): the rank plays every peer --
            // "slot [rank] of rank r's window" is made to land in slot [r] of its own -- so that the kernel's exchange adds
            // TP copies of this rank's partial: outputs are those of a TP = N job whose every rank holds shard `rank`
            for (int r = 0; r < cfg.tensor_para_size && r < PERSIST_MAX_TP; r++) {
                pp.xw[r] = static_cast<unsigned long long*>(cfg.comm->win[0])
                           + (ptrdiff_t)(r - cfg.tensor_para_rank) * ((ptrdiff_t)B * H / 2);
            }
        }
        pp.plan = pplan;
        pp.d_step = &state->step;
        pp.d_stop = &state->all_finished;
        pp.seq_len = seq_len;
        pp.pad_count = pad_count;
        pp.masked_tokens = masked;
        pp.finished = finished;
        pp.rot_table = rot_table;
        pp.eps = 1e-5f;
        pp.ts = ps_ts;
        pp.tab = ps_tab;
        pp.tab_mode = (ps_tab && ps_tab_ready) ? 2 : 0;
        return pp;
    }

    // the model's shape for the rows kernel: every layer of `layer_table`, hidden state xio -> xio (the batcher's decode step
    // fills the rest for its paged pool, rows_params below for this engine's cache)
    RowsParams rows_shape(const PersistLayer* layer_table, f16* xio) const
    {
        RowsParams rp{};
        rp.layers = layer_table;
        rp.L = L;
        rp.l_begin = 0;
        rp.l_end = L;
        rp.x_in = xio;
        rp.x_out = xio;
        rp.H = H;
        rp.Hl = hl;
        rp.Il = il;
        rp.nh = nhl;
        rp.dh = dh;
        rp.rot = cfg.rotary_embedding_dim;
        rp.eps = 1e-5f;
        return rp;
    }
    RowsParams rows_params(int B, int s_max)
    {
        RowsParams rp = rows_shape(d_players, x);
        rp.M = B;
        rp.s_max = s_max;
        rp.tp = cfg.tensor_para_size;
        rp.plan = rplan;
        rows_carve(rp, rows_ws);
        rp.d_step = &state->step;
        rp.d_stop = &state->all_finished;
        rp.seq_len = seq_len;
        rp.pad_count = pad_count;
        rp.input_lengths = ses.sp.input_lengths;
        rp.max_input_len = ses.S;
        rp.finished = finished;
        rp.rot_table = rot_table;
        rp.ts = rows_ts;
        return rp;
    }

    // GptNeoXDecoder::forward (GptNeoXDecoder.cc:245-384)
    void decoder(int B, int s_max)
    {
        Range r("ftcf.GptNeoXDecoder");
        bind_layers();
        const double wbytes  = int8 ? 1.0 : 2.0;
        // (beam search reads K/V through the cache indirection, sequential-residual layers have their own order: general path)
        const bool staged = B <= STAGE_MAX_ROWS && ses.K == 1 && cfg.use_gptj_residual && (dh == 64 || dh == 128);
        stats.decode_path = pplan.ok ? 1 : (staged ? 0 : 2);
        stats.persist_layout = pplan.ok ? pplan.own : 0;
        if (!ses.path_logged) {  // once per request
            ses.path_logged = true;
            FT_LOG_DEBUG(cfg.device, "decoder of this request: %s (rows %d, context %d%s)",
                         pplan.ok ? "persistent layers"
                                  : (rplan.ok ? "persistent layers for up to 16 rows"
                                              : (staged ? "per-stage launches" : "general path (batched GEMMs)")),
                         B, s_max, pplan.ok ? (pplan.uk == 16 ? ", 512 keys per KV split" : ", 256 keys per KV split") : "");
        }
        if (pplan.ok) {
            // all stages of every layer inside persistent launches (kernels_persist.hip); one launch per token when
            // there is no collective between the layers
            PersistParams pp = persist_params(B, s_max);
            // algorithmic bytes of a layer: its four weight matrices + the K/V rows of the current length
            const double layer_bytes = wbytes * ((double)H * 3 * hl + (double)H * il + (double)hl * H + (double)il * H)
                                       + 4.0 * ses.next_step * hl * B;
            pp.l_begin = 0;
            pp.l_end   = L;
            if (cfg.tensor_para_size > 1 && cfg.comm->local) {
                // local group: ONE launch runs every rank (workgroups [r * NB, (r + 1) * NB) = rank r), issued by rank 0
                // between two thread barriers; the other ranks' streams are idle meanwhile
                LocalGroup& g = *cfg.comm->local;
                FTCF_HIP_CHECK(hipStreamSynchronize(stream));  // this rank's inputs (x, rotary table, state) are complete
                g.item[cfg.tensor_para_rank] = &pp;
                g.barrier();
                if (cfg.tensor_para_rank == 0) {
                    PersistGroupParams gp{};
                    for (int r = 0; r < g.world; r++) {
                        gp.p[r] = *static_cast<const PersistParams*>(g.item[r]);
                    }
                    gp.world = g.world;
                    gp.nb    = pplan.NB;
                    launch_decode_persistent_group(gp, int8, stream);
                    FTCF_HIP_CHECK(hipStreamSynchronize(stream));
                }
                g.barrier();
                return;
            }
            timed(KIND_PERSIST, layer_bytes * L, [&] { launch_decode_persistent(pp, int8, stream); });
            return;
        }
        if (rplan.ok) {
            // every stage of every layer inside ONE launch for up to 16 rows (kernels_rows.hip; plan_rows(): tensor_para_size 1 only)
            RowsParams   rp          = rows_params(B, s_max);
            const double layer_bytes = wbytes * ((double)H * 3 * hl + (double)H * il + (double)hl * H + (double)il * H)
                                       + 4.0 * ses.next_step * hl * B;
            stats.decode_path = 3;
            timed(KIND_PERSIST, layer_bytes * L, [&] { launch_decode_rows(rp, int8, stream); });
            return;
        }
        if (!staged && cfg.use_gptj_residual) {
            // general path: the batched parallel-residual layers (layers.hip.h) with this engine's attention, all-reduce and timing
            auto attention = [&](int l, const LayerWeights& w, int r0, int M, hipStream_t st) {
                // (beam search reads K/V through the cache indirection)
                MmhaParams mp = mmha_params(l, w, B, s_max, r0, M, l);
                if (ses.K > 1) {
                    mp.cache_indir   = cache_indir;
                    mp.beam_width    = ses.K;
                    mp.max_input_len = ses.S;
                    mp.indir_plane   = (size_t)B * s_max;
                }
                launch_mmha(mp, st);
            };
            auto reduce = [&](f16* buf, size_t count, hipStream_t st, bool scaled) { allreduce(buf, count, st, scaled); };
            auto time   = [&](double bytes, auto&& launch, hipStream_t st) { timed(KIND_SMALLM, bytes, launch, st); };
            if (decoder_overlapped(B)) {
                Range ro("ftcf.GptNeoXDecoder.overlapped");
                layer_walk().forward_overlapped(B, attention, reduce, time);
                return;
            }
            // Up to SMALLM_MAX_ROWS rows the attention and the FFN branch on two streams, else up to 16 rows the independent GEMMs
            // paired per launch, else gemm()
            const DecodeGemms gemms = (B <= SMALLM_MAX_ROWS && smallm_ws && decode_branches && side) ? DecodeGemms::branches
                                      : (B <= 16 && smallm_ws)                                    ? DecodeGemms::grouped
                                                                                                   : DecodeGemms::plain;
            layer_walk().forward(B, gemms, attention, reduce, time);
            return;
        }
        for (int l = 0; l < L; l++) {
            const LayerWeights& w = layers[l];
            if (staged) {
                // layer_input/output alias for 0 < l < L-1 in the reference (:249-250) -> which residual form it runs
                const int inplace = (l > 0 && l < L - 1) ? 1 : 0;
                // Per-stage launches over row groups of <= 4 rows (the GEMV kernels' register budget).  STAGE_MAX_ROWS > 4
                // would replay every stage per group; measured no faster than the batched GEMM path (the m = 4 forms
                // of these kernels stream at half the m = 1 rate), so larger batches take the small-m GEMM below.
                const int ngrp = (B + 3) / 4;
                for (int stage = 0; stage < 3; stage++) {
                    for (int rg = 0; rg < ngrp; rg++) {
                        const int r0 = rg * 4, M = std::min(4, B - r0);
                        stage_launch(stage, l, w, inplace, B, s_max, r0, M, l + rg * L, ngrp == 1);
                    }
                }
                allreduce(x, (size_t)B * H);
                continue;
            }
            // sequential residual (GptNeoXDecoder.cc:313-331,362-367): h = attn + bias + x ; x' = ffn(LN2(h)) + bias + h
            MmhaParams mp = mmha_params(l, w, B, s_max, 0, B, l);
            if (ses.K > 1) {
                mp.cache_indir   = cache_indir;
                mp.beam_width    = ses.K;
                mp.max_input_len = ses.S;
                mp.indir_plane   = (size_t)B * s_max;
            }
            launch_layernorm(x, w.ln1_g, w.ln1_b, nrm, B, H, 1e-5f, true, stream);
            self_attention_layer.forward(nrm, qkv, ctx, att, w, [&] { launch_mmha(mp, stream); }, B, stream);
            allreduce(att, (size_t)B * H);
            launch_add_bias_residual(att, x, att, w.attn_out.bias, B, H, stream);
            launch_layernorm(att, w.ln2_g, w.ln2_b, nrm, B, H, 1e-5f, true, stream);
            ffn_layer.forward(nrm, mid, ffn, w, B, stream);
            allreduce(ffn, (size_t)B * H);
            launch_add_bias_residual(x, ffn, att, w.ffn2.bias, B, H, stream);
        }
    }

    // the batched parallel-residual decode layers (layers.hip.h) over this engine's decode buffers, burst workspace and streams
    ParallelResidualDecoder layer_walk()
    {
        ParallelResidualDecoder d;
        d.layers = layers.data();
        d.L = L, d.H = H, d.hl = hl, d.il = il;
        d.int8 = int8;
        d.tp = cfg.tensor_para_size;
        d.fake_mul = fake_peers_mul();
        d.pair_ar = tp_pair_ar;
        d.x = x, d.nrm = nrm, d.nrm2 = nrm2, d.qkv = qkv, d.ctx = ctx, d.att = att, d.ffn = ffn, d.mid = mid;
        d.ws = smallm_ws, d.partial = smallm_partial, d.region = smallm_region;
        d.d_step = &state->step;
        d.seq = &smallm_seq;
        d.plain = self_attention_layer.gemm;
        d.stream = stream, d.side = side, d.side2 = side2;
        d.ev_fork = ev_fork, d.ev_join = ev_join;
        d.dv_fork = dv_fork, d.dv_done = dv_done, d.dv_red = dv_red;
        return d;
    }
    // Batched decode under tensor parallelism with the layer's all-reduce OFF the compute stream (GptNeoXDecoder.cc:342-359 runs it
    // in line; the walk itself is ParallelResidualDecoder::forward_overlapped, layers.hip.h).  A parallel-residual layer has ONE reduction, of x' = x + attn + ffn, and everything of the next layer depends on
    // it: the only independent work is another row's.  So the batch is cut in two micro-batches of <= 16 rows that walk the
    // layers on TWO compute streams, independent of each other from the token's embedding to its final LayerNorm; micro-batch c
    // hands x' to the comm stream by event and waits for the reduced x' by event before its next layer, so c's reduction runs
    // under (1 - c)'s GEMMs / attention -- and, this path being bound by the latency of dependent launches rather than by bytes
    // (a TP 8 shard's layer at 16 rows: six launches, 43 us, 39 MB), one micro-batch's launch gaps are filled by the other's
    // kernels.  Each micro-batch reads the layer's weight shard once: for 17..32 rows that is what the chunked GEMMs do anyway, for
    // 4..16 rows it doubles the weight bytes.  All reductions sit on ONE stream in the order c = 0, 1, 0, 1, ...: the window
    // all-reduce's flag words and RCCL see a serial sequence, identical on every rank.  Row-wise arithmetic is that of the whole-batch
    // walk (the burst GEMM's K slices do not depend on the row count; the micro-batches' GEMMs have their own split-K regions), so
    // the tokens are bit-identical to the un-overlapped path (tests/test_gpu_tp_overlap.py, test_gpu_tp_process.py).
    // FTCF_DECODE_OVERLAP = 1 switches it on; "auto" (ranks joined by RCCL): the first eligible request's token loop runs plain,
    // the second one overlapped, every rank keeps the slowest rank's ms per step (comm_max in finish()) and the engine stays with
    // the faster form -- what an all-reduce over xGMI hides can only be measured on the node.  The default is OFF since round 6:
    // the eager three-stream form hides 5-15 % of a modelled reduction and loses at 16 rows (profiles/r05_decode_overlap_model.txt),
    // the auto trial compares two different requests, and none of it has run on a multi-GPU node.
    hipEvent_t dv_done[2] = {nullptr, nullptr}, dv_red[2] = {nullptr, nullptr}, dv_fork[2] = {nullptr, nullptr};
    int        dv_trial = 0;
    float      dv_ms[2] = {0.f, 0.f};  // ms per decode step of the two trials (the slowest rank's)
    bool       dv_ran = false, dv_eligible = false;
    bool decode_overlap_shape(int B) const
    {
        return cfg.tensor_para_size > 1 && !fp32 && ses.K == 1 && cfg.use_gptj_residual && residual_dual_ln_supported(H) && side
               && smallm_ws && smallm_partial >= 2 * smallm_region && B >= 4 && B <= 2 * 16 && !pplan.ok && !rplan.ok;
    }
    void decode_overlap_streams()
    {
        if (!side2) {
            FTCF_HIP_CHECK(hipStreamCreateWithFlags(&side2, hipStreamNonBlocking));
        }
        for (int c = 0; c < 2; c++) {
            if (!dv_done[c]) {
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&dv_done[c], hipEventDisableTiming));
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&dv_red[c], hipEventDisableTiming));
                FTCF_HIP_CHECK(hipEventCreateWithFlags(&dv_fork[c], hipEventDisableTiming));
            }
        }
    }
    // (no side effects: step() asks it too -- the three-stream form is enqueued eagerly, not captured into the token's hipGraph:
    // a capture of it aborted inside the runtime on the one-rank RCCL communicator of `bench.py --fake-tp`, round 5)
    bool decode_overlap_wanted(int B, bool* auto_trial = nullptr) const
    {
        // (decode_overlap_mode: FTCF_DECODE_OVERLAP read when a request begins -- 0, the default, 1, or 2 = "auto")
        const bool  aut = decode_overlap_mode == 2 && rccl_ranks();
        const int   env = decode_overlap_mode == 1 ? 1 : 0;
        if ((!env && !aut) || !decode_overlap_shape(B)) {
            return false;
        }
        if (auto_trial) {
            *auto_trial = aut;
        }
        return !aut || dv_trial == 1 || (dv_trial == 2 && dv_ms[1] < dv_ms[0]);
    }
    // whether this step's layers take the overlapped walk (ParallelResidualDecoder::forward_overlapped); makes its streams ready
    bool decoder_overlapped(int B)
    {
        bool aut = false;
        const bool want = decode_overlap_wanted(B, &aut);
        dv_eligible = aut;
        if (!want) {
            return false;
        }
        dv_ran = true;
        decode_overlap_streams();
        return true;
    }

    // Rows up to which the per-stage GEMV launches run (when the persistent kernel is not eligible).  Measured at 13B int8,
    // TP = 1, ms per step, per-stage vs general path (burst GEMMs): B = 1: 3.34 vs 3.61 (and 1.28 vs 1.57 on a TP = 8
    // shard); B = 2: 4.13 vs 3.85; B = 3: 4.64 vs 3.65; B = 4: 5.78 vs 3.73 -- the m = 2..4 forms of the GEMV kernels stream
    // at a fraction of the m = 1 rate.  FTCF_STAGE_MAX_ROWS (<= 4) overrides, the tests use it to keep those forms covered.
    int STAGE_MAX_ROWS = 1;
    // Rows up to which the batched decode GEMMs (and short prompt phases) run the burst kernel, 16 rows per launch (the weights
    // are then read ceil(B / 16) times).  Above 16 rows the alternative is the tiled GEMM in its split-K form (64-row tiles cut
    // along K, four k-steps of weights and activations in flight): 13B int8, ms per decode step, chunked burst vs split-K tiled:
    // bs = 24: 6.8 vs 6.4; 32: 7.4 vs 6.5; 48: 10.2 vs 7.5; 64: 13.6 vs 8.7 -- and prompt phases of 17 / 33 / 64 tokens
    // 7.0 / 10.2 / 13.8 vs 6.0 / 6.2 / 6.5 ms.  (Round 2's tiled GEMM without the split: 13.8 ms at bs = 24, 19.4 at 64.)
    // FTCF_SMALLM_MAX_ROWS overrides (<= 256; the chunked form stays covered by the tests through it).
    int SMALLM_MAX_ROWS = 16;

    // decoder attention of rows [r0, r0 + M) of the batch (KV cache [L][B][nh][s_max][dh]); `salt` makes the granule
    // tags of every launch of a token distinct
    MmhaParams mmha_params(int l, const LayerWeights& w, int B, int s_max, int r0, int M, int salt)
    {
        const size_t cache_l = (size_t)B * nhl * s_max * dh;
        const size_t row_kv  = (size_t)nhl * s_max * dh;
        MmhaParams   mp{};
        mp.qkv = qkv + (size_t)r0 * 3 * hl;
        mp.qkv_bias = w.qkv.bias;
        mp.k_cache = k_cache + l * cache_l + r0 * row_kv;
        mp.v_cache = v_cache + l * cache_l + r0 * row_kv;
        mp.seq_len = seq_len + r0;
        mp.pad_count = pad_count + r0;
        mp.masked_tokens = masked + (size_t)r0 * s_max;
        mp.finished = finished + r0;
        mp.d_step = &state->step;
        mp.rot_table = rot_table + (size_t)r0 * (cfg.rotary_embedding_dim / 2) * 2;
        mp.B = M;
        mp.nh = nhl;
        mp.dh = dh;
        mp.rot = cfg.rotary_embedding_dim;
        mp.s_max = s_max;
        mp.ctx = ctx + (size_t)r0 * hl;
        mp.gran = (unsigned long long*)mmha_ws + (size_t)r0 * nhl * nsplit * (dh + 2);
        mp.layer = salt;
        mp.nsplit = nsplit;
        return mp;
    }

    // One of the three launches of a layer for rows [r0, r0 + M), M <= 4:
    //   0: K1  LN1 -> QKV                                  (78.6 MB/TP int8)
    //   1: K2  MMHA  ||  LN2 -> FFN1 + bias + gelu         (attention hidden under 104.9 MB/TP of streaming)
    //   2: K3  [out-proj U FFN2] -> residual               (131 MB/TP)
    void stage_launch(int stage, int l, const LayerWeights& w, int inplace, int B, int s_max, int r0, int M, int salt,
                      bool time_it)
    {
        const double wbytes = int8 ? 1.0 : 2.0;
        f16*         xr     = x + (size_t)r0 * H;
        auto run = [&](int kind, double bytes, auto&& f) {
            if (time_it) {
                timed(kind, bytes, f);
            }
            else {
                f();
            }
        };
        if (stage == 0) {
            LnGemvParams a{};
            a.x = xr;
            a.gamma0 = w.ln1_g;
            a.beta0 = w.ln1_b;
            a.W0 = w.qkv.kernel;
            a.scale0 = w.qkv.scale;
            a.out0 = qkv + (size_t)r0 * 3 * hl;
            a.K = H;
            a.NT0 = 3 * hl / 16;
            a.NT1 = 0;
            a.blocks0 = (a.NT0 + 3) / 4;
            a.blocks1 = 0;
            a.eps = 1e-5f;
            run(KIND_LN_GEMV, wbytes * H * (3.0 * hl), [&] {
                if (k1_wpg > 0) {
                    launch_ln_gemv_group(a, int8, M, k1_wpg, stream);
                }
                else {
                    launch_ln_gemv(a, int8, M, stream);
                }
            });
        }
        else if (stage == 1) {
            MmhaParams   mp = mmha_params(l, w, B, s_max, r0, M, salt);
            LnGemvParams f{};
            f.x = xr;
            f.gamma1 = w.ln2_g;
            f.beta1 = w.ln2_b;
            f.W1 = w.ffn1.kernel;
            f.scale1 = w.ffn1.scale;
            f.bias1 = w.ffn1.bias;
            f.out1 = mid + (size_t)r0 * il;
            f.K = H;
            f.NT0 = 0;
            f.NT1 = il / 16;
            f.blocks0 = 0;
            f.blocks1 = f.NT1 / 2;  // two column groups per workgroup (NT1 is even: local inter is a multiple of 64)
            f.eps = 1e-5f;
            run(KIND_FUSED, wbytes * H * (double)il, [&] { launch_mmha_ln_gemv(mp, f, int8, M, stream); });
        }
        else {
            const int tk = int8 ? TILE_K_I8 : TILE_K_F16;
            if (k3_q > 0) {
                ChunkParams c{};
                c.x_a = ctx + (size_t)r0 * hl;
                c.x_b = mid + (size_t)r0 * il;
                c.W_a = w.attn_out.kernel;
                c.W_b = w.ffn2.kernel;
                c.scale_a = w.attn_out.scale;
                c.scale_b = w.ffn2.scale;
                c.bias = w.ffn2.bias;
                c.x_in = xr;
                c.out = xr;
                c.N = H;
                c.KT_a = hl / tk;
                c.KT_b = il / tk;
                c.Q = k3_q;
                c.T = (c.KT_a + c.KT_b + c.Q - 1) / c.Q;
                c.tp = cfg.tensor_para_size;
                c.inplace_variant = inplace;
                c.gran = chunk_ws;
                c.d_step = &state->step;
                c.salt = salt;
                run(KIND_SPLITK, wbytes * H * ((double)hl + il), [&] { launch_gemv_chunked(c, int8, M, stream); });
            }
            else {
                SplitKParams c{};
                c.x_a = ctx + (size_t)r0 * hl;
                c.x_b = mid + (size_t)r0 * il;
                c.W_a = w.attn_out.kernel;
                c.W_b = w.ffn2.kernel;
                c.scale_a = w.attn_out.scale;
                c.scale_b = w.ffn2.scale;
                c.bias = w.ffn2.bias;
                c.x_in = xr;
                c.out = xr;
                c.N = H;
                c.KT_a = hl / tk;
                c.KT_b = il / tk;
                c.tp = cfg.tensor_para_size;
                c.inplace_variant = inplace;
                plan_splitk(c, int8, M, 10);
                run(KIND_SPLITK, wbytes * H * ((double)hl + il),
                    [&] { launch_gemv_splitk(c, int8, M, EPI_RESIDUAL, stream); });
            }
        }
    }

    // ---- request session: forward() == begin() + step(all) + finish() ----
    struct Session {
        bool              active = false;
        ftcf_forward_args a{};
        SamplingParams    sp{};
        BeamParams        bp{};
        int               B = 0, S = 0, total = 0, s_max = 0;  // B = rows (batch * beam_width)
        int               K = 1, batch = 0;
        int               next_step = 0;  // host mirror of state->step
        int               steps = 0;
        bool              all_finished = false;
        hipEvent_t        e0 = nullptr, e1 = nullptr;
        hipGraphExec_t    graph_exec = nullptr;
        bool              path_logged = false;  // the decoder of this request has been named in the log (FT_LOG_LEVEL=DEBUG)
        hipGraphExec_t    graph_exec_n = nullptr;  // graph_tokens consecutive tokens in one graph (persistent path, no callback)
        // speculative decoding: on for this request; K, N; the draft count the last step's draft kernel left for the next one;
        // verify passes, drafts proposed / accepted so far
        bool              spec = false;
        int               spec_K = 0, spec_N = 0, spec_nd = 0;
        int               spec_steps = 0, spec_drafted = 0, spec_accepted = 0;
        // a top-k sampled request that speculates: its passes close with the sampled tail on what the plain steps sample with
        bool              spec_sampled = false;
        int               spec_top_k = 0, spec_apply_temp = 0;
        float             spec_p_topk = 1.f, spec_temp = 1.f;
        uint64_t          spec_seed = 0;
        // the state a request starts its token loop from: everything above as declared (no step taken; no graph captured: the
        // previous request's were destroyed by abandon_session() / finish()) but what the request itself says.  [e0, e1] time
        // the prompt phase.
        void open(const ftcf_forward_args& args, const SamplingParams& sampling, const BeamParams& beams, hipEvent_t t0, hipEvent_t t1,
                  bool speculate)
        {
            Session s;
            s.active    = true;
            s.a         = args;
            s.sp        = sampling;
            s.bp        = beams;
            s.K         = args.beam_width;
            s.batch     = args.batch_size;
            s.B         = args.batch_size * args.beam_width;
            s.S         = args.max_input_len;
            s.total     = args.max_input_len + args.output_len;
            s.s_max     = s.total;
            s.next_step = s.S;
            s.e0        = t0;
            s.e1        = t1;
            s.spec      = speculate;
            s.spec_K    = args.speculative_tokens;
            s.spec_N    = args.speculative_ngram > 0 ? args.speculative_ngram : 3;
            *this       = s;
        }
    } ses;
    bool use_graph = true;
    void destroy_graphs()
    {
        for (hipGraphExec_t* g : {&ses.graph_exec, &ses.graph_exec_n}) {
            if (*g) {
                (void)hipGraphExecDestroy(*g);
                *g = nullptr;
            }
        }
    }
    // drops whatever an unfinished request left behind: the captured graph holds the OLD arena pointers, shapes and sampling
    // flags, and plan() may free that arena -- replaying it for the next request would corrupt memory silently
    void abandon_session()
    {
        if (!ses.active && !ses.graph_exec) {
            return;
        }
        (void)hipStreamSynchronize(stream);
        destroy_graphs();
        if (ses.e0) {
            event_pool.push_back(ses.e0);
            ses.e0 = nullptr;
        }
        if (ses.e1) {
            event_pool.push_back(ses.e1);
            ses.e1 = nullptr;
        }
        drain_events();
        ses.active = false;
    }
    // ---- the request lifecycle (engine.hip), each of begin / step / finish a sequence of the stages declared under it ----
    void bind_weights(const ftcf_gptneox_weights& w);  // (create: the layer table; fp16 kernels are re-tiled on `stream`)
    void read_env_knobs();                             // (create: every knob that is read once per engine)
    void begin(const ftcf_forward_args& a);
    void check_request(const ftcf_forward_args& a) const;
    void ensure_exchange_window(int B, int K);
    void clear_exchange_window();
    bool speculation_wanted(const ftcf_forward_args& a, int total);
    SamplingRouting upload_sampling_args(const ftcf_forward_args& a);
    void reset_workspaces(int B);
    void tile_beam_inputs(const ftcf_forward_args& a);
    void upload_layer_tables(int B, int s_max);
    void prompt_phase(const ftcf_forward_args& a, const int* in_ids, const int* in_len);
    void score_prompt(const ftcf_forward_args& a);
    void ensure_top_logprob_buffers(size_t pairs);
    SamplingParams session_sampling_params(const ftcf_forward_args& a, const SamplingRouting& route, const int* in_len) const;
    BeamParams     session_beam_params(const ftcf_forward_args& a, const SamplingRouting& route, const int* in_len) const;
    void enqueue_step(bool with_decoder);
    void enqueue_decoder(bool with_decoder);
    bool enqueue_lm_head();
    hipGraphExec_t capture_steps(int tokens);
    int  step(int max_steps);
    int  step_speculative(int max_steps);
    void verify_pass(int step, int drafts);
    void finish();
    void write_outputs();
    void beam_log_probs(float* log_probs, size_t capacity);  // (of the last request, until the next begin)
    struct ErrorWords {  // what the kernels' sticky give-up words held when the request ended
        int ps = 0, smallm = 0, rows = 0;
    };
    void read_error_words(ErrorWords& w);
    void close_overlap_trials(float prefill_ms);
    void dump_timestamps(int NB, const long long* ts);
    void raise_give_ups(ErrorWords w);
    // the stopwatch of one step() call: [start, stop] on the stream; stop waits for the stream and adds to stats.decode_ms
    struct DecodeStopwatch {
        ftcf_gptneox& e;
        hipEvent_t    ea, eb;
        explicit DecodeStopwatch(ftcf_gptneox& eng): e(eng), ea(eng.get_event()), eb(eng.get_event())
        {
            FTCF_HIP_CHECK(hipEventRecord(ea, e.stream));
        }
        void stop(const char* what)
        {
            FTCF_HIP_CHECK(hipEventRecord(eb, e.stream));
            comm_event_sync(e.cfg.comm, eb, what);
        }
        void add_to_stats()
        {
            float ms = 0.f;
            FTCF_HIP_CHECK(hipEventElapsedTime(&ms, ea, eb));
            e.stats.decode_ms += ms;
            e.event_pool.push_back(ea);
            e.event_pool.push_back(eb);
        }
    };
    bool persist_failed = false;  // the persistent kernel gave up on a hand-off during the last request
    bool winar_failed = false;    // ... or the exchange-window all-reduce of the prompt phase did
    int  persist_fail_once = 0;
    void forward(const ftcf_forward_args& a)
    {
        begin(a);
        step(a.output_len);
        try {
            finish();
        }
        catch (const Error&) {
            if (winar_failed && !persist_failed) {
                winar_failed = false;
                FT_LOG_WARNING(cfg.device, "exchange-window all-reduce gave up: replaying the request with the communicator's own "
                                           "all-reduce (it stays there)");
                begin(a);
                step(a.output_len);
                finish();
                return;
            }
            if (!persist_failed) {
                throw;
            }
            // The persistent kernel's hand-offs need every workgroup resident; the plan checks that, but compute units can
            // still be taken away (another process, a masked CU) after the check.  Its spins are bounded and report through
            // a sticky error word instead of hanging the GPU; the request is then replayed from the start on the
            // per-stage / general path (tensor parallel: every rank takes this branch -- finish() agrees on the error
            // word across the ranks) and the engine stays off the persistent path.
            persist_failed = false;  // (finish() has switched off the kernel that gave up: `persist` or `rows`)
            FT_LOG_WARNING(cfg.device, "persistent decode kernel gave up on a hand-off: replaying the request on the per-stage "
                                       "path (this engine stays there)");
            begin(a);
            step(a.output_len);
            finish();
        }
    }
};
