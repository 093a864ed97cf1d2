// Continuous batching over a paged K/V cache (include/ftcf.h `ftcf_batcher_*`): split out of engine.hip in round 4.
#include "engine.hip.h"
#include "attn_device.hip.h"  // rotary_coef (the rows kernel's rotary table of a step)
#include "batcher_sched.h"

#include <chrono>


// ---------------------------------------------------------------------------------------------------------------
// Continuous batching over a paged K/V cache (no counterpart in the reference, whose serving layer -- the
// Triton backend -- allocates the cache per request, GptNeoX.cc:84-156).
//
// A batcher borrows an engine (weights, streams, kernels) and owns
//   * a K/V POOL of fixed-size pages, [L][page][head][P tokens][dh] fp16, shared by all sequences, with a free list;
//   * `max_batch` SLOTS: page table, length, last token, sampling parameters of the sequence living there;
//   * a queue of waiting requests.
// One iteration (ftcf_batcher_step) = ADMIT waiting requests into free slots while their pages (prompt + max_new_tokens,
// reserved up front: by default a running sequence never has to be preempted) are available, then ONE decode step for all running
// slots.  Admission runs the prompt through the engine's own context path (ftcf_gptneox_forward with output_len 1: prefill +
// first token sampled by the engine's dynamic decode) and scatters the prompt's K/V into the slot's pages; the decode
// step is the general layer sequence of the engine (§4a: dual LayerNorm, burst / tiled GEMMs, fused residual) with the
// attention replaced by k_mmha_paged (the engine's mmha_partial over the page table, one split), the LM head, and the engine's sampling kernels on per-slot arrays.  A sequence leaves
// when it emits end_id or reaches max_new_tokens; its pages return to the free list at once.
// Scope: parallel-residual models, any tensor_para_size (round 4: one batcher per rank), fp16 / int8 engines; top-k / top-p /
// temperature sampling with repetition penalty, stop words and a token callback; beam search (round 4: BeamGroup below).
// Prefix cache (ftcf_batcher_create_ex, off by default): the pages of finished prompt blocks stay in a PrefixIndex
// (prefix_index.h); a request whose prompt starts with cached blocks takes those pages, k_gather_pages_to_kv copies them into
// the engine's cache and the prompt phase runs from the first uncached token (context_decoder_chunked with prefill_begin).
// Beam requests neither read nor populate it.
// Overcommit (ftcf_batcher_create_opts, off by default; batcher_sched.h): requests take their pages as they grow; when
// the pool runs dry the latest arrival among the running ordinary requests is swapped out -- k_pages_pack into a staging buffer,
// a linear copy to pinned host pages -- and resumes later in any free slot on fresh pages (the reverse with k_pages_unpack), its
// device state uploaded by the function an admission uses (upload_slot_state).  Beam groups are never swapped.
// Fork requests (ftcf_batcher_submit_n; admit_fork): n samples of one prompt from ONE prompt phase -- the prompt's
// full pages shared by reference, k_batcher_fanout for the logits row and the tail rows, the first tokens drawn by the decode
// step's own logit and sampling stages; from then on n ordinary sequences.
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_batcher_embed(f16* out, const f16* table, const int* tok, int H)
{
    const int  id  = tok[blockIdx.x];
    const f16* src = table + (size_t)id * H;
    f16*       dst = out + (size_t)blockIdx.x * H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        *reinterpret_cast<f16x8*>(dst + i) = *reinterpret_cast<const f16x8*>(src + i);
    }
}
// d_tok[b] = the token the sampling kernels just wrote into slot b's history (time-major [max_len][B], position len[b])
__global__ void k_batcher_last_token(int* tok, const int* hist, const int* len, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        tok[b] = hist[(size_t)len[b] * B + b];
    }
}
__global__ void k_batcher_tick(DecodeState* gemm_state)
{
    gemm_state->step = (gemm_state->step + 1) & 0x7ffff;  // part of the burst GEMMs' granule tags (19 bits)
}

// the rows kernel inside the batcher (round 5): its step counter (the hand-off tags are step * 256 + layer + 1) and the rotary table
// of the step -- a slot's new token sits at position len[slot] (decoder_masked_multihead_attention_utils.h:1325-1345 coefficients,
// as mmha_partial computes them in place for k_mmha_paged, whose rotary position is the slot's length)
__global__ void k_batcher_rows_prep(int* step, float* rot_table, const int* len, int rot)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *step = *step + 1;
    }
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < rot / 2; j += blockDim.x) {
        float cs, sn;
        rotary_coef(j, rot, len[b], cs, sn);
        rot_table[((size_t)b * (rot / 2) + j) * 2]     = cs;
        rot_table[((size_t)b * (rot / 2) + j) * 2 + 1] = sn;
    }
}

// beam groups (see ftcf_batcher::BeamGroup): copy-on-write of K/V pages, every layer of both pools; pairs = {src, dst} page ids
__global__ void k_batcher_copy_pages(f16* kpool, f16* vpool, const int* pairs, size_t page_elems, size_t pool_layer_elems)
{
    f16*         pool = blockIdx.z ? vpool : kpool;
    const int    src = pairs[2 * blockIdx.x], dst = pairs[2 * blockIdx.x + 1];
    const u32x4* sp = reinterpret_cast<const u32x4*>(pool + (size_t)blockIdx.y * pool_layer_elems + (size_t)src * page_elems);
    u32x4*       dp = reinterpret_cast<u32x4*>(pool + (size_t)blockIdx.y * pool_layer_elems + (size_t)dst * page_elems);
    for (size_t i = threadIdx.x; i < page_elems / 8; i += blockDim.x) {
        dp[i] = sp[i];
    }
}
// A fork admission (ftcf_batcher_submit_n: n siblings of one prompt), ONE launch.  fork = {slot of sibling i}[n], then {tail
// page of sibling i}[n]: the first page of its own, which receives the prompt's `tail` = len % P last rows.
//   blockIdx.y == 0: the prompt's last-row logits `src` [V] into the n sibling rows of the step's logits buffer.  A row starts at
//     element slot * V: 16-byte stores from the row's first aligned element on, scalar elements before it and behind the last whole
//     quad (V = 97); the loads are 16 bytes too where V % 4 == 0 keeps source and row aligned alike.
//   blockIdx.y == 1 + ((j - 1) * L + l) * 2 + kv: layer l, K | V, the LIVE rows [0, tail) of every head of sibling 0's tail page
//     (written by the scatter from the engine's cache) into sibling j's.  A page is [nh][P][dh]: a head's live rows are ONE
//     contiguous run of tail * dh fp16 (dh a multiple of 8: 16-byte pieces), one wave per run; the rest of the fresh page stays
//     untouched.  tail == 0: the launch has no such blocks.
__global__ __launch_bounds__(256) void k_batcher_fanout(float* logits, const float* src, int V, f16* kpool, f16* vpool, const int* fork,
                                                        int n, int L, int nh, int P, int dh, int tail, size_t pool_layer_elems)
{
    if (blockIdx.y == 0) {
        const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsize = gridDim.x * blockDim.x;
        for (int i = 0; i < n; i++) {
            const size_t o    = (size_t)fork[i] * V;
            float*       d    = logits + o;
            const int    head = min(V, (int)((4 - (o & 3)) & 3)), nq = (V - head) >> 2;
            for (int q = gtid; q < nq; q += gsize) {
                const float* s = src + head + 4 * q;
                f32x4        v;
                if (head == 0) {
                    v = *reinterpret_cast<const f32x4*>(s);
                }
                else {
                    v = f32x4{s[0], s[1], s[2], s[3]};
                }
                *reinterpret_cast<f32x4*>(d + head + 4 * q) = v;
            }
            if (blockIdx.x == 0) {
                for (int t = threadIdx.x; t < head; t += blockDim.x) {
                    d[t] = src[t];
                }
                for (int t = head + 4 * nq + threadIdx.x; t < V; t += blockDim.x) {
                    d[t] = src[t];
                }
            }
        }
        return;
    }
    const int    y = blockIdx.y - 1, kv = y & 1, l = (y >> 1) % L, j = 1 + (y >> 1) / L;
    const int    lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const size_t page_elems = (size_t)nh * P * dh;
    f16*         pool = (kv ? vpool : kpool) + (size_t)l * pool_layer_elems;
    const u32x4* sp = reinterpret_cast<const u32x4*>(pool + (size_t)fork[n] * page_elems);
    u32x4*       dp = reinterpret_cast<u32x4*>(pool + (size_t)fork[n + j] * page_elems);
    const int    run = tail * dh / 8;  // 16-byte pieces of one head's live rows
    for (int h = blockIdx.x * waves + wave; h < nh; h += gridDim.x * waves) {
        const size_t ho = (size_t)h * P * dh / 8;
        for (int i = lane; i < run; i += 64) {
            dp[ho + i] = sp[ho + i];
        }
    }
}
// the sampling kernels' view of `finished`: the rows of beam groups are not theirs (merge = 0: make the view, 1: take the
// sampled rows' new flags back)
__global__ void k_batcher_sampling_view(uint8_t* sfin, uint8_t* fin, const uint8_t* isbeam, int B, int merge)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        if (!merge) {
            sfin[b] = fin[b] | isbeam[b];
        }
        else if (!isbeam[b]) {
            fin[b] = sfin[b];
        }
    }
}
__global__ void k_batcher_set_step(DecodeState* st, int step)
{
    st->step = step;
}
// a group's beams after k_beam_batch: next input token = the word chosen for the beam, one more cached position
__global__ void k_batcher_beam_advance(int* tok, int* len, const int* out_row, int K)
{
    if ((int)threadIdx.x < K) {
        tok[threadIdx.x] = out_row[threadIdx.x];
        len[threadIdx.x] += 1;
    }
}

static_assert(BatcherSched::MAX_BEAM_WIDTH == BEAM_MAX_K, "the scheduler's beam width limit is the beam kernels'");

// the scheduler's host state (batcher_sched.h: queue, slots, pages, admission policy) + the device side
struct ftcf_batcher : BatcherSched {
    struct BeamResult {
        int                K = 0, total = 0;
        std::vector<int>   ids, lens;
        std::vector<float> cum;
        bool               has_lp = false;  // the request asked for token_log_probs
        std::vector<float> lp;              // [K][max_new]
    };
    std::map<long, BeamResult> beam_results;  // finished beam requests until they are fetched
    ftcf_gptneox* e = nullptr;
    size_t        pool_layer_elems = 0;
    // device
    f16 *kpool = nullptr, *vpool = nullptr;
    f16 *x = nullptr, *nrm = nullptr, *nrm2 = nullptr, *qkv = nullptr, *ctx = nullptr, *att = nullptr, *mid = nullptr, *ffn = nullptr;
    float*    logits = nullptr;
    float*    gather = nullptr;  // tensor parallel: [TP][max_batch][V / TP] slices of the LM head
    int *     d_pt = nullptr, *d_len = nullptr, *d_tok = nullptr, *d_topk = nullptr, *d_zero = nullptr, *d_prompt = nullptr, *d_plen = nullptr,
        *d_pout = nullptr, *d_pseq = nullptr, *d_pages_tmp = nullptr;
    uint8_t*     d_fin = nullptr;
    // beam groups: the sampling kernels' view of d_fin, which slots are beams, per-group state of the beam kernels
    uint8_t *    d_sfin = nullptr, *d_isbeam = nullptr;
    int *        d_bout = nullptr, *d_bpar = nullptr, *d_bseq = nullptr, *d_bin = nullptr, *d_pairs = nullptr, *d_bres = nullptr,
        *d_bres_len = nullptr;
    // every group's step log-probabilities (a region like d_bout's) and the finished group's [K][max_new] values
    float *      d_blp = nullptr, *d_bres_lp = nullptr;
    float *      d_btemp = nullptr, *d_brep = nullptr, *d_bdiv = nullptr, *d_blen = nullptr;
    int *        d_bsw = nullptr, *d_bmin = nullptr;  // a group's stop words ([2][STOP_LW], the reference's layout) and min_length
    DecodeState* d_bstate = nullptr;
    void*        beam_ws = nullptr;
    float *      d_ptopk = nullptr, *d_ptopp = nullptr, *d_temp = nullptr, *d_cum = nullptr, *d_rep = nullptr;
    float *      d_olp = nullptr, *d_polp = nullptr;  // log-probability of each slot's token of a decode step / of an admission's first
    // ftcf_batcher_step_top: the same for the top_n (<= 20) alternatives, [slot][top_n] {id, log-probability}
    int *        d_top_ids = nullptr, *d_ptop_ids = nullptr;
    float *      d_top_lp = nullptr, *d_ptop_lp = nullptr;
    int*         d_hist = nullptr;  // [max_len + 1][max_batch] time-major token history of the slots (repetition penalty)
    int *        d_sw = nullptr;    // admission: stop words of the ragged batch, the reference's [n][2][Lw] layout
    uint64_t *   d_seed = nullptr, *d_draws = nullptr;
    DecodeState *d_state = nullptr, *d_gstate = nullptr;
    void*        samp_ws = nullptr;
    float*       smallm_ws = nullptr;
    float*       tiled_ws  = nullptr;  // split-K workspace of the tiled GEMM (decode steps of 17..768 rows)
    // the decode step's layers as ONE launch of the rows kernel (kernels_rows.hip, paged K/V form): tensor_para_size 1, at most 16
    // slots, page_tokens a multiple of the kernel's attention block (FTCF_BATCHER_ROWS=0: the per-GEMM launches)
    RowsPlan      rplan{};
    bool          use_rows = false;
    char*         rows_ws = nullptr;
    PersistLayer* d_rlayers = nullptr;
    float*        d_rot = nullptr;
    int*          d_rstep = nullptr;
    unsigned      rows_steps = 0;
    size_t       smallm_partial = 0, smallm_region = 0;
    unsigned     smallm_seq = 0;
    long         gemm_steps = 0;
    std::vector<void*> owned;
    // overcommit (batcher_sched.h): the swap space -- `swap_total` host pages of page_all_elems fp16 (one page of every layer of
    // both pools) in ONE pinned region, and the device staging buffer of stage_pages such pages the copies go through
    void*            swap_host = nullptr;
    f16*             swap_stage = nullptr;
    int              stage_pages = 0;
    size_t           page_all_elems = 0;
    int*             d_swap_list = nullptr;
    std::vector<int> swap_list_host, grow_host;
    std::vector<int> pt_host;  // [max_batch][max_pages]: where page-table rows are staged (stage_page_row)
    // Logit processors (kernels_logits.hip): the options and masks of `rows` rows on the device with their host mirrors -- one set
    // indexed by slot for the decode steps, one by the rows of an admission's ragged batch for its first tokens.  The host
    // mirrors are members: an asynchronous copy reads them until the step's synchronisation, and nobody changes them before it.
    struct LogitRows {
        float *            d_pres = nullptr, *d_freq = nullptr, *d_bias_values = nullptr;
        int *              d_min_new = nullptr, *d_gen_start = nullptr, *d_n_bias = nullptr, *d_bias_ids = nullptr, *d_bad = nullptr;
        unsigned*          d_mask = nullptr;
        uint8_t*           d_flags = nullptr;  // [2][rows]: row_on, mask_on
        std::vector<float> pres, freq;
        std::vector<int>   min_new, gen_start, n_bias;
        std::vector<uint8_t> flags, flags_dev;
        int                rows = 0, W = 0;
    };
    LogitRows lp_slots, lp_adm;
    long      logit_launches = 0;  // stages enqueued so far (decode steps and admissions)
    // fork admissions (admit_fork): the prompt's last-row logits as the LM head left them [V], k_batcher_fanout's {slots, tail
    // pages}, the draw counters of the rows the fork's sampling launch is not about, and the host sides of the asynchronous copies
    float*               fork_logits = nullptr;
    int*                 d_fork = nullptr;
    uint64_t*            d_draws_keep = nullptr;
    std::vector<int>     fork_host;
    std::vector<uint8_t> fork_view;
    void init_logit_rows(LogitRows& lr, int rows)
    {
        lr.rows          = rows;
        lr.W             = (e->V + 31) / 32;
        lr.d_pres        = dmalloc<float>(rows);
        lr.d_freq        = dmalloc<float>(rows);
        lr.d_min_new     = dmalloc<int>(rows);
        lr.d_gen_start   = dmalloc<int>(rows);
        lr.d_n_bias      = dmalloc<int>(rows);
        lr.d_bias_ids    = dmalloc<int>((size_t)rows * BIAS_MAX);
        lr.d_bias_values = dmalloc<float>((size_t)rows * BIAS_MAX);
        lr.d_bad         = dmalloc<int>((size_t)rows * 2 * BAD_LW);
        lr.d_mask        = dmalloc<unsigned>((size_t)rows * lr.W);
        lr.d_flags       = dmalloc<uint8_t>(2 * (size_t)rows);
        lr.pres.assign(rows, 0.f);
        lr.freq.assign(rows, 0.f);
        lr.min_new.assign(rows, 0);
        lr.gen_start.assign(rows, 0);
        lr.n_bias.assign(rows, 0);
        lr.flags.assign(2 * (size_t)rows, 0);
        lr.flags_dev = lr.flags;
    }
    // row `i` <- the options (opts given) and / or the mask (mask given) of a request whose generated tokens begin at gen_start
    void stage_logit_row(LogitRows& lr, int i, const LogitOptions* opts, const std::vector<unsigned>* mask, int gen_start, hipStream_t st)
    {
        static const std::vector<int> no_words = [] {
            std::vector<int> w(2 * BAD_LW, -1);
            return w;
        }();
        if (opts) {
            lr.pres[i]      = opts->presence;
            lr.freq[i]      = opts->frequency;
            lr.min_new[i]   = opts->min_new;
            lr.gen_start[i] = gen_start;
            lr.n_bias[i]    = (int)opts->bias_ids.size();
            if (lr.n_bias[i] > 0) {
                FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_bias_ids + (size_t)i * BIAS_MAX, opts->bias_ids.data(), (size_t)lr.n_bias[i] * 4,
                                              hipMemcpyHostToDevice, st));
                FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_bias_values + (size_t)i * BIAS_MAX, opts->bias_values.data(), (size_t)lr.n_bias[i] * 4,
                                              hipMemcpyHostToDevice, st));
            }
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_bad + (size_t)i * 2 * BAD_LW, opts->bad.empty() ? no_words.data() : opts->bad.data(),
                                          (size_t)2 * BAD_LW * 4, hipMemcpyHostToDevice, st));
        }
        if (mask) {
            lr.flags[lr.rows + i] = mask->empty() ? 0 : 1;
            if (!mask->empty()) {
                FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_mask + (size_t)i * lr.W, mask->data(), (size_t)lr.W * 4, hipMemcpyHostToDevice, st));
            }
        }
    }
    // the per-row scalars of rows that changed and the flags when they differ from the device's, then the stage itself
    void enqueue_logit_stage(LogitRows& lr, bool scalars_changed, float* lg, int rows, const uint8_t* finished, const int* hist,
                             long long stride_t, long long stride_b, const int* hist_len, int hist_len_add, hipStream_t st)
    {
        if (scalars_changed) {
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_pres, lr.pres.data(), (size_t)lr.rows * 4, hipMemcpyHostToDevice, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_freq, lr.freq.data(), (size_t)lr.rows * 4, hipMemcpyHostToDevice, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_min_new, lr.min_new.data(), (size_t)lr.rows * 4, hipMemcpyHostToDevice, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_gen_start, lr.gen_start.data(), (size_t)lr.rows * 4, hipMemcpyHostToDevice, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_n_bias, lr.n_bias.data(), (size_t)lr.rows * 4, hipMemcpyHostToDevice, st));
        }
        if (lr.flags != lr.flags_dev) {
            FTCF_HIP_CHECK(hipMemcpyAsync(lr.d_flags, lr.flags.data(), lr.flags.size(), hipMemcpyHostToDevice, st));
            lr.flags_dev = lr.flags;
        }
        LogitProcessParams lp{};
        lp.logits       = lg;
        lp.B            = rows;
        lp.V            = e->V;
        lp.end_id       = e->cfg.end_id;
        lp.finished     = finished;
        lp.row_on       = lr.d_flags;
        lp.hist         = hist;
        lp.stride_t     = stride_t;
        lp.stride_b     = stride_b;
        lp.hist_len     = hist_len;
        lp.gen_start    = lr.d_gen_start;
        lp.hist_len_add = hist_len_add;
        lp.presence     = lr.d_pres;
        lp.frequency    = lr.d_freq;
        lp.min_new      = lr.d_min_new;
        lp.bias_ids     = lr.d_bias_ids;
        lp.bias_values  = lr.d_bias_values;
        lp.n_bias       = lr.d_n_bias;
        lp.bias_stride  = BIAS_MAX;
        lp.bad_words    = lr.d_bad;
        lp.bad_len      = BAD_LW;
        lp.mask         = lr.d_mask;
        lp.mask_on      = lr.d_flags + lr.rows;
        launch_logit_process(lp, st);
        logit_launches++;
    }
    // the decode step's stage: the rows of running ordinary slots with options or a mask (none: nothing is enqueued)
    void enqueue_decode_logit_stage(hipStream_t st)
    {
        bool any = false, scalars = false;
        for (int si = 0; si < max_batch; si++) {
            Slot&      s  = slots[si];
            const bool on = s.active && s.group < 0 && s.processed();
            lp_slots.flags[si] = on ? 1 : 0;
            if (!on) {
                continue;
            }
            any = true;
            if (s.lopt_dirty || s.mask_dirty) {
                stage_logit_row(lp_slots, si, s.lopt_dirty ? &s.lopt : nullptr, s.mask_dirty ? &s.mask : nullptr,
                                (int)s.hist.size() - s.generated, st);
                scalars |= s.lopt_dirty;
                s.lopt_dirty = s.mask_dirty = false;
            }
        }
        if (any) {
            // (the slot's history: column si of d_hist, positions [0, len]; finished rows and the rows of beam groups are not on)
            enqueue_logit_stage(lp_slots, scalars, logits, max_batch, d_fin, d_hist, max_batch, 1, d_len, 1, st);
        }
    }
    static_assert(BIAS_MAX == LOGIT_BIAS_MAX && BAD_LW == LOGIT_BAD_WORDS_MAX, "the scheduler's option limits are the logit stage's");

    template<typename T>
    T* dmalloc(size_t n, bool zero = true)
    {
        void* p = nullptr;
        FTCF_HIP_CHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        if (zero) {
            FTCF_HIP_CHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
        }
        owned.push_back(p);
        return reinterpret_cast<T*>(p);
    }
    ~ftcf_batcher()
    {
        for (void* p : owned) {
            (void)hipFree(p);
        }
        if (swap_host) {
            (void)hipHostFree(swap_host);
        }
    }

    void init(ftcf_gptneox* eng, int mb, int page_tokens, int pages, int max_seq_len, bool prefix_cache = false,
              bool overcommit_on = false, int swap_pages = 0, size_t swap_stage_bytes = 0)
    {
        e = eng;
        FTCF_CHECK_ARG(!overcommit_on || e->cfg.tensor_para_size == 1,
                       "overcommit needs tensor_para_size 1 (every rank would have to swap the same requests: not built)");
        FTCF_CHECK_ARG(swap_pages >= 0, "swap_pages must not be negative");
        FTCF_CHECK_ARG(!prefix_cache
                           || ftcf_gptneox::chunked_supported(e->fp32, e->cfg.tensor_para_size, e->cfg.use_gptj_residual, e->H),
                       "the prefix cache needs an fp16 / int8 engine with tensor_para_size 1, parallel residual and a hidden size "
                       "with the dual LayerNorm (a prompt phase from a token offset)");
        FTCF_CHECK_ARG(!e->fp32 && e->cfg.use_gptj_residual && (e->dh == 64 || e->dh == 128),
                       "the batcher serves fp16 / int8 engines with parallel residual and size_per_head 64 / 128");
        FTCF_CHECK_ARG(mb >= 1 && mb <= 64 && page_tokens >= 8 && pages >= 1 && max_seq_len >= 2, "bad batcher geometry");
        FTCF_HIP_CHECK(hipSetDevice(e->cfg.device));
        if (const char* c = getenv("FTCF_BATCHER_PREFILL_CHUNK")) {
            prefill_chunk = std::max(0, atoi(c));
        }
        init_sched(mb, page_tokens, pages, max_seq_len, e->V, prefix_cache);
        FTCF_CHECK_ARG(mmha_paged_smem_bytes(e->dh, max_pages, max_len) <= 64 * 1024, "max_seq_len too large for the paged attention");
        const int    H = e->H, hl = e->hl, il = e->il, L = e->L, V = e->V;
        const size_t B = (size_t)max_batch;
        pool_layer_elems = (size_t)num_pages * e->nhl * P * e->dh;
        kpool = dmalloc<f16>((size_t)L * pool_layer_elems, false);
        vpool = dmalloc<f16>((size_t)L * pool_layer_elems, false);
        x = dmalloc<f16>(B * H);
        nrm = dmalloc<f16>(B * H);
        nrm2 = dmalloc<f16>(B * H);
        qkv = dmalloc<f16>(B * 3 * hl);
        ctx = dmalloc<f16>(B * hl);
        att = dmalloc<f16>(2 * B * H);  // [att | ffn]: one message for a tensor-parallel layer's all-reduce
        ffn = att + B * H;
        mid = dmalloc<f16>(B * il);
        logits = dmalloc<float>(B * V);
        // tensor parallel (every rank runs its own batcher over its shard, fed the same requests in the same order: the
        // schedulers take identical decisions, the decode step's collectives are the engine's): the LM head's [TP][B][V/TP] slices
        gather = e->cfg.tensor_para_size > 1 ? dmalloc<float>(B * V) : nullptr;
        d_pt = dmalloc<int>(B * max_pages);
        pt_host.assign(B * max_pages, 0);
        d_len = dmalloc<int>(B);
        d_tok = dmalloc<int>(B);
        d_topk = dmalloc<int>(B);
        d_zero = dmalloc<int>(B);
        d_fin = dmalloc<uint8_t>(B);
        d_sfin = dmalloc<uint8_t>(B);
        d_isbeam = dmalloc<uint8_t>(B);
        d_bout = dmalloc<int>(B * (max_len + 2));
        d_bpar = dmalloc<int>(B * (max_len + 2));
        d_bres = dmalloc<int>(B * (max_len + 2));
        d_bres_len = dmalloc<int>(B);
        d_blp = dmalloc<float>(B * (max_len + 2));
        d_bres_lp = dmalloc<float>(B * (max_len + 2));
        d_bseq = dmalloc<int>(B);
        d_bin = dmalloc<int>(B);
        d_pairs = dmalloc<int>(2 * B);
        d_btemp = dmalloc<float>(B);
        d_brep = dmalloc<float>(B);
        d_bdiv = dmalloc<float>(B);
        d_blen = dmalloc<float>(B);
        d_bsw = dmalloc<int>(B * 2 * STOP_LW);
        d_bmin = dmalloc<int>(B);
        d_bstate = dmalloc<DecodeState>(B);
        beam_ws = dmalloc<char>(beam_workspace_bytes(1, std::min(max_batch, BEAM_MAX_K)));
        d_ptopk = dmalloc<float>(B);
        d_ptopp = dmalloc<float>(B);
        d_temp = dmalloc<float>(B);
        d_cum = dmalloc<float>(B);
        d_olp = dmalloc<float>(B);
        d_polp = dmalloc<float>(B);
        d_top_ids = dmalloc<int>(B * TOP_LOGPROBS_MAX);
        d_ptop_ids = dmalloc<int>(B * TOP_LOGPROBS_MAX);
        d_top_lp = dmalloc<float>(B * TOP_LOGPROBS_MAX);
        d_ptop_lp = dmalloc<float>(B * TOP_LOGPROBS_MAX);
        d_rep = dmalloc<float>(B);
        d_hist = dmalloc<int>((size_t)(max_len + 2) * B);
        d_sw = dmalloc<int>(B * 2 * STOP_LW);
        d_seed = dmalloc<uint64_t>(B);
        d_draws = dmalloc<uint64_t>(B);
        d_state = dmalloc<DecodeState>(1);
        d_gstate = dmalloc<DecodeState>(1);
        d_prompt = dmalloc<int>(B * max_seq_len);
        d_plen = dmalloc<int>(B);
        d_pout = dmalloc<int>(B * (max_seq_len + 1));
        d_pseq = dmalloc<int>(B);
        d_pages_tmp = dmalloc<int>(max_pages);
        samp_ws = dmalloc<char>(sampling_workspace_bytes(max_batch, V), false);
        init_logit_rows(lp_slots, max_batch);
        init_logit_rows(lp_adm, max_batch);
        fork_logits  = dmalloc<float>((size_t)V);
        d_fork       = dmalloc<int>(2 * B);
        d_draws_keep = dmalloc<uint64_t>(B);
        init_rows();
        // (tensor parallel: up to 32 slots as two micro-batches of <= 16 rows with their own split-K regions -- the decode overlap)
        if (max_batch > 4 && (max_batch <= e->SMALLM_MAX_ROWS || (e->cfg.tensor_para_size > 1 && max_batch <= 32))) {
            const bool i8 = e->int8;
            const int  bc = std::min(max_batch, 16);  // 16 rows per launch
            smallm_partial = gemm_smallm_workspace_bytes(bc, 3 * hl, H, i8) + gemm_smallm_workspace_bytes(bc, il, H, i8)
                             + gemm_smallm_workspace_bytes(bc, H, hl, i8) + gemm_smallm_workspace_bytes(bc, H, il, i8);
            smallm_region  = smallm_partial;
            smallm_partial *= e->cfg.tensor_para_size > 1 ? 2 : 1;
            smallm_ws = dmalloc<float>((smallm_partial + gemm_smallm_ticket_bytes()) / 4 + 1);
        }
        if (max_batch > 16 && max_batch <= gemm_tiled_splitk_max_m()) {
            tiled_ws = dmalloc<float>(gemm_tiled_workspace_bytes() / 4);
        }
        std::vector<uint8_t> fin(max_batch, 1);
        FTCF_HIP_CHECK(hipMemcpy(d_fin, fin.data(), max_batch, hipMemcpyHostToDevice));
        if (overcommit_on) {
            init_swap(swap_pages, swap_stage_bytes);
        }
    }
    // the rows kernel's plan, workspace and layer table over the pools, where the model, the geometry and FTCF_BATCHER_ROWS allow it
    void init_rows()
    {
        const int H = e->H, hl = e->hl, il = e->il, L = e->L;
        const int rows_env = getenv("FTCF_BATCHER_ROWS") ? atoi(getenv("FTCF_BATCHER_ROWS")) : 1;
        if (rows_env && e->rows && e->cfg.tensor_para_size == 1 && !e->fp32 && max_batch <= 16 && e->cfg.use_gptj_residual && L <= 255
            && (e->dh == 64 || e->dh == 128) && P % rows_paged_block(e->dh) == 0) {
            rplan = rows_plan(max_batch, H, hl, il, e->nhl, e->dh, 1, e->int8, e->num_cu, 0);
            if (rplan.ok && rows_resident(rplan, e->int8, e->dh, e->num_cu, true)) {
                rows_ws   = dmalloc<char>(rows_workspace_bytes(rplan, max_batch, H, hl, il, e->nhl, e->dh));
                d_rlayers = dmalloc<PersistLayer>(L);
                d_rot     = dmalloc<float>((size_t)max_batch * std::max(1, e->cfg.rotary_embedding_dim));
                d_rstep   = dmalloc<int>(1);
                const std::vector<PersistLayer> pl = persist_layer_table(e->layers, kpool, vpool, pool_layer_elems);
                FTCF_HIP_CHECK(hipMemcpy(d_rlayers, pl.data(), sizeof(PersistLayer) * L, hipMemcpyHostToDevice));
                use_rows = true;
            }
        }
    }
    // overcommit: the host pages and the staging buffer
    void init_swap(const int swap_pages, const size_t swap_stage_bytes)
    {
        init_overcommit(swap_pages);
        page_all_elems = 2 * (size_t)e->L * e->nhl * P * e->dh;
        const size_t want = swap_stage_bytes ? swap_stage_bytes : (size_t)64 << 20;
        // at least one page of all layers; no more than one request's pages (nobody swaps more at a time) and than one launch of
        // the copy kernels takes (2^31 16-byte pieces)
        stage_pages = (int)std::min<size_t>(std::max<size_t>(want / (page_all_elems * sizeof(f16)), 1), (size_t)max_pages);
        stage_pages = (int)std::max<size_t>(std::min<size_t>((size_t)stage_pages, (((size_t)1 << 31) - 1) / (page_all_elems / 8)), 1);
        swap_stage  = dmalloc<f16>((size_t)stage_pages * page_all_elems, false);
        d_swap_list = dmalloc<int>(max_pages);
        grow_host.assign(max_batch, 0);
        FTCF_HIP_CHECK(hipHostMalloc(&swap_host, (size_t)swap_total * page_all_elems * sizeof(f16), hipHostMallocDefault));
    }

    struct Event {
        long  id;
        int   token, finished;
        float log_prob = NAN;  // ftcf_batcher_step_ex: the token's log-probability (NaN: a beam request's event)
        // ftcf_batcher_step_top: the step's top_n {id, log-probability} pairs (empty: none were taken -- reported as (-1, NaN))
        std::vector<int>   top_ids;
        std::vector<float> top_lp;
    };
    bool want_log_probs = false;  // inside ftcf_batcher_step_ex: admissions compute their first token's log-probability too
    int  want_top = 0;            // inside ftcf_batcher_step_top: its top_n
    std::vector<Event>* hook_ev = nullptr;  // where the decode steps inside a chunked admission put their events
    std::deque<Event>   outbox;             // events of an iteration that did not fit the caller's arrays
    ftcf_token_callback_fn on_token = nullptr;  // called for every event the moment it exists (inside step())
    void*                  on_token_user = nullptr;
    void emit(std::vector<Event>& ev, const Event& x)
    {
        ev.push_back(x);
        if (on_token) {
            on_token(on_token_user, x.id, x.token, x.finished);
        }
    }

    // the first tokens of an admission reach the callback only when the admission is known to have succeeded: a failed one is
    // rolled back and retried, and a streaming consumer must not see its first tokens twice
    void fire(const std::vector<Event>& ev)
    {
        if (on_token) {
            for (const Event& x : ev) {
                on_token(on_token_user, x.id, x.token, x.finished);
            }
        }
    }

    // the slot's sequence leaves: its pages back to the pool, `finished` set on the device (device_knows: a kernel set it already)
    hipError_t retire(const int si, const bool device_knows = false)
    {
        release(slots[si]);
        const uint8_t one8 = 1;
        return device_knows ? hipSuccess : hipMemcpy(d_fin + si, &one8, 1, hipMemcpyHostToDevice);
    }
    int* pt_row(const int si) const
    {
        return d_pt + (size_t)si * max_pages;
    }
    // slot si's region of the beam arrays d_bout / d_bpar / d_bres (a group's [max_len + 2][K] steps start at its leader's)
    size_t beam_region(const int si) const
    {
        return (size_t)si * (max_len + 2);
    }
    // `rows` page lists as the page-table rows of slots si, si + 1, ... (unused entries: page 0), ONE copy.  The rows are staged
    // in pt_host, a member with a row per slot: an asynchronous copy reads it until the caller's next synchronisation, and
    // every caller synchronises before it returns -- nobody stages a row again while a copy of it is in flight.
    void upload_page_rows(const int si, const std::vector<int>* lists, const int rows, hipStream_t st, const bool blocking = false)
    {
        int* src = pt_host.data() + (size_t)si * max_pages;
        for (int k = 0; k < rows; k++) {
            FTCF_CHECK_ARG(si + k < max_batch && (int)lists[k].size() <= max_pages, "batcher: a page list longer than max_pages");
            std::fill(std::copy(lists[k].begin(), lists[k].end(), src + (size_t)k * max_pages), src + (size_t)(k + 1) * max_pages, 0);
        }
        const size_t bytes = (size_t)rows * max_pages * 4;
        FTCF_HIP_CHECK(blocking ? hipMemcpy(pt_row(si), src, bytes, hipMemcpyHostToDevice)
                                : hipMemcpyAsync(pt_row(si), src, bytes, hipMemcpyHostToDevice, st));
    }
    // the engine's prompt phase from a token offset, for one forward()
    struct PrefillFrom {
        ftcf_gptneox* e;
        PrefillFrom(ftcf_gptneox* eng, int begin, std::function<void()> prefix): e(eng)
        {
            e->prefill_begin  = begin;
            e->prefill_prefix = std::move(prefix);
        }
        ~PrefillFrom()
        {
            e->prefill_begin  = 0;
            e->prefill_prefix = nullptr;
        }
    };

    // the engine's logits hook (engine.hip.h), for one forward(); an empty function leaves the engine as it is
    struct LogitsHook {
        ftcf_gptneox* e;
        LogitsHook(ftcf_gptneox* eng, std::function<void(float*, int, hipStream_t)> fn): e(eng)
        {
            e->logits_hook = std::move(fn);
        }
        ~LogitsHook()
        {
            e->logits_hook = nullptr;
        }
    };

    // The device's per-slot state of the decode steps, from the slot's host fields: length, last token, token history (time-major
    // column si), sampling parameters, seed, and what the caller knows of the device's own counters -- draws made so far and
    // the cumulative log-probability.  A fresh admission and a resume after a swap go through here; the slot is live afterwards
    // (d_fin = 0).  Host synchronous: the temporaries die here.
    void upload_slot_state(const int si, const Slot& s, const uint64_t draws, const float cum, hipStream_t st)
    {
        const int     len = s.len, last = s.hist.back(), k_eff = keff(s.top_k, s.top_p);
        const float   ptk = (s.top_p == 0.f) ? 1.f : s.top_p;
        const uint8_t zero8 = 0;
        FTCF_HIP_CHECK(hipMemcpyAsync(d_len + si, &len, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_tok + si, &last, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_topk + si, &k_eff, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_ptopk + si, &ptk, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_ptopp + si, &s.top_p, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_temp + si, &s.temperature, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_rep + si, &s.repetition_penalty, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpy2DAsync(d_hist + si, (size_t)max_batch * 4, s.hist.data(), 4, 4, s.hist.size(), hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_seed + si, &s.seed, 8, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_draws + si, &draws, 8, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_cum + si, &cum, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_fin + si, &zero8, 1, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
    }

    // ---- overcommit: the device half of a preemption and of a resume (batcher_sched.h: preempt / resume) -------------------------
    char* host_page(const int hp) const
    {
        return reinterpret_cast<char*>(swap_host) + (size_t)hp * page_all_elems * sizeof(f16);
    }
    // staging <-> the host pages host[c0 .. c0 + nc), one linear copy per run of consecutive host pages
    void copy_host_pages(const std::vector<int>& host, const int c0, const int nc, const bool out, hipStream_t st)
    {
        const size_t pb = page_all_elems * sizeof(f16);
        for (int j = 0, run; j < nc; j += run) {
            for (run = 1; j + run < nc && host[c0 + j + run] == host[c0 + j] + run;) {
                run++;
            }
            char* dev = reinterpret_cast<char*>(swap_stage) + (size_t)j * pb;
            FTCF_CHECK_ARG(host[c0 + j] >= 0 && host[c0 + j] + run <= swap_total, "batcher: a host page outside the swap space");
            if (out) {
                FTCF_HIP_CHECK(hipMemcpyAsync(host_page(host[c0 + j]), dev, (size_t)run * pb, hipMemcpyDeviceToHost, st));
            }
            else {
                FTCF_HIP_CHECK(hipMemcpyAsync(dev, host_page(host[c0 + j]), (size_t)run * pb, hipMemcpyHostToDevice, st));
            }
        }
    }
    void upload_swap_list(const std::vector<int>& pages, hipStream_t st)
    {
        FTCF_CHECK_ARG((int)pages.size() <= max_pages, "batcher: a page list longer than max_pages");
        for (const int pg : pages) {
            FTCF_CHECK_ARG(pg >= 0 && pg < num_pages, "batcher: a page outside the pool");
        }
        swap_list_host = pages;  // (a member: the asynchronous copy reads it until the synchronisation that ends the swap)
        FTCF_HIP_CHECK(hipMemcpyAsync(d_swap_list, swap_list_host.data(), pages.size() * 4, hipMemcpyHostToDevice, st));
    }
    // every page of the victim's list -> its host pages, in chunks of whole pages through the staging buffer (k_pages_pack, then
    // the linear copy; stream order alone keeps a chunk's pack behind the previous chunk's copy); the draw counter and the
    // cumulative log-probability come back with the same synchronisation; the device learns the slot is finished
    void swap_out_dev(const int si, const std::vector<int>& pages, const std::vector<int>& host, uint64_t& draws, float& cum)
    {
        Range       rg("ftcf.batcher.swap_out");
        hipStream_t st = e->stream;
        const int   n  = (int)pages.size();
        FTCF_CHECK_ARG(host.size() == pages.size(), "batcher: a victim's host pages do not match its page list");
        upload_swap_list(pages, st);
        for (int c0 = 0; c0 < n; c0 += stage_pages) {
            const int nc = std::min(stage_pages, n - c0);
            launch_pages_pack(swap_stage, kpool, vpool, d_swap_list + c0, nc, e->L, page_all_elems / (2 * (size_t)e->L), pool_layer_elems, st);
            copy_host_pages(host, c0, nc, true, st);
        }
        const uint8_t one8 = 1;
        FTCF_HIP_CHECK(hipMemcpyAsync(&draws, d_draws + si, 8, hipMemcpyDeviceToHost, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(&cum, d_cum + si, 4, hipMemcpyDeviceToHost, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_fin + si, &one8, 1, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
    }
    // the reverse into the first pages of the slot's fresh list (k_pages_unpack), then the slot's page table row and its state
    // through the function an admission uses
    void swap_in_dev(const int si, const Swapped& w, const std::vector<int>& pages)
    {
        Range       rg("ftcf.batcher.swap_in");
        hipStream_t st = e->stream;
        const int   n  = (int)w.host.size();
        FTCF_CHECK_ARG(n <= (int)pages.size(), "batcher: a resumed request has more host pages than its new page list");
        upload_swap_list(pages, st);
        for (int c0 = 0; c0 < n; c0 += stage_pages) {
            const int nc = std::min(stage_pages, n - c0);
            copy_host_pages(w.host, c0, nc, false, st);
            launch_pages_unpack(swap_stage, kpool, vpool, d_swap_list + c0, nc, e->L, page_all_elems / (2 * (size_t)e->L), pool_layer_elems, st);
        }
        upload_page_rows(si, &pages, 1, st);
        upload_slot_state(si, slots[si], w.draws, w.cum, st);  // (host synchronous)
    }
    // before a decode step enqueues anything: the slots whose next token starts a page take it (preempting when the pool has
    // none); their page table rows get the new entry
    void grow_before_decode(hipStream_t st)
    {
        try {
            grow_slots(
                [this](int si, const std::vector<int>& pages, const std::vector<int>& host, uint64_t& draws, float& cum) {
                    swap_out_dev(si, pages, host, draws, cum);
                },
                // ONE growth: the row's new last entry goes up the moment the host has handed the page out, so that a failure at a
                // later slot ("swap space exhausted", a HIP error of a swap-out) leaves no page the device does not know of
                [this, st](int si) {
                    const int k = (int)slots[si].pages.size() - 1;
                    FTCF_CHECK_ARG(k >= 0 && k < max_pages && slots[si].pages[k] >= 0 && slots[si].pages[k] < num_pages,
                                   "batcher: a page list outgrew max_pages");
                    grow_host[si] = slots[si].pages[k];  // (a member: read by the copy until the step's synchronisation)
                    FTCF_HIP_CHECK(hipMemcpyAsync(pt_row(si) + k, &grow_host[si], 4, hipMemcpyHostToDevice, st));
                });
        }
        catch (...) {
            (void)hipStreamSynchronize(st);  // (no decode step follows: the entries already enqueued land before the caller goes on)
            throw;
        }
    }

    // slot i's top_n {id, log-probability} pairs out of a step's [rows][top_n] arrays
    static void cut_top(Event& x, const std::vector<int>& ids, const std::vector<float>& lp, const int i, const int top_n)
    {
        x.top_ids.assign(ids.begin() + (size_t)i * top_n, ids.begin() + (size_t)(i + 1) * top_n);
        x.top_lp.assign(lp.begin() + (size_t)i * top_n, lp.begin() + (size_t)(i + 1) * top_n);
    }

    // ONE ragged batch of prompts for the engine's context path: the engine's arguments and the host arrays they point into
    struct AdmitBatch {
        int                   n = 0, S = 0, hit_tokens = 0, top_n = 0;
        std::vector<int>      lens, topk;
        std::vector<float>    topp, temp, rep;
        std::vector<uint64_t> seed;
        bool                  any_lp = false;  // a row has logit processors: the stage runs as the engine's logits hook
        float*                capture = nullptr;  // a fork's one row: its logits [V] go here before anything touches them
        ftcf_forward_args     a{};
    };
    // the first n of rs into the first n of sis: their pages, the ragged batch on the device, the engine's arguments, the logit
    // rows of the first tokens
    // hit (one request only): the cached pages of its first prompt blocks (pinned here: the slot's page list owns one reference)
    // take_pages = false (a fork's one row): the slots have their pages already (take_fork_pages)
    void build_admission(AdmitBatch& b, const std::vector<int>& sis, const std::vector<Request>& rs, const int n,
                         const std::vector<int>* hit, hipStream_t st, const bool take_pages = true)
    {
        int S = 0;
        for (int i = 0; i < n; i++) {
            S = std::max(S, (int)rs[i].prompt.size());
        }
        b.n          = n;
        b.S          = S;
        b.hit_tokens = hit ? (int)hit->size() * P : 0;
        b.top_n      = want_top;
        std::vector<int>&      lens = b.lens;
        std::vector<int>       ids((size_t)n * S, e->cfg.end_id), sw((size_t)n * 2 * STOP_LW, 0);
        bool                   any_stop = false;
        lens.resize(n), b.topk.resize(n), b.topp.resize(n), b.temp.resize(n), b.rep.resize(n), b.seed.resize(n);
        for (int i = 0; i < n; i++) {
            const Request& r = rs[i];
            std::copy(r.prompt.begin(), r.prompt.end(), ids.begin() + (size_t)i * S);
            lens[i]   = (int)r.prompt.size();
            b.topk[i] = r.top_k;
            b.topp[i] = r.top_p;
            b.temp[i] = r.temperature;
            b.rep[i]  = r.repetition_penalty;
            b.seed[i] = r.seed;
            // the request's stop sequences in the reference's word-list layout (the engine samples the FIRST token)
            build_word_list(r.stop, sw.data() + (size_t)i * 2 * STOP_LW);
            any_stop |= !r.stop.empty();
            FTCF_CHECK_ARG(!hit || n == 1, "batcher: a prefix hit is admitted alone");
            if (take_pages) {
                take_slot_pages(sis[i], r, hit);
            }
        }
        FTCF_HIP_CHECK(hipMemcpy(d_prompt, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
        FTCF_HIP_CHECK(hipMemcpy(d_plen, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        ftcf_forward_args& a = b.a;
        a.input_ids = d_prompt;
        a.input_lengths = d_plen;
        a.batch_size = n;
        a.max_input_len = S;
        a.output_len = 1;
        a.beam_width = 1;
        a.top_k = b.topk.data();
        a.n_top_k = n;
        a.top_p = b.topp.data();
        a.n_top_p = n;
        a.temperature = b.temp.data();
        a.n_temperature = n;
        a.repetition_penalty = b.rep.data();
        a.n_repetition_penalty = n;
        if (any_stop) {
            FTCF_HIP_CHECK(hipMemcpy(d_sw, sw.data(), sw.size() * 4, hipMemcpyHostToDevice));
            a.stop_words_list = d_sw;
            a.stop_words_len = STOP_LW;
        }
        a.random_seed = b.seed.data();
        a.n_random_seed = n;
        a.output_ids = d_pout;
        a.sequence_lengths = d_pseq;
        if (want_log_probs) {  // (the engine then runs the soft-max statistics as return_cum_log_probs = 1 does: the decode steps' setting)
            a.output_log_probs = d_polp;
        }
        if (b.top_n > 0) {
            a.top_logprobs       = b.top_n;
            a.top_logprob_ids    = d_ptop_ids;  // [n, 1, 1, top_n]
            a.top_logprob_values = d_ptop_lp;
        }
        // the first tokens' logit processors: the rows' options and masks by row of this batch (history = the padded prompt
        // rows, nothing generated yet)
        for (int i = 0; i < n; i++) {
            const bool on = rs[i].lopt.any() || !rs[i].mask.empty();
            lp_adm.flags[i] = on ? 1 : 0;
            if (on) {
                stage_logit_row(lp_adm, i, &rs[i].lopt, &rs[i].mask, lens[i], st);
                b.any_lp = true;
            }
        }
    }
    // the prompt phase (host synchronous: K/V of row i, positions [0, len_i), are in the engine's cache [L][n][nh][S + 1][dh]
    // afterwards), from the first uncached token when slot si0's request had a prefix hit
    void prompt_phase(const AdmitBatch& b, const int si0)
    {
        const int  n = b.n, S = b.S, hit_tokens = b.hit_tokens;
        float* const capture = b.capture;
        const bool   any_lp  = b.any_lp;
        LogitsHook first_logits(e, (any_lp || capture) ? std::function<void(float*, int, hipStream_t)>([this, n, S, capture, any_lp](float* lg, int rows, hipStream_t s2) {
            FTCF_CHECK_ARG(rows == n, "batcher: the engine's first step has other rows than the admission");
            if (capture) {
                FTCF_HIP_CHECK(hipMemcpyAsync(capture, lg, (size_t)e->V * sizeof(float), hipMemcpyDeviceToDevice, s2));
            }
            if (any_lp) {
                enqueue_logit_stage(lp_adm, true, lg, n, nullptr, d_prompt, 1, S, d_plen, 0, s2);
            }
        }) : nullptr);
        if (hit_tokens == 0) {
            e->forward(b.a);
            return;
        }
        // first the cached pages go to cache row 0 (the engine's cache exists only inside forward(): the gather is its
        // prefill_prefix hook)
        upload_page_rows(si0, &slots[si0].pages, 1, e->stream, true);
        PrefillFrom from(e, hit_tokens, [this, si0, S, hit_tokens] {
            launch_gather_pages_to_kv(e->k_cache, e->v_cache, kpool, vpool, pt_row(si0), e->L, e->nhl, e->dh, S + 1, hit_tokens, P,
                                      pool_layer_elems, e->stream);
        });
        e->forward(b.a);
    }
    // the first tokens (with what the step asked for: log-probabilities, top-N pairs) and, per request, the prompt's K/V into
    // the slot's pages and the slot's state
    void install_admitted(const AdmitBatch& b, const std::vector<int>& sis, const std::vector<Request>& rs, std::vector<Event>& ev,
                          hipStream_t st)
    {
        const int        n = b.n, S = b.S, hit_tokens = b.hit_tokens, top_n = b.top_n;
        std::vector<int> out((size_t)n * (S + 1));
        FTCF_HIP_CHECK(hipMemcpy(out.data(), d_pout, out.size() * 4, hipMemcpyDeviceToHost));
        std::vector<float> first_lp((size_t)n, NAN);
        if (b.a.output_log_probs) {
            FTCF_HIP_CHECK(hipMemcpy(first_lp.data(), d_polp, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
        std::vector<int>   first_top_ids((size_t)n * top_n);
        std::vector<float> first_top_lp((size_t)n * top_n);
        if (top_n > 0) {
            FTCF_HIP_CHECK(hipMemcpy(first_top_ids.data(), d_ptop_ids, first_top_ids.size() * 4, hipMemcpyDeviceToHost));
            FTCF_HIP_CHECK(hipMemcpy(first_top_lp.data(), d_ptop_lp, first_top_lp.size() * 4, hipMemcpyDeviceToHost));
        }
        const size_t row_kv = (size_t)e->nhl * (S + 1) * e->dh;  // one row of one layer of the engine's cache
        for (int i = 0; i < n; i++) {
            const Request& r  = rs[i];
            const int      si = sis[i], len = b.lens[i];
            Slot&          s  = slots[si];
            // the engine's output rows are compacted (prompt, then the generated tokens: invokeGatherTree removes the padding)
            const int first = out[(size_t)i * (S + 1) + len];
            upload_page_rows(si, &s.pages, 1, st);
            // (a hit: only the tail's pages; the cached ones are immutable)
            launch_scatter_kv_to_pages(e->k_cache + (size_t)i * row_kv + (size_t)hit_tokens * e->dh,
                                       e->v_cache + (size_t)i * row_kv + (size_t)hit_tokens * e->dh, kpool, vpool,
                                       pt_row(si) + hit_tokens / P, e->L, e->nhl, e->dh, S + 1, len - hit_tokens, P, pool_layer_elems, st,
                                       (size_t)n * row_kv);
            // per-slot state of the decode steps: the history is prompt, then the first token; draw 0 went to the first token
            const int done = start_slot(si, r, first, e->cfg.end_id) ? 1 : 0;
            upload_slot_state(si, s, 1, 0.f, st);
            ev.push_back(Event{r.id, first, done, first_lp[i]});  // (the token callback fires when the admission has succeeded: step())
            cut_top(ev.back(), first_top_ids, first_top_lp, i, top_n);
            if (done) {
                const uint8_t one8 = 1;
                FTCF_HIP_CHECK(hipMemcpy(d_fin + si, &one8, 1, hipMemcpyHostToDevice));
                end_with_first_token(si);  // (prefix cache: its prompt pages are inserted first, commit())
            }
        }
    }
    // prompts -> ONE ragged batch through the engine's context path (+ first tokens) -> pages of their slots
    void admit(const std::vector<int>& sis, const std::vector<Request>& rs, const int n, std::vector<Event>& ev,
               const std::vector<int>* hit = nullptr)
    {
        Range rg("ftcf.batcher.admit");
        deferred.clear();
        AdmitBatch b;
        build_admission(b, sis, rs, n, hit, e->stream);
        prompt_phase(b, sis[0]);
        install_admitted(b, sis, rs, ev, e->stream);
    }

    // ---- fork requests (submit_n) ----------------------------------------------------------------------------------------
    // ONE prompt phase for n siblings (batcher_sched.h: take_fork_pages).  The prompt runs as a batch of one greedy row whose own
    // token nobody uses; the logits hook keeps its last-row logits.  Sibling 0's pages are filled from the engine's cache as any
    // admission's; k_batcher_fanout copies the logits into the siblings' rows of the step's logits buffer and the prompt's tail
    // rows into the other siblings' first own pages.  The n first tokens are then drawn by the stages a decode step runs -- the
    // logit processors and the sampling kernels over the slots' rows -- with every sibling's slot set up as the plain request
    // of seed + index BEFORE its first draw: length len - 1 (the engine's own convention: launch_decode_init), history = the
    // prompt, draw counter 0, cumulative log-probability 0.  Every other row is finished in that launch's view (d_sfin); the top-p
    // kernel draws for finished rows too, so the draw counters of those rows are put back.
    void admit_fork(const std::vector<int>& sis, const Request& r, std::vector<Event>& ev, const std::vector<int>* hit)
    {
        Range       rg("ftcf.batcher.admit_fork");
        hipStream_t st = e->stream;
        const int   n = r.n_samples, S = (int)r.prompt.size(), shared = fork_shared_pages(r), tail = S % P, top_n = want_top;
        const int   hit_tokens = hit ? (int)hit->size() * P : 0;
        FTCF_CHECK_ARG(n >= 1 && (int)sis.size() == n && (int)r.sibs.size() == n, "batcher: a fork admission's slots are not its siblings'");
        deferred.clear();
        take_fork_pages(sis, r, hit);
        std::vector<Request> one(1, r);
        Request&             r0 = one[0];
        r0.top_k = 0, r0.top_p = 0.f, r0.temperature = 1.f, r0.repetition_penalty = 1.f, r0.seed = 0;
        r0.stop.clear(), r0.mask.clear(), r0.sibs.clear();
        r0.lopt = LogitOptions{};
        AdmitBatch b;
        b.capture = fork_logits;
        build_admission(b, sis, one, 1, hit, st, false);
        prompt_phase(b, sis[0]);  // (host synchronous)
        // the page table rows; sibling 0's pages from the engine's cache (a hit: the tail's pages only)
        fork_host.assign(2 * (size_t)n, 0);
        for (int i = 0; i < n; i++) {
            const std::vector<int>& pages = slots[sis[i]].pages;
            FTCF_CHECK_ARG(sis[i] >= 0 && sis[i] < max_batch && (int)pages.size() > shared && (int)pages.size() * P > S,
                           "batcher: a sibling without a page of its own");
            for (const int pg : pages) {
                FTCF_CHECK_ARG(pg >= 0 && pg < num_pages, "batcher: a page outside the pool");
            }
            upload_page_rows(sis[i], &pages, 1, st);
            fork_host[i]     = sis[i];
            fork_host[n + i] = pages[shared];
        }
        const size_t row_kv = (size_t)e->nhl * (S + 1) * e->dh;
        launch_scatter_kv_to_pages(e->k_cache + (size_t)hit_tokens * e->dh, e->v_cache + (size_t)hit_tokens * e->dh, kpool, vpool,
                                   pt_row(sis[0]) + hit_tokens / P, e->L, e->nhl, e->dh, S + 1, S - hit_tokens, P, pool_layer_elems, st, row_kv);
        FTCF_HIP_CHECK(hipMemcpyAsync(d_fork, fork_host.data(), fork_host.size() * 4, hipMemcpyHostToDevice, st));
        const unsigned gx = (unsigned)std::min(64, std::max((e->V + 1023) / 1024, (e->nhl + 3) / 4));
        const unsigned gy = 1u + (tail > 0 ? (unsigned)(n - 1) * (unsigned)e->L * 2u : 0u);
        FTCF_CHECK_ARG(gy <= 65535u && e->dh % 8 == 0, "batcher: a fork of too many siblings and layers for one launch");
        hipLaunchKernelGGL(k_batcher_fanout, dim3(gx, gy), dim3(256), 0, st, logits, fork_logits, e->V, kpool, vpool, d_fork, n, e->L, e->nhl,
                           P, e->dh, tail, pool_layer_elems);
        FTCF_HIP_CHECK(hipGetLastError());
        // every sibling's slot before its first draw; the launch's view of `finished`; its flags are the siblings' alone
        FTCF_HIP_CHECK(hipMemcpyAsync(d_draws_keep, d_draws, (size_t)max_batch * 8, hipMemcpyDeviceToDevice, st));
        fork_view.assign(max_batch, 1);
        std::fill(lp_slots.flags.begin(), lp_slots.flags.begin() + max_batch, 0);
        bool any_lp = false;
        for (int i = 0; i < n; i++) {
            const Request::Sibling& sb = r.sibs[i];
            Slot                    t;
            t.len                = S - 1;
            t.hist               = r.prompt;
            t.top_k              = r.top_k;
            t.top_p              = r.top_p;
            t.temperature        = r.temperature;
            t.repetition_penalty = r.repetition_penalty;
            t.seed               = r.seed + (uint64_t)sb.index;
            upload_slot_state(sis[i], t, 0, 0.f, st);
            fork_view[sis[i]] = 0;
            if (r.lopt.any() || !sb.mask.empty()) {
                lp_slots.flags[sis[i]] = 1;
                stage_logit_row(lp_slots, sis[i], &r.lopt, &sb.mask, S, st);
                any_lp = true;
            }
        }
        FTCF_HIP_CHECK(hipMemcpyAsync(d_sfin, fork_view.data(), (size_t)max_batch, hipMemcpyHostToDevice, st));
        host_max_top_k       = keff(r.top_k, r.top_p);
        host_any_top_p       = host_max_top_k == 0 ? 1 : 0;
        host_max_top_k       = std::max(host_max_top_k, 1);
        host_any_temperature = r.temperature != 1.f;
        host_any_repetition  = r.repetition_penalty != 1.f;
        if (any_lp) {
            enqueue_logit_stage(lp_slots, true, logits, max_batch, d_sfin, d_hist, max_batch, 1, d_len, 1, st);
        }
        SamplingParams sp = sampling_params();
        sp.finished       = d_sfin;
        DynamicDecodeLayer{}.forward(sp, st, false);
        FTCF_HIP_CHECK(hipMemcpyAsync(d_draws, d_draws_keep, (size_t)max_batch * 8, hipMemcpyDeviceToDevice, st));
        // the first tokens (position len of every slot's history column) with what the step asked for
        const size_t       B = (size_t)max_batch;
        std::vector<int>   tok(B), top_ids(B * top_n);
        std::vector<float> lp(B, NAN), top_lp(B * top_n);
        FTCF_HIP_CHECK(hipMemcpyAsync(tok.data(), d_hist + (size_t)S * B, B * 4, hipMemcpyDeviceToHost, st));
        if (want_log_probs) {
            FTCF_HIP_CHECK(hipMemcpyAsync(lp.data(), d_olp, B * 4, hipMemcpyDeviceToHost, st));
        }
        if (top_n > 0) {
            FTCF_HIP_CHECK(hipMemcpyAsync(top_ids.data(), d_top_ids, top_ids.size() * 4, hipMemcpyDeviceToHost, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(top_lp.data(), d_top_lp, top_lp.size() * 4, hipMemcpyDeviceToHost, st));
        }
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
        // from here on every sibling is an ordinary sequence: its slot as install_admitted leaves one, n events in sibling order
        for (int i = 0; i < n; i++) {
            const int     si = sis[i], first = tok[si];
            const Request q  = sibling_request(r, r.sibs[i]);
            FTCF_CHECK_ARG(first >= 0 && first < e->V, "batcher: a sibling's first token is outside the vocabulary");
            const int done = start_slot(si, q, first, e->cfg.end_id) ? 1 : 0;
            upload_slot_state(si, slots[si], 1, 0.f, st);
            ev.push_back(Event{q.id, first, done, lp[si]});
            cut_top(ev.back(), top_ids, top_lp, si, top_n);
            if (done) {
                const uint8_t one8 = 1;
                FTCF_HIP_CHECK(hipMemcpy(d_fin + si, &one8, 1, hipMemcpyHostToDevice));
                end_with_first_token(si);
            }
        }
    }

    // ---- beam groups ------------------------------------------------------------------------------------------------
    void upload_group_tables(const BeamGroup& g, hipStream_t st)
    {
        upload_page_rows(g.si, g.lists.data(), g.K, st);
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
    }
    // every unfinished beam gets a page of its OWN for position `pos` (the next append): a fresh one on a page boundary, a copy
    // of the shared one otherwise
    void prepare_append(BeamGroup& g, const int pos, const std::vector<uint8_t>& fin, hipStream_t st)
    {
        const std::vector<int> pairs = take_append_pages(g, pos, fin);
        if (!pairs.empty()) {
            FTCF_HIP_CHECK(hipMemcpyAsync(d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, st));
            const size_t page_elems = (size_t)e->nhl * P * e->dh;
            hipLaunchKernelGGL(k_batcher_copy_pages, dim3((unsigned)pairs.size() / 2, e->L, 2), dim3(256), 0, st, kpool, vpool, d_pairs,
                               page_elems, pool_layer_elems);
            FTCF_HIP_CHECK(hipGetLastError());
            FTCF_HIP_CHECK(hipStreamSynchronize(st));
        }
        upload_group_tables(g, st);
    }
    void release_group(const int si)
    {
        const int K = drop_group(si);
        if (K == 0) {
            return;
        }
        std::vector<uint8_t> ones(K, 1), zeros(K, 0);
        (void)hipMemcpy(d_fin + si, ones.data(), K, hipMemcpyHostToDevice);
        (void)hipMemcpy(d_isbeam + si, zeros.data(), K, hipMemcpyHostToDevice);
    }
    // gatherTree over the group's steps (decoding_kernels.cu:452-583, as GptNeoXOp.forward returns its beams: [K][n + max_new]
    // ids padded with end_id, lengths, cum_log_probs), the result parked until it is fetched, the slots and pages freed
    // fire_now = false (from inside an admission): the event is only recorded, step() fires it once the admission has succeeded
    void finish_group(const int si, std::vector<Event>& ev, const bool fire_now = true)
    {
        BeamGroup&  g = groups.at(si);
        hipStream_t st = e->stream;
        const int   total = g.n + g.max_new;
        const size_t reg  = beam_region(si);
        launch_gather_tree_beam(d_bres + reg, d_bres_len + si, d_bout + reg, d_bpar + reg, d_bseq + si, d_bin + si, 1, g.K, g.n, total,
                                e->cfg.end_id, st);
        BeamResult r;
        r.K     = g.K;
        r.total = total;
        r.ids.resize((size_t)g.K * total);
        r.lens.resize(g.K);
        r.cum.resize(g.K);
        FTCF_HIP_CHECK(hipMemcpyAsync(r.ids.data(), d_bres + reg, r.ids.size() * 4, hipMemcpyDeviceToHost, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(r.lens.data(), d_bres_len + si, (size_t)g.K * 4, hipMemcpyDeviceToHost, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(r.cum.data(), d_cum + si, (size_t)g.K * 4, hipMemcpyDeviceToHost, st));
        if (g.token_log_probs) {  // (only a request that asked pays the walk and the copy)
            launch_gather_tree_beam_log_probs(d_bres_lp + reg, d_blp + reg, d_bout + reg, d_bpar + reg, d_bseq + si, d_bin + si, 1, g.K,
                                              g.n, total, e->cfg.end_id, st);
            r.has_lp = true;
            r.lp.resize((size_t)g.K * g.max_new);
            FTCF_HIP_CHECK(hipMemcpyAsync(r.lp.data(), d_bres_lp + reg, r.lp.size() * 4, hipMemcpyDeviceToHost, st));
        }
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
        const long id    = g.id;
        beam_results[id] = std::move(r);
        while (beam_results.size() > 256) {  // (results nobody fetches do not pile up: the oldest ids go first)
            FT_LOG_WARNING(e->cfg.device, "batcher: the result of beam request %ld was never fetched and is dropped (256 wait at most)",
                           beam_results.begin()->first);
            beam_results.erase(beam_results.begin());
        }
        release_group(si);
        if (fire_now) {
            emit(ev, Event{id, -1, 1});
        }
        else {
            ev.push_back(Event{id, -1, 1});
        }
    }
    static bool all_finished(const std::vector<uint8_t>& fin)
    {
        return std::all_of(fin.begin(), fin.end(), [](uint8_t f) { return f != 0; });
    }
    // a group whose beams' flags after a step are `fin`: it leaves when every beam has finished or its budget is used up, else
    // its beams get their pages for the next append
    void finish_or_append(BeamGroup& g, const std::vector<uint8_t>& fin, std::vector<Event>& ev, const bool fire_now)
    {
        if (all_finished(fin) || g.generated >= g.max_new) {
            finish_group(g.si, ev, fire_now);
        }
        else {
            prepare_append(g, g.n + g.generated - 1, fin, e->stream);
        }
    }
    // prompt -> the engine's own beam-search request of ONE step (prefill of the K tiled rows, first beam step) -> the group's
    // state; the prompt's K/V are scattered once (beam 0's rows) into pages all beams share
    void admit_beam(const int si, const Request& r, std::vector<Event>& ev)
    {
        Range       rg("ftcf.batcher.admit_beam");
        hipStream_t st = e->stream;
        const int   K = r.beam_width, n = (int)r.prompt.size();
        const bool  has_min = r.min_length > 0, has_stop = !r.stop.empty();
        FTCF_HIP_CHECK(hipMemcpy(d_prompt, r.prompt.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        FTCF_HIP_CHECK(hipMemcpy(d_plen, &n, 4, hipMemcpyHostToDevice));
        ftcf_forward_args a{};
        a.input_ids = d_prompt;
        a.input_lengths = d_plen;
        a.batch_size = 1;
        a.max_input_len = n;
        a.output_len = 1;
        a.beam_width = K;
        a.temperature = &r.temperature;
        a.n_temperature = 1;
        a.repetition_penalty = &r.repetition_penalty;
        a.n_repetition_penalty = 1;
        a.beam_search_diversity_rate = &r.diversity;
        a.n_beam_search_diversity_rate = 1;
        a.len_penalty = &r.len_penalty;
        a.n_len_penalty = 1;
        a.output_ids = d_pout;
        a.sequence_lengths = d_pseq;
        if (has_min) {
            a.min_length = &r.min_length;
            a.n_min_length = 1;
            FTCF_HIP_CHECK(hipMemcpy(d_bmin + si, &r.min_length, 4, hipMemcpyHostToDevice));
        }
        if (has_stop) {  // the group's stop words stay on the device for its beam steps (checked along the parent chain there)
            std::vector<int> sw(2 * STOP_LW);
            build_word_list(r.stop, sw.data());
            FTCF_HIP_CHECK(hipMemcpy(d_bsw + (size_t)si * 2 * STOP_LW, sw.data(), sw.size() * 4, hipMemcpyHostToDevice));
            a.stop_words_list = d_bsw + (size_t)si * 2 * STOP_LW;
            a.stop_words_len = STOP_LW;
        }
        e->forward(a);  // host synchronous; the engine's buffers keep the request's state: step_ids / parent_ids [n + 1][K], ...
        BeamGroup& G = open_group(si, r);  // the prompt's pages, shared by every beam
        upload_group_tables(G, st);
        const size_t row_kv = (size_t)e->nhl * (n + 1) * e->dh;
        launch_scatter_kv_to_pages(e->k_cache, e->v_cache, kpool, vpool, pt_row(si), e->L, e->nhl, e->dh, n + 1, n, P, pool_layer_elems, st,
                                   (size_t)K * row_kv);
        const std::vector<uint8_t> fin = upload_group_state(si, r, st);
        start_group_slots(G);
        finish_or_append(G, fin, ev, false);  // (a group that leaves at once: step() fires its event when the admission has succeeded)
    }
    // the state of a group's K slots after the engine's first beam step, out of the engine's buffers and the request; returns the
    // beams' finished flags
    std::vector<uint8_t> upload_group_state(const int si, const Request& r, hipStream_t st)
    {
        const int    K = r.beam_width, n = (int)r.prompt.size();
        const size_t reg = beam_region(si);
        FTCF_HIP_CHECK(hipMemcpyAsync(d_bout + reg, e->step_ids, (size_t)(n + 1) * K * 4, hipMemcpyDeviceToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_bpar + reg, e->parent_ids, (size_t)(n + 1) * K * 4, hipMemcpyDeviceToDevice, st));
        // the first step's log-probabilities (row n; the prompt's rows are 0), and 0 in the rows the group's own steps may not reach
        FTCF_HIP_CHECK(hipMemcpyAsync(d_blp + reg, e->step_log_probs, (size_t)(n + 1) * K * 4, hipMemcpyDeviceToDevice, st));
        FTCF_HIP_CHECK(hipMemsetAsync(d_blp + reg + (size_t)(n + 1) * K, 0, (size_t)(max_len + 2 - (n + 1)) * K * 4, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_bseq + si, e->seq_len, (size_t)K * 4, hipMemcpyDeviceToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_cum + si, e->cum, (size_t)K * 4, hipMemcpyDeviceToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_tok + si, e->step_ids + (size_t)n * K, (size_t)K * 4, hipMemcpyDeviceToDevice, st));
        // (the engine's own `finished` is all ones by now: its one-token request ran into the length criterion)
        std::vector<int>     lens(K, n), first(K);
        std::vector<uint8_t> ones(K, 1), fin(K, 0);
        FTCF_HIP_CHECK(hipMemcpy(first.data(), e->step_ids + (size_t)n * K, (size_t)K * 4, hipMemcpyDeviceToHost));
        std::vector<int> hist(r.prompt);  // (stop_criteria_kernels.cu:24-83 on prompt + first token: every beam's parent is the prompt)
        hist.push_back(0);
        for (int k = 0; k < K; k++) {
            hist.back() = first[k];
            fin[k]      = (first[k] == e->cfg.end_id || ends_with_stop(r.stop, hist)) ? 1 : 0;
        }
        FTCF_HIP_CHECK(hipMemcpyAsync(d_fin + si, fin.data(), (size_t)K, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_len + si, lens.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_bin + si, lens.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_isbeam + si, ones.data(), (size_t)K, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_btemp + si, &r.temperature, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_brep + si, &r.repetition_penalty, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_bdiv + si, &r.diversity, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(d_blen + si, &r.len_penalty, 4, hipMemcpyHostToDevice, st));
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
        return fin;
    }
    // the beam kernels of every running group on this step's logits, BEFORE the sampling kernels (whose end-id mask rewrites the
    // logits of rows that are finished in their view -- the groups' rows)
    void enqueue_beam_steps(hipStream_t st)
    {
        for (auto& kv : groups) {
            BeamGroup&   g   = kv.second;
            const int    si  = g.si, step = g.n + g.generated;
            const size_t reg = beam_region(si);
            hipLaunchKernelGGL(k_batcher_set_step, dim3(1), dim3(1), 0, st, d_bstate + si, step);
            BeamParams bp{};
            bp.logits = logits + (size_t)si * e->V;
            bp.B = 1;
            bp.K = g.K;
            bp.V = e->V;
            bp.max_input_len = g.n;
            bp.total_len = max_len + 2;
            bp.end_id = e->cfg.end_id;
            bp.s_max = 0;  // (no cache indirection: the page lists are reordered instead)
            bp.input_lengths = d_bin + si;
            bp.temperature = d_btemp + si;
            bp.repetition_penalty = g.penalised ? d_brep + si : nullptr;  // (NULL: no history staging buffer in LDS)
            bp.diversity_rate = d_bdiv + si;
            bp.len_penalty = d_blen + si;
            bp.min_length = g.has_min ? d_bmin + si : nullptr;
            bp.stop_words = g.has_stop ? d_bsw + (size_t)si * 2 * STOP_LW : nullptr;
            bp.stop_len = STOP_LW;
            bp.output_ids = d_bout + reg;
            bp.parent_ids = d_bpar + reg;
            bp.finished = d_fin + si;
            bp.seq_len = d_bseq + si;
            bp.cum_log_probs = d_cum + si;
            bp.step_log_probs = d_blp + reg;
            bp.cache_indir = d_zero;
            bp.state = d_bstate + si;
            bp.ws = beam_ws;
            launch_beam_search(bp, st);
        }
    }
    // ... and behind them (k_batcher_last_token writes every slot's input token): the groups' next input tokens and positions
    void enqueue_beam_advance(hipStream_t st)
    {
        for (auto& kv : groups) {
            const BeamGroup& g    = kv.second;
            const int        step = g.n + g.generated;
            hipLaunchKernelGGL(k_batcher_beam_advance, dim3(1), dim3(64), 0, st, d_tok + g.si, d_len + g.si,
                               d_bout + beam_region(g.si) + (size_t)step * g.K, g.K);
        }
    }
    // after the step's synchronisation: every beam takes over its parent's pages, finished groups leave
    void advance_groups(std::vector<Event>& ev, const std::vector<uint8_t>& fin_all)
    {
        std::vector<int> leaders;
        for (auto& kv : groups) {
            leaders.push_back(kv.first);
        }
        for (const int si : leaders) {
            BeamGroup&       g = groups.at(si);
            const int        step = g.n + g.generated;
            std::vector<int> parent(g.K);
            FTCF_HIP_CHECK(hipMemcpy(parent.data(), d_bpar + beam_region(si) + (size_t)step * g.K, (size_t)g.K * 4, hipMemcpyDeviceToHost));
            reparent_group(g, parent);
            for (int k = 0; k < g.K; k++) {
                slots[si + k].len += 1;
            }
            finish_or_append(g, std::vector<uint8_t>(fin_all.begin() + si, fin_all.begin() + si + g.K), ev, true);
        }
    }

    // Which form the next decode step's layers take under tensor parallelism.  FTCF_DECODE_OVERLAP (read when a request begins: an admission)
    // = 1 switches the overlapped form on, the default is off; "auto" (ranks joined by RCCL): decode steps 4..19 of this batcher run plain, 20..35 overlapped, each timed from
    // enqueue to the step's stream synchronisation on the host; after step 35 every rank learns the slowest rank's two sums
    // (comm_max; the ranks' batchers run the same steps) and the batcher stays with the faster form.
    long   ov_steps = 0;
    double ov_us[2] = {0.0, 0.0};
    int    ov_choice = -1;  // -1 undecided, 0 plain, 1 overlapped
    bool   ov_auto = false, ov_last = false;
    bool decode_overlap_now(int B, bool dual)
    {
        ftcf_gptneox* g  = e;
        ov_auto = g->decode_overlap_mode == 2 && g->rccl_ranks();
        const int env = g->decode_overlap_mode == 1 ? 1 : 0;
        ov_last = false;
        if (g->cfg.tensor_para_size == 1 || !dual || !smallm_ws || smallm_partial < 2 * smallm_region || !g->side || B < 4 || B > 32
            || (!env && !ov_auto)) {
            ov_auto = false;
            return false;
        }
        if (ov_auto) {
            ov_last = ov_choice >= 0 ? ov_choice == 1 : (ov_steps >= 20 && ov_steps < 36);
        }
        else {
            ov_last = true;
        }
        return ov_last;
    }
    void decode_overlap_trial(double us, hipStream_t st)
    {
        if (!ov_auto || ov_choice >= 0) {
            return;
        }
        if (ov_steps >= 4 && ov_steps < 36) {
            ov_us[ov_steps >= 20 ? 1 : 0] += us;
        }
        ov_steps++;
        if (ov_steps == 36 && e->tp_scratch) {
            const int a = comm_max(e->cfg.comm, (int)ov_us[0], st, e->tp_scratch), b = comm_max(e->cfg.comm, (int)ov_us[1], st, e->tp_scratch);
            ov_choice = b < a ? 1 : 0;
            e->stats.decode_step_ms_plain      = a * 1e-3f / 16.f;
            e->stats.decode_step_ms_overlapped = b * 1e-3f / 16.f;
            FT_LOG_INFO(e->cfg.device, "batcher: decode all-reduce overlap (auto): plain %.3f ms per step, overlapped %.3f -> %s", a * 1e-3 / 16,
                        b * 1e-3 / 16, ov_choice ? "overlapped from now on" : "plain from now on");
        }
    }

    // ---- one decode step, stage by stage in enqueue order (decode() below) ------------------------------------------------------
    // every slot's hidden state from its token (recomputed each step: the residual never aliases across steps), the burst
    // GEMMs' tag space and step counter
    void enqueue_embedding(hipStream_t st)
    {
        hipLaunchKernelGGL(k_batcher_embed, dim3(max_batch), dim3(256), 0, st, x, e->wte, d_tok, e->H);
        if ((gemm_steps++ & 0x3ffff) == 0 && smallm_ws) {  // the tag space of the burst GEMMs wraps: start it clean
            FTCF_HIP_CHECK(hipMemsetAsync(smallm_ws, 0, smallm_partial + gemm_smallm_ticket_bytes(), st));
        }
        hipLaunchKernelGGL(k_batcher_tick, dim3(1), dim3(1), 0, st, d_gstate);
    }
    // the rows kernel over the paged pool: every slot has its own step (no stop flag, no input lengths), x -> x
    RowsParams rows_params()
    {
        RowsParams rp = e->rows_shape(d_rlayers, x);
        rp.M     = max_batch;
        rp.s_max = max_len;
        rp.tp    = 1;
        rp.plan  = rplan;
        rows_carve(rp, rows_ws);
        rp.d_step      = d_rstep;
        rp.seq_len     = d_len;
        rp.finished    = d_fin;
        rp.rot_table   = d_rot;
        rp.page_table  = d_pt;
        rp.page_tokens = P;
        rp.max_pages   = max_pages;
        return rp;
    }
    // every layer of the step in one launch (rows_device.hip.h, paged K/V)
    void enqueue_rows_layers(hipStream_t st)
    {
        if ((rows_steps++ & 0xfffff) == 0) {  // (the tag space: start it clean now and then)
            FTCF_HIP_CHECK(hipMemsetAsync(rows_ws, 0, rows_flag_bytes(rplan, max_batch, e->nhl), st));
            FTCF_HIP_CHECK(hipMemsetAsync(d_rstep, 0, sizeof(int), st));
        }
        hipLaunchKernelGGL(k_batcher_rows_prep, dim3(max_batch), dim3(64), 0, st, d_rstep, d_rot, d_len, e->cfg.rotary_embedding_dim);
        launch_decode_rows(rows_params(), e->int8, st);
    }
    // the batched parallel-residual layers (layers.hip.h) over the paged K/V pool, with this batcher's buffers and burst workspace
    // overlap (tensor parallel, 4..32 slots): the layer's all-reduce on the side stream under the other micro-batch's launches
    void enqueue_walk_layers(const bool overlap, hipStream_t st)
    {
        const int  B = max_batch, hl = e->hl;
        const bool int8 = e->int8;
        if (overlap) {
            e->decode_overlap_streams();
        }
        ParallelResidualDecoder walk = e->layer_walk();
        walk.fake_mul = 1;  // (fake peers: the all-reduce below scales the sum itself)
        walk.x = x, walk.nrm = nrm, walk.nrm2 = nrm2, walk.qkv = qkv, walk.ctx = ctx, walk.att = att, walk.ffn = ffn, walk.mid = mid;
        walk.ws = smallm_ws, walk.partial = smallm_partial, walk.region = smallm_region;
        walk.d_step = &d_gstate->step;
        walk.seq = &smallm_seq;
        walk.plain = [&](const f16* A, const DenseWeight& dw, const f16* bias, int act, f16* C, int m, int n, int k, hipStream_t s2, int) {
            gemm_dispatch(A, dw.kernel, dw.scale, bias, act, C, m, n, k, int8, s2, nullptr, 0, e->num_cu, nullptr, nullptr,
                          s2 == st ? tiled_ws : nullptr);
        };
        auto attention = [&](int l, const LayerWeights& w, int r0, int M, hipStream_t s2) {
            const size_t    o = (size_t)r0;
            MmhaPagedParams mp{};
            mp.qkv = qkv + o * 3 * hl;
            mp.qkv_bias = w.qkv.bias;
            mp.kpool = kpool + (size_t)l * pool_layer_elems;
            mp.vpool = vpool + (size_t)l * pool_layer_elems;
            mp.page_table = pt_row(r0);
            mp.len = d_len + o;
            mp.finished = d_fin + o;
            mp.B = M;
            mp.nh = e->nhl;
            mp.dh = e->dh;
            mp.rot = e->cfg.rotary_embedding_dim;
            mp.P = P;
            mp.max_pages = max_pages;
            mp.ctx = ctx + o * hl;
            launch_mmha_paged(mp, max_len, s2);
        };
        auto reduce = [&](f16* buf, size_t count, hipStream_t s2, bool) { e->allreduce(buf, count, s2); };
        if (overlap) {
            walk.forward_overlapped(B, attention, reduce);
            return;
        }
        // the attention branch and the FFN branch on two streams, as the engine's batched decode, else up to
        // 16 slots the independent GEMMs paired per launch, else gemm_dispatch
        const DecodeGemms gemms = (smallm_ws && e->decode_branches && e->side) ? DecodeGemms::branches
                                  : (smallm_ws && B <= 16)                     ? DecodeGemms::grouped
                                                                               : DecodeGemms::plain;
        walk.forward(B, gemms, attention, reduce);
    }
    // LM head; tensor parallel: rank r computes rows [r V/TP, (r+1) V/TP) of the replicated lm_head into its slice of
    // `gather`, all-gather + transpose (GptNeoX.cc:888-925, as the engine's own step)
    void enqueue_lm_head(hipStream_t st)
    {
        const int  B = max_batch, H = e->H;
        const bool tp1 = e->cfg.tensor_para_size == 1;
        const int  rows = tp1 ? e->V : e->vl;
        const f16* Wr   = tp1 ? e->lm_head : e->lm_head + (size_t)e->cfg.tensor_para_rank * e->vl * H;
        float*     out  = tp1 ? logits : gather + (size_t)e->cfg.tensor_para_rank * B * e->vl;
        if (B <= 4) {
            launch_lm_head(x, Wr, out, B, rows, H, rows, st, e->final_g, e->final_b, 1e-5f);
        }
        else {
            launch_layernorm(x, e->final_g, e->final_b, nrm, B, H, 1e-5f, true, st);
            lm_head_dispatch(nrm, Wr, out, B, rows, H, rows, st);
        }
        if (!tp1) {
            e->allgather_logits(gather, logits, B, st);
        }
    }
    SamplingParams sampling_params()
    {
        SamplingParams sp{};
        sp.logits = logits;
        sp.B = max_batch;
        sp.V = e->V;
        sp.max_input_len = 0;
        sp.end_id = e->cfg.end_id;
        sp.input_lengths = d_zero;
        sp.top_k = d_topk;
        sp.top_p_topk = d_ptopk;
        sp.top_p_topp = d_ptopp;
        sp.temperature = d_temp;
        sp.random_seed = d_seed;
        sp.draw_counter = d_draws;
        sp.apply_temperature = host_any_temperature ? 1 : 0;
        sp.apply_repetition = host_any_repetition ? 1 : 0;  // (BaseSamplingLayer.cc:283-313: skipped when every row has 1.0)
        sp.repetition_penalty = d_rep;
        sp.return_cum_log_probs = 1;
        // every slot has its own step: its history is column b of the time-major d_hist, positions [0, len[b]]; the sampled
        // token goes to position len[b] + 1 (the penalty of sampling_penalty_kernels.cu:367-425 reads the whole history)
        sp.output_ids = d_hist;
        sp.row_len = d_len;
        sp.total_len = max_len + 2;
        sp.finished = d_fin;
        sp.seq_len = d_len;     // + 1 per sampled token: the slot's length
        sp.cum_log_probs = d_cum;
        sp.output_log_probs = d_olp;  // (row_len: one value per slot, written where cum_log_probs is)
        if (want_top > 0) {  // (row_len: one [B, top_n] row; only the slots that sample are written and read)
            sp.top_logprobs       = want_top;
            sp.top_logprob_ids    = d_top_ids;
            sp.top_logprob_values = d_top_lp;
        }
        sp.pad_count = d_zero;
        sp.state = d_state;     // step stays 0
        sp.ws = samp_ws;
        sp.max_top_k = host_max_top_k;
        sp.any_top_p = host_any_top_p;
        return sp;
    }
    // the sampling kernels on the slots' rows and, with beam groups running, the beam kernels on theirs: the groups' rows are
    // "finished" in the sampling kernels' view (d_sfin), whose new flags of the other rows go back to d_fin afterwards
    void enqueue_sampling(hipStream_t st)
    {
        SamplingParams sp    = sampling_params();
        const bool     beams = !groups.empty();
        if (beams) {
            enqueue_beam_steps(st);
            hipLaunchKernelGGL(k_batcher_sampling_view, dim3(1), dim3(64), 0, st, d_sfin, d_fin, d_isbeam, max_batch, 0);
            sp.finished = d_sfin;
        }
        DynamicDecodeLayer{}.forward(sp, st, false);  // (the stop / length criteria are the scheduler's: no finish step)
        hipLaunchKernelGGL(k_batcher_last_token, dim3(1), dim3(64), 0, st, d_tok, d_hist, d_len, max_batch);
        if (beams) {
            hipLaunchKernelGGL(k_batcher_sampling_view, dim3(1), dim3(64), 0, st, d_sfin, d_fin, d_isbeam, max_batch, 1);
            enqueue_beam_advance(st);
        }
    }
    // the host's copies of one decode step
    struct StepResult {
        int                  top_n = 0;
        std::vector<int>     tok, top_ids;  // [B], [B][top_n]
        std::vector<float>   lp, top_lp;
        std::vector<uint8_t> fin;
        // the sticky give-up words: the exchange-window all-reduce (read while ar_live), the rows kernel, the burst GEMMs
        bool ar_live = false;
        int  ar_err = 0, rows_err = 0, gemm_err = 0;
    };
    // ... filled by copies behind the step's kernels, then the step's ONE synchronisation
    void read_back(StepResult& r, hipStream_t st)
    {
        const size_t B = (size_t)max_batch;
        r.top_n = want_top;
        r.tok.resize(B), r.lp.resize(B), r.fin.resize(B), r.top_ids.resize(B * r.top_n), r.top_lp.resize(B * r.top_n);
        FTCF_HIP_CHECK(hipMemcpyAsync(r.tok.data(), d_tok, B * 4, hipMemcpyDeviceToHost, st));
        FTCF_HIP_CHECK(hipMemcpyAsync(r.lp.data(), d_olp, B * 4, hipMemcpyDeviceToHost, st));
        if (r.top_n > 0) {
            FTCF_HIP_CHECK(hipMemcpyAsync(r.top_ids.data(), d_top_ids, r.top_ids.size() * 4, hipMemcpyDeviceToHost, st));
            FTCF_HIP_CHECK(hipMemcpyAsync(r.top_lp.data(), d_top_lp, r.top_lp.size() * 4, hipMemcpyDeviceToHost, st));
        }
        FTCF_HIP_CHECK(hipMemcpyAsync(r.fin.data(), d_fin, B, hipMemcpyDeviceToHost, st));
        if (smallm_ws) {  // sticky flag of the burst GEMMs' in-launch split-K reduction (the engine's finish() reads its own)
            FTCF_HIP_CHECK(hipMemcpyAsync(&r.gemm_err, reinterpret_cast<char*>(smallm_ws) + smallm_partial, sizeof(int),
                                          hipMemcpyDeviceToHost, st));
        }
        if (use_rows) {
            FTCF_HIP_CHECK(hipMemcpyAsync(&r.rows_err, rows_ws, sizeof(int), hipMemcpyDeviceToHost, st));
        }
        // tensor parallel: the window all-reduce's sticky give-up word of this step's 2 L all-reduces (a peer that never arrived:
        // x is partly reduced and the step's tokens are not to be trusted either), read with the same copies
        r.ar_live = e->cfg.tensor_para_size > 1 && e->cfg.comm && e->cfg.comm->ar_sync && e->cfg.comm->ar_seq > 0 && !e->cfg.comm->ar_failed;
        if (r.ar_live) {
            FTCF_HIP_CHECK(hipMemcpyAsync(&r.ar_err, e->cfg.comm->ar_sync + 2, sizeof(int), hipMemcpyDeviceToHost, st));
        }
        FTCF_HIP_CHECK(hipStreamSynchronize(st));
    }
    // a step one of whose kernels gave up waiting: its tokens are dropped (nothing is reported, the slots keep their host state)
    void check_give_ups(StepResult& r, hipStream_t st)
    {
        if (r.ar_live && e->tp_scratch) {
            // (collective: every rank's batcher runs the same step and has called the window all-reduce as often; all of them learn
            //  of any rank's failure and drop the step)
            r.ar_err = comm_max(e->cfg.comm, r.ar_err, st, e->tp_scratch);
            if (r.ar_err != 0) {
                e->cfg.comm->ar_failed = true;  // this communicator keeps RCCL (or the emulation) from now on
                throw Error(-2, "batcher decode: the exchange-window all-reduce gave up waiting for a peer; the step's tokens are dropped");
            }
        }
        if (r.rows_err != 0) {
            // a hand-off of the rows kernel ran out of its bounded wait (cannot happen with every workgroup resident; bounded all the
            // same): the batcher goes on with the per-GEMM launches
            use_rows = false;
            throw Error(-2, "batcher decode: the rows kernel gave up waiting for a hand-off (code " + std::to_string(r.rows_err) + ")");
        }
        if (r.gemm_err != 0) {
            // (lengths and draw counters advanced on the device: the requests cannot be resumed exactly); the flag is cleared for
            // the caller's next attempt
            FTCF_HIP_CHECK(hipMemsetAsync(smallm_ws, 0, smallm_partial + gemm_smallm_ticket_bytes(), st));
            FTCF_HIP_CHECK(hipStreamSynchronize(st));
            throw Error(-2, "batcher decode: a split-K reducer of the batched GEMM gave up waiting for its sibling workgroups");
        }
    }
    // the step's tokens into the running ordinary slots: events, and the sequences that end leave
    void apply_tokens(const StepResult& r, std::vector<Event>& ev)
    {
        for (int si = 0; si < max_batch; si++) {
            Slot& s = slots[si];
            if (!s.active || s.group >= 0) {
                continue;
            }
            s.len += 1;
            s.generated += 1;
            s.hist.push_back(r.tok[si]);
            const int done = (r.fin[si] || s.generated >= s.max_new || hits_stop_word(s)) ? 1 : 0;
            Event     x{s.id, r.tok[si], done, r.lp[si]};
            cut_top(x, r.top_ids, r.top_lp, si, r.top_n);
            emit(ev, x);
            if (done) {
                FTCF_HIP_CHECK(retire(si, r.fin[si] != 0));
            }
        }
    }

    // one token for every running slot
    void decode(std::vector<Event>& ev)
    {
        Range       rg("ftcf.batcher.decode");
        hipStream_t st = e->stream;
        e->stats.decode_path = use_rows ? 3 : 2;  // (ftcf_gptneox_get_stats of the borrowed engine: which layers the last decode step ran)
        if (overcommit) {
            grow_before_decode(st);  // (may swap requests out; throws "swap space exhausted" before anything of the step is enqueued)
            if (!any_active()) {
                return;  // (the only running request swapped itself out: beam budgets hold the pool)
            }
            refresh_host_flags();
        }
        enqueue_embedding(st);
        if (use_rows) {
            enqueue_rows_layers(st);
        }
        // (FTCF_DECODE_OVERLAP = 0 / 1, auto = timed on this node from here to the step's synchronisation)
        const bool overlap = !use_rows && decode_overlap_now(max_batch, residual_dual_ln_supported(e->H));
        const auto t_dec0  = std::chrono::steady_clock::now();
        if (!use_rows) {
            enqueue_walk_layers(overlap, st);
        }
        enqueue_lm_head(st);
        // the logit processors of the rows that have any: everything behind this point (beam kernels aside: their rows are not
        // processed) reads the processed logits.  No such row: nothing is enqueued.
        enqueue_decode_logit_stage(st);
        enqueue_sampling(st);
        StepResult r;
        read_back(r, st);
        decode_overlap_trial(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_dec0).count(), st);
        e->stats.decode_overlap = overlap ? 1 : 0;
        check_give_ups(r, st);
        apply_tokens(r, ev);
        if (!groups.empty()) {
            advance_groups(ev, r.fin);
        }
    }

    // ONE admission as plan_admission() described it: the prompt phase (with the chunk hook when the plan says so: a decode step
    // of the running slots after every chunk, whose events are final whatever happens to the admission and reach the callback at
    // once), then commit -- or, when anything throws, the rollback by kind (batcher_sched.h: Admission).  The admission's own
    // events reach `ev` and the callback only when it has succeeded: a failed one is retried, and nobody sees a first token twice.
    void run_admission(Admission& a, std::vector<Event>& ev)
    {
        std::vector<Event> own, between;
        const int          n = a.kind == Kind::chunked_one ? 1 : (int)a.requests.size();  // (fork: ONE request)
        try {
            if (a.install_hook) {
                hook_ev          = &between;
                e->prefill_chunk = prefill_chunk;
                // (any_active() where the beam admission once asked "an ordinary slot is active, or a group exists": the same
                //  set, since `slot.group >= 0 && slot.active` <=> the group is in `groups` whenever a hook can run -- groups
                //  enter the map after the admission's forward() and leave it with their slots, drop_group)
                e->prefill_hook = [this] {
                    if (any_active()) {
                        refresh_host_flags();
                        decode(*hook_ev);
                    }
                };
            }
            if (a.kind == Kind::beam) {
                admit_beam(a.slots[0], a.requests[0], own);
            }
            else if (a.kind == Kind::fork) {
                admit_fork(a.slots, a.requests[0], own, a.hit.empty() ? nullptr : &a.hit);
            }
            else {
                admit(a.slots, a.requests, n, own, a.kind == Kind::hit ? &a.hit : nullptr);
            }
        }
        catch (...) {
            // pages to the pool, slots free, the requests back at the head of the queue in their order, the admission's own
            // events dropped (the caller sees the exception, not half an admission)
            e->prefill_hook = nullptr;
            hook_ev         = nullptr;
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
            const long id = a.requests[0].id;
            rollback(
                a, [this](int si) { (void)retire(si); },
                [this, id](int si) {
                    release_group(si);
                    beam_results.erase(id);
                });
            ev.insert(ev.end(), between.begin(), between.end());
            throw;
        }
        e->prefill_hook = nullptr;
        hook_ev         = nullptr;
        if (a.kind == Kind::fork) {
            count_fork(a.requests[0], (int)a.hit.size() * P);
        }
        if (a.kind != Kind::beam) {  // (beam requests neither read nor populate the prefix cache; a fork's prompt blocks enter once)
            commit(a.slots, a.requests, n, (int)a.hit.size() * P);
        }
        ev.insert(ev.end(), between.begin(), between.end());
        ev.insert(ev.end(), own.begin(), own.end());
        fire(own);
    }

    void step(std::vector<Event>& ev)
    {
        FTCF_HIP_CHECK(hipSetDevice(e->cfg.device));
        // the running slots first (a request admitted in this iteration has its first token already)
        const bool any = any_active();
        if (any) {
            decode(ev);
        }
        // then what plan_admission() finds room for: a beam request or a prefix hit alone, else the queue's head requests as one
        // ragged batch -- or, with slots running and a long prompt among them, one after the other
        // overcommit: swapped-out requests resume first, oldest first, each in the lowest free slot (no event: the slot decodes
        // with the next step); while one is left plan_admission() admits nobody
        for (int si; (si = plan_resume()) >= 0;) {
            resume(si, [this](int s2, const Swapped& w, const std::vector<int>& pages) { swap_in_dev(s2, w, pages); });
        }
        Admission a = plan_admission(any);
        if (a.kind != Kind::none) {
            do {
                run_admission(a, ev);
            } while (a.kind == Kind::chunked_one && next_chunked(a));
        }
        refresh_host_flags();
    }
};

extern "C" int ftcf_batcher_create(ftcf_gptneox_t engine, int max_batch, int page_tokens, int num_pages, int max_seq_len,
                                   ftcf_batcher_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(engine && out, "NULL argument");
        require_device();
        auto b = std::make_unique<ftcf_batcher>();
        b->init(engine, max_batch, page_tokens, num_pages, max_seq_len);
        *out = b.release();
    });
}
extern "C" int ftcf_batcher_create_ex(ftcf_gptneox_t engine, int max_batch, int page_tokens, int num_pages, int max_seq_len,
                                      int prefix_cache, ftcf_batcher_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(engine && out, "NULL argument");
        require_device();
        auto b = std::make_unique<ftcf_batcher>();
        b->init(engine, max_batch, page_tokens, num_pages, max_seq_len, prefix_cache != 0);
        *out = b.release();
    });
}
extern "C" int ftcf_batcher_create_opts(ftcf_gptneox_t engine, const ftcf_batcher_options* options, ftcf_batcher_t* out)
{
    return guarded([&] {
        FTCF_CHECK_ARG(engine && options && out, "NULL argument");
        FTCF_CHECK_ARG(options->struct_size == (int)sizeof(ftcf_batcher_options), "struct_size is not sizeof(ftcf_batcher_options)");
        require_device();
        auto b = std::make_unique<ftcf_batcher>();
        b->init(engine, options->max_batch, options->page_tokens, options->num_pages, options->max_seq_len, options->prefix_cache != 0,
                options->overcommit != 0, options->swap_pages, options->swap_stage_bytes);
        *out = b.release();
    });
}
extern "C" int ftcf_batcher_preempt_stats(ftcf_batcher_t b, int* enabled, int* swapped_requests, int* swap_pages_used,
                                          int* swap_pages_total, long* preemptions, long* resumes, long* pages_out, long* pages_in)
{
    return guarded([&] {
        require_device();  // (no batcher exists without one)
        FTCF_CHECK_ARG(b, "NULL argument");
        if (enabled) {
            *enabled = b->overcommit ? 1 : 0;
        }
        if (swapped_requests) {
            *swapped_requests = (int)b->swapped.size();
        }
        if (swap_pages_used) {
            *swap_pages_used = b->swap_total - (int)b->host_free.size();
        }
        if (swap_pages_total) {
            *swap_pages_total = b->swap_total;
        }
        if (preemptions) {
            *preemptions = b->pe_preemptions;
        }
        if (resumes) {
            *resumes = b->pe_resumes;
        }
        if (pages_out) {
            *pages_out = b->pe_pages_out;
        }
        if (pages_in) {
            *pages_in = b->pe_pages_in;
        }
    });
}
extern "C" int ftcf_batcher_prefix_stats(ftcf_batcher_t b, int* enabled, int* cached_pages, int* evictable_pages, long* lookups,
                                         long* prompt_tokens, long* hit_tokens, long* computed_tokens, long* evictions)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        if (enabled) {
            *enabled = b->prefix_on ? 1 : 0;
        }
        if (cached_pages) {
            *cached_pages = b->pindex.n_cached;
        }
        if (evictable_pages) {
            *evictable_pages = b->pindex.evictable(b->page_ref);
        }
        if (lookups) {
            *lookups = b->px_lookups;
        }
        if (prompt_tokens) {
            *prompt_tokens = b->px_prompt_tokens;
        }
        if (hit_tokens) {
            *hit_tokens = b->px_hit_tokens;
        }
        if (computed_tokens) {
            *computed_tokens = b->px_computed_tokens;
        }
        if (evictions) {
            *evictions = b->px_evictions;
        }
    });
}
extern "C" int ftcf_batcher_clear_prefix_cache(ftcf_batcher_t b)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        b->clear_prefix_cache();
    });
}
extern "C" int ftcf_batcher_submit(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k,
                                   float top_p, float temperature, unsigned long long seed, long* request_id)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_id, "NULL argument");
        *request_id = b->submit(prompt_ids, prompt_len, max_new_tokens, top_k, top_p, temperature, (uint64_t)seed);
    });
}
extern "C" int ftcf_batcher_submit_ex(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k,
                                      float top_p, float temperature, float repetition_penalty, unsigned long long seed,
                                      const int* stop_words, int stop_len, long* request_id)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_id, "NULL argument");
        *request_id = b->submit(prompt_ids, prompt_len, max_new_tokens, top_k, top_p, temperature, (uint64_t)seed,
                                repetition_penalty, stop_words, stop_len);
    });
}
// a request's logit processors out of the C struct (NULL: none), checked
static ftcf_batcher::LogitOptions logit_options_of(ftcf_batcher_t b, const ftcf_logit_options* opts)
{
    ftcf_batcher::LogitOptions o;
    // (a zeroed struct, struct_size included, asks for nothing)
    const bool zeroed = opts && opts->struct_size == 0 && opts->presence_penalty == 0.f && opts->frequency_penalty == 0.f
                        && opts->min_new_tokens == 0 && !opts->bias_ids && !opts->bias_values && opts->n_bias == 0
                        && !opts->bad_words && opts->bad_words_len == 0;
    if (opts && !zeroed) {
        FTCF_CHECK_ARG(opts->struct_size == (int)sizeof(ftcf_logit_options), "struct_size is not sizeof(ftcf_logit_options)");
        o = b->make_logit_options(opts->presence_penalty, opts->frequency_penalty, opts->min_new_tokens, opts->bias_ids,
                                  opts->bias_values, opts->n_bias, opts->bad_words, opts->bad_words_len);
    }
    return o;
}
extern "C" int ftcf_batcher_submit_opts(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k,
                                        float top_p, float temperature, float repetition_penalty, unsigned long long seed,
                                        const int* stop_words, int stop_len, const ftcf_logit_options* opts, long* request_id)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_id, "NULL argument");
        *request_id = b->submit_opts(prompt_ids, prompt_len, max_new_tokens, top_k, top_p, temperature, (uint64_t)seed,
                                     repetition_penalty, stop_words, stop_len, logit_options_of(b, opts));
    });
}
extern "C" int ftcf_batcher_submit_n(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int top_k, float top_p,
                                     float temperature, float repetition_penalty, unsigned long long seed, const int* stop_words,
                                     int stop_len, const ftcf_logit_options* opts, int n_samples, long* request_ids)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_ids, "NULL argument");
        b->submit_n(prompt_ids, prompt_len, max_new_tokens, top_k, top_p, temperature, (uint64_t)seed, repetition_penalty, stop_words,
                    stop_len, logit_options_of(b, opts), n_samples, request_ids);
    });
}
extern "C" int ftcf_batcher_fork_stats(ftcf_batcher_t b, long* requests, long* siblings, long* shared_pages, long* prompt_tokens_computed)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        if (requests) {
            *requests = b->fk_requests;
        }
        if (siblings) {
            *siblings = b->fk_siblings;
        }
        if (shared_pages) {
            *shared_pages = b->fk_shared_pages;
        }
        if (prompt_tokens_computed) {
            *prompt_tokens_computed = b->fk_prompt_tokens;
        }
    });
}
extern "C" int ftcf_batcher_set_token_mask(ftcf_batcher_t b, long request_id, const unsigned* allowed_bits, int n_words)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        b->set_token_mask(request_id, allowed_bits, n_words);
    });
}
extern "C" int ftcf_batcher_submit_beam(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int beam_width,
                                        float beam_search_diversity_rate, float len_penalty, float temperature,
                                        float repetition_penalty, long* request_id)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_id, "NULL argument");
        *request_id = b->submit_beam(prompt_ids, prompt_len, max_new_tokens, beam_width, beam_search_diversity_rate, len_penalty,
                                     temperature, repetition_penalty);
    });
}
extern "C" int ftcf_batcher_submit_beam_ex(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens, int beam_width,
                                           float beam_search_diversity_rate, float len_penalty, float temperature,
                                           float repetition_penalty, int min_length, const int* stop_words, int stop_len,
                                           long* request_id)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_id, "NULL argument");
        *request_id = b->submit_beam(prompt_ids, prompt_len, max_new_tokens, beam_width, beam_search_diversity_rate, len_penalty,
                                     temperature, repetition_penalty, min_length, stop_words, stop_len);
    });
}
// the parked result of a beam request, fetched once; token_log_probs: ftcf_batcher_beam_result_ex's array or NULL
static void fetch_beam_result(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths, float* cum_log_probs,
                              float* token_log_probs, int capacity, int* beam_width, int* total_len)
{
    FTCF_CHECK_ARG(b && beam_width && total_len, "NULL argument");
    auto it = b->beam_results.find(request_id);
    if (it == b->beam_results.end()) {
        *beam_width = 0;
        *total_len  = 0;
        return;
    }
    const ftcf_batcher::BeamResult& r = it->second;
    *beam_width = r.K;
    *total_len  = r.total;
    if (!output_ids) {
        return;  // (a size query)
    }
    FTCF_CHECK_ARG(capacity >= r.K * r.total && sequence_lengths && cum_log_probs, "beam result: arrays too small");
    FTCF_CHECK_ARG(!token_log_probs || r.has_lp, "beam result: the request was not submitted with token_log_probs");
    std::copy(r.ids.begin(), r.ids.end(), output_ids);
    std::copy(r.lens.begin(), r.lens.end(), sequence_lengths);
    std::copy(r.cum.begin(), r.cum.end(), cum_log_probs);
    if (token_log_probs) {
        std::copy(r.lp.begin(), r.lp.end(), token_log_probs);
    }
    b->beam_results.erase(it);
}
extern "C" int ftcf_batcher_beam_result(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths,
                                        float* cum_log_probs, int capacity, int* beam_width, int* total_len)
{
    return guarded([&] {
        fetch_beam_result(b, request_id, output_ids, sequence_lengths, cum_log_probs, nullptr, capacity, beam_width, total_len);
    });
}
extern "C" int ftcf_batcher_submit_beam_opts(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens,
                                             const ftcf_beam_options* o, long* request_id)
{
    return guarded([&] {
        require_device();  // (no batcher exists without one)
        FTCF_CHECK_ARG(b && o && request_id, "NULL argument");
        FTCF_CHECK_ARG(o->struct_size == (int)sizeof(ftcf_beam_options), "struct_size is not sizeof(ftcf_beam_options)");
        *request_id = b->submit_beam(prompt_ids, prompt_len, max_new_tokens, o->beam_width, o->beam_search_diversity_rate, o->len_penalty,
                                     o->temperature, o->repetition_penalty, o->min_length, o->stop_words, o->stop_len,
                                     o->token_log_probs != 0);
    });
}
extern "C" int ftcf_batcher_beam_result_ex(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths,
                                           float* cum_log_probs, float* token_log_probs, int capacity, int* beam_width, int* total_len)
{
    return guarded([&] {
        require_device();  // (no batcher exists without one)
        fetch_beam_result(b, request_id, output_ids, sequence_lengths, cum_log_probs, token_log_probs, capacity, beam_width, total_len);
    });
}
static int batcher_step(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int capacity, int* n_events,
                        int top_n = 0, int* top_ids = nullptr, float* top_log_probs = nullptr)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b && request_ids && tokens && finished && n_events, "NULL argument");
        FTCF_CHECK_ARG(top_n >= 0 && top_n <= TOP_LOGPROBS_MAX, "top_n must be in [1, 20]");
        FTCF_CHECK_ARG(top_n == 0 || (top_ids && top_log_probs), "NULL argument");
        FTCF_CHECK_ARG(capacity >= 2 * b->max_batch, "event arrays must hold 2 * max_batch entries");
        if (b->outbox.empty()) {  // (else: the rest of the previous iteration's events first)
            std::vector<ftcf_batcher::Event> ev;
            b->want_log_probs = log_probs != nullptr;
            b->want_top       = top_n;
            try {
                b->step(ev);
            }
            catch (...) {
                b->want_log_probs = false;
                b->want_top       = 0;
                b->outbox.insert(b->outbox.end(), ev.begin(), ev.end());  // tokens of decode steps that did run are not lost
                throw;
            }
            b->want_log_probs = false;
            b->want_top       = 0;
            b->outbox.insert(b->outbox.end(), ev.begin(), ev.end());
        }
        int n = 0;
        for (; n < capacity && !b->outbox.empty(); n++) {
            request_ids[n] = b->outbox.front().id;
            tokens[n]      = b->outbox.front().token;
            finished[n]    = b->outbox.front().finished;
            if (log_probs) {
                log_probs[n] = b->outbox.front().log_prob;
            }
            if (top_n > 0) {  // (pairs taken with another top_n, or not at all: none)
                const ftcf_batcher::Event& x  = b->outbox.front();
                const bool                 ok = (int)x.top_ids.size() == top_n;
                for (int j = 0; j < top_n; j++) {
                    top_ids[(size_t)n * top_n + j]       = ok ? x.top_ids[j] : -1;
                    top_log_probs[(size_t)n * top_n + j] = ok ? x.top_lp[j] : NAN;
                }
            }
            b->outbox.pop_front();
        }
        *n_events = n;
    });
}
extern "C" int ftcf_batcher_step(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, int capacity, int* n_events)
{
    return batcher_step(b, request_ids, tokens, finished, nullptr, capacity, n_events);
}
extern "C" int ftcf_batcher_step_ex(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int capacity,
                                    int* n_events)
{
    if (!log_probs) {
        return guarded([&] { FTCF_CHECK_ARG(false, "NULL argument"); });
    }
    return batcher_step(b, request_ids, tokens, finished, log_probs, capacity, n_events);
}
extern "C" int ftcf_batcher_step_top(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int top_n,
                                     int* top_ids, float* top_log_probs, int capacity, int* n_events)
{
    if (top_n < 1 || !top_ids || !top_log_probs) {
        return guarded([&] { FTCF_CHECK_ARG(false, "top_n must be in [1, 20] with both arrays"); });
    }
    return batcher_step(b, request_ids, tokens, finished, log_probs, capacity, n_events, top_n, top_ids, top_log_probs);
}
extern "C" int ftcf_batcher_set_token_callback(ftcf_batcher_t b, ftcf_token_callback_fn fn, void* user)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        b->on_token      = fn;
        b->on_token_user = user;
    });
}
extern "C" int ftcf_batcher_status(ftcf_batcher_t b, int* waiting, int* running, int* free_pages)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        int run = 0;
        for (const auto& s : b->slots) {
            run += s.active ? 1 : 0;
        }
        if (waiting) {
            *waiting = (int)(b->waiting.size() + b->swapped.size());  // (a swapped-out request waits for a slot and pages)
        }
        if (running) {
            *running = run + (b->outbox.empty() ? 0 : 1);  // (events still to be fetched keep the batcher "busy")
        }
        if (free_pages) {
            *free_pages = (int)b->free_pages.size();
        }
    });
}
extern "C" int ftcf_batcher_cancel(ftcf_batcher_t b, long request_id, int* found)
{
    return guarded([&] {
        FTCF_CHECK_ARG(b, "NULL argument");
        int hit = 0;
        if (b->cancel_waiting(request_id)) {  // (a waiting fork request: the sibling alone)
            hit = 1;
        }
        if (!hit && b->drop_swapped(request_id)) {  // a swapped-out request: its host pages return
            hit = 1;
        }
        for (int si = 0; si < b->max_batch && !hit; si++) {
            ftcf_batcher::Slot& s = b->slots[si];
            if (s.active && s.id == request_id && s.group >= 0) {
                FTCF_HIP_CHECK(hipSetDevice(b->e->cfg.device));
                b->release_group(s.group);
                hit = 1;
                break;
            }
            if (s.active && s.id == request_id) {
                FTCF_HIP_CHECK(hipSetDevice(b->e->cfg.device));
                FTCF_HIP_CHECK(b->retire(si));
                hit = 1;
            }
        }
        if (!hit && b->beam_results.erase(request_id) > 0) {  // a finished beam request whose result was never fetched
            hit = 1;
        }
        if (found) {
            *found = hit;
        }
    });
}
extern "C" int ftcf_batcher_destroy(ftcf_batcher_t b)
{
    return guarded([&] { delete b; });
}
