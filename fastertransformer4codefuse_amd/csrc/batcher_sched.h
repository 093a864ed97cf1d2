// What the continuous batcher (batcher.hip) decides on the host: the request queue, the slots' host
// fields, page accounting and the admission policy.  Plain C++ (no HIP): tools/check_batcher_sched.cc drives it with a fake
// prompt phase that fails at seeded points and checks the page accounting, the queue order and the rollbacks.
// tools/check_batcher_preempt.cc does the same for the overcommit policy (pages on demand, preemption by swap, resume),
// tools/check_batcher_fork.cc for fork requests (submit_n: n samples of one prompt, the prompt's full pages shared).
//
// ftcf_batcher derives from BatcherSched and adds the device side: buffers, launches and the mirrors of this state on the
// device (d_fin, d_isbeam, page tables).  Where an operation has a device half the name here is the host half's.
//
// A FAILED ADMISSION is rolled back to: none of its slots active, no group of its id, every page it took back in the pool, its
// requests back at the queue's head in the order they had.  NOT restored: cached pages that take_page() evicted from the
// prefix index on the way (they stay evicted; px_evictions counts them) and the ORDER of the free list.
#pragma once

#include "ftcf_error.h"
#include "prefix_index.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace ftcf {

struct BatcherSched {
    typedef std::vector<std::vector<int>> StopWords;  // stop sequences (token ids)
    static constexpr int BIAS_MAX = 1024;  // logit-bias pairs per request (the logit stage's LOGIT_BIAS_MAX)
    static constexpr int BAD_LW   = 256;   // total bad-word tokens per request (its LOGIT_BAD_WORDS_MAX)
    // a request's logit processors (ftcf_batcher_submit_opts), checked; all defaults: none
    struct LogitOptions {
        float              presence = 0.f, frequency = 0.f;
        int                min_new = 0;
        std::vector<int>   bias_ids;
        std::vector<float> bias_values;
        std::vector<int>   bad;  // the [2][BAD_LW] word list of the device, or empty
        bool any() const
        {
            return presence != 0.f || frequency != 0.f || min_new > 0 || !bias_ids.empty() || !bad.empty();
        }
    };
    struct Request {
        long             id;
        std::vector<int> prompt;
        int              max_new, top_k;
        float            top_p, temperature, repetition_penalty = 1.f;
        uint64_t         seed;
        StopWords        stop;
        int              beam_width = 1;     // > 1: a beam group (submit_beam)
        float            diversity = 0.f, len_penalty = 0.f;
        int              min_length = 0;     // beam requests: the end token is held back for this many new tokens
        bool             token_log_probs = false;  // beam requests: the result carries every hypothesis' per-token log-probabilities
        LogitOptions          lopt;  // ordinary requests: logit processors
        std::vector<unsigned> mask;  // ... and the allowed-token mask set while it waits (empty: none)
        // a fork request (submit_n): ONE prompt phase, n_samples siblings.  Sibling `index` is the plain request of seed + index
        // with its own id and mask; `sibs` lists the ones still wanted (a cancelled sibling leaves it); `id` is the first one's.
        struct Sibling {
            long                  id;
            int                   index;
            std::vector<unsigned> mask;
        };
        int                  n_samples = 1;  // == sibs.size() for a fork request
        std::vector<Sibling> sibs;           // (empty: not a fork request)
        bool is_fork() const
        {
            return !sibs.empty();
        }
    };
    struct Slot {
        bool             active = false;
        long             id = 0;
        int              len = 0, generated = 0, max_new = 0;
        std::vector<int> pages;
        // the request's own token history (prompt + generated) and stop sequences: the stop criterion
        // (stop_criteria_kernels.cu:24-83: finished AFTER the sequence has been emitted) is the scheduler's, on the host,
        // which sees every token anyway
        std::vector<int> hist;
        StopWords        stop;
        float            repetition_penalty = 1.f;
        int              group = -1;  // a beam of the group whose first slot this is (-1: an ordinary sequence)
        // the request's logit processors and allowed-token mask; *_dirty: the device's copy of the slot's row is not this one yet
        LogitOptions          lopt;
        std::vector<unsigned> mask;
        bool                  lopt_dirty = false, mask_dirty = false;
        // the request's sampling parameters (the device holds them per slot; a swapped-out request takes them to its next slot)
        int      top_k = 0;
        float    top_p = 0.f, temperature = 1.f;
        uint64_t seed = 0;
        bool processed() const
        {
            return lopt.any() || !mask.empty();
        }
    };
    // A preempted request (overcommit): its slot's fields without the pages, the host pages that hold its K/V (in the order of
    // its page list), the host's view of its top-k and temperature, and what only the device knew: draw counter, cumulative
    // log-probability.
    struct Swapped {
        Slot             s;
        std::vector<int> host;
        int              slot_topk = 1;
        float            slot_temp = 1.f;
        uint64_t         draws = 0;
        float            cum = 0.f;
    };
    // Beam search inside the batcher (round 4; the reference's serving layer runs beam requests through the same decoder:
    // triton_backend/gptneox/GptNeoXTritonModelInstance.cc).  A request of beam width K lives in K CONSECUTIVE slots -- its
    // beams ride in the same batched GEMMs as everybody else's rows -- and is scored by the engine's own beam kernels
    // (launch_beam_search with batch 1: OnlineBeamSearchLayer semantics, kernels_beam.hip) on per-group state.  The cache
    // indirection of the reference (BaseBeamSearchLayer.cu:30-62: which beam's cache row holds position t) is replaced by what a
    // paged cache is for: after every step beam k's page list becomes a copy of its parent's (pages are reference counted),
    // and only the page the next token will be appended to is copied when it is shared (copy-on-write, all layers, one launch
    // per step); the attention kernel is the ordinary paged one.  The prompt's pages are written once and shared by all beams.
    struct BeamGroup {
        long id = 0;
        int  si = 0, K = 0, n = 0, max_new = 0, generated = 0, budget = 0;
        bool penalised = false;  // repetition_penalty != 1
        bool has_stop = false, has_min = false;
        bool token_log_probs = false;  // the request asked for its hypotheses' per-token log-probabilities
        std::vector<std::vector<int>> lists;  // page list of every beam
    };
    // The next admission, as plan_admission() describes it and ftcf_batcher::run_admission() carries it out.
    //   kind         requests                      hook installed when                                  rolled back          commit
    //   beam         1, in K consecutive slots     slots run NOW and the prompt is long                 group, parked result no
    //   hit          1 (its cached pages in `hit`) slots ran BEFORE the decode step, the tail is long   its slot             yes
    //   chunked_one  the FIRST of `requests`       slots run NOW                                        all of `slots`       yes
    //   ragged       all, one batch                never                                                all of `slots`       yes
    //   fork         1, in n_samples free slots    slots ran BEFORE the decode step, the tail is long   all of `slots`       yes
    // ("long": more than prefill_chunk tokens; chunked_one is chosen when slots ran before the decode step and one of the
    // requests is long.)  The requests have left the queue; rollback() puts them back.
    enum class Kind { none, beam, hit, chunked_one, ragged, fork };
    struct Admission {
        Kind                 kind = Kind::none;
        std::vector<int>     slots;  // beam: its K slots
        std::vector<Request> requests;
        std::vector<int>     hit;    // hit, fork: the cached pages of the prompt's first blocks
        bool                 install_hook = false;
    };

    static constexpr int STOP_LW = 64;  // total stop-word tokens per request (the [2][Lw] word list of the admission)
    static constexpr int MAX_BEAM_WIDTH = 64;  // (the beam kernels' BEAM_MAX_K)

    int max_batch = 0, P = 0, num_pages = 0, max_pages = 0, max_len = 0, max_prompt = 0, vocab = 0;
    // chunked admission: with slots running, a prompt longer than this is prefilled alone, `prefill_chunk` tokens at a time, one
    // decode step of the running slots between two chunks (FTCF_BATCHER_PREFILL_CHUNK; 0 = whole prompts)
    int prefill_chunk = 512;

    std::vector<Slot>        slots;
    std::deque<Request>      waiting;
    std::vector<int>         free_pages;
    std::vector<int>         page_ref;  // references to a page (ordinary sequences: 1)
    std::map<int, BeamGroup> groups;    // by first slot
    // prefix cache: the index holds one reference to each of its pages; `deferred` = slots of an admission whose
    // request finished with its first token, released only after the admission's prompts have been inserted
    bool             prefix_on = false;
    PrefixIndex      pindex;
    std::vector<int> deferred;
    long             px_lookups = 0, px_prompt_tokens = 0, px_hit_tokens = 0, px_computed_tokens = 0, px_evictions = 0;
    long             next_id = 1;
    // fork requests (submit_n) since creation: admissions, the siblings they opened, the page allocations sharing saved ((n - 1)
    // per shared page) and the prompt tokens their prompt phases computed
    long             fk_requests = 0, fk_siblings = 0, fk_shared_pages = 0, fk_prompt_tokens = 0;
    // host view of the running slots' sampling parameters (refresh_host_flags)
    int                host_max_top_k = 1, host_any_top_p = 0;
    bool               host_any_temperature = false, host_any_repetition = false;
    std::vector<int>   slot_topk;
    std::vector<float> slot_temp;
    // Overcommit (ftcf_batcher_create_opts; off: none of this is touched).  An ordinary request takes the pages
    // its prompt needs and one more each time its sequence crosses a page boundary (grow_slots); when the pool cannot give
    // one, the latest arrival among the running ordinary slots is swapped out to host pages and resumes -- before anybody is
    // admitted -- when a slot and pages are free again.  `swapped` is in request-id order; host_free: the host pages nobody holds;
    // inflight_reserve: pages a beam admission in flight was promised and has not taken yet (its group opens after the prompt
    // phase, and the decode steps between its chunks must leave them alone).
    bool                overcommit = false;
    int                 swap_total = 0, inflight_reserve = 0;
    std::vector<int>    host_free;
    std::deque<Swapped> swapped;
    long                pe_preemptions = 0, pe_resumes = 0, pe_pages_out = 0, pe_pages_in = 0;

    void init_overcommit(int swap_pages)
    {
        overcommit = true;
        swap_total = swap_pages > 0 ? swap_pages : num_pages;
        host_free.resize(swap_total);
        for (int i = 0; i < swap_total; i++) {
            host_free[i] = swap_total - 1 - i;  // (taken from the back: ascending, so that a victim's host pages are mostly one run)
        }
    }

    void init_sched(int mb, int page_tokens, int pages, int max_seq_len, int vocab_size, bool prefix_cache)
    {
        max_batch  = mb;
        P          = page_tokens;
        num_pages  = pages;
        max_pages  = (max_seq_len + P - 1) / P;
        max_len    = max_pages * P;
        max_prompt = max_seq_len - 1;
        vocab      = vocab_size;
        prefix_on  = prefix_cache;
        slots.assign(max_batch, Slot{});
        slot_topk.assign(max_batch, 1);
        slot_temp.assign(max_batch, 1.f);
        free_pages.resize(num_pages);
        for (int i = 0; i < num_pages; i++) {
            free_pages[i] = num_pages - 1 - i;
        }
        page_ref.assign(num_pages, 0);
        pindex = PrefixIndex(P);
    }

    int pages_needed(int n, int max_new) const
    {
        return (n + max_new + P - 1) / P;
    }
    static int keff(int top_k, float top_p)  // BaseSamplingLayer: (0, 0) = greedy
    {
        return (top_k == 0 && top_p == 0.f) ? 1 : std::min(top_k, 1024);
    }
    bool any_active() const
    {
        return std::any_of(slots.begin(), slots.end(), [](const Slot& s) { return s.active; });
    }

    // ---- pages -------------------------------------------------------------------------------------------------------
    int take_page()
    {
        if (free_pages.empty() && prefix_on) {  // a cached page only the index holds makes room (LRU, leaves first)
            const int pg = pindex.evict_one(page_ref);
            if (pg >= 0) {
                px_evictions++;
                drop_page(pg);
            }
        }
        if (free_pages.empty()) {
            throw Error(-2, "batcher: the page pool is exhausted (a reservation was wrong)");
        }
        const int pg = free_pages.back();
        free_pages.pop_back();
        page_ref[pg] = 1;
        return pg;
    }
    void drop_page(const int pg)
    {
        if (--page_ref[pg] == 0) {
            free_pages.push_back(pg);
        }
    }
    // pages promised to running beam groups but not yet taken (a group takes its pages as its beams diverge: at most
    // budget = K * pages of one full-length sequence)
    int reserved_pages() const
    {
        int r = 0;
        for (const auto& kv : groups) {
            std::set<int> held;
            for (const auto& l : kv.second.lists) {
                held.insert(l.begin(), l.end());
            }
            r += std::max(0, kv.second.budget - (int)held.size());
        }
        return r;
    }
    // what an admission may take: the free pages nobody was promised and (prefix cache) the cached pages nobody else holds --
    // take_page evicts them when the free list runs dry
    int pages_available() const
    {
        return (int)free_pages.size() - reserved_pages() + (prefix_on ? pindex.evictable(page_ref) : 0);
    }
    void release(Slot& s)
    {
        for (int pg : s.pages) {
            drop_page(pg);
        }
        s.pages.clear();
        s.active = false;
    }
    // the group's pages and slots; returns its width (0: there is no such group)
    int drop_group(const int si)
    {
        auto it = groups.find(si);
        if (it == groups.end()) {
            return 0;
        }
        const BeamGroup& g = it->second;
        const int        K = g.K;
        for (int k = 0; k < K; k++) {
            for (int pg : g.lists[k]) {
                drop_page(pg);
            }
            slots[si + k].active = false;
            slots[si + k].group  = -1;
        }
        groups.erase(it);
        return K;
    }
    void clear_prefix_cache()
    {
        for (int pg; (pg = pindex.evict_one(page_ref)) >= 0;) {
            drop_page(pg);
        }
    }

    // ---- overcommit: pages on demand, preemption by swap -------------------------------------------------------------------
    // the pages an ordinary request takes at admission: all it can ever need, or (overcommit) its prompt's and the first token's
    int admission_pages(const Request& r) const
    {
        return overcommit ? ((int)r.prompt.size() + 1 + P - 1) / P : pages_needed((int)r.prompt.size(), r.max_new);
    }
    int running_ordinary() const
    {
        int n = 0;
        for (const Slot& s : slots) {
            n += (s.active && s.group < 0) ? 1 : 0;
        }
        return n;
    }
    // what an ordinary sequence may take now: not what running groups or a beam admission in flight were promised
    int pages_grantable() const
    {
        return pages_available() - inflight_reserve;
    }
    // the victim of a preemption: the running ordinary slot of the largest request id (the latest arrival) whose pages the swap
    // space can take; -1: none.  Beams and the slots of an admission in flight (not active yet) are never victims.
    int pick_victim() const
    {
        int v = -1;
        for (int si = 0; si < max_batch; si++) {
            const Slot& s = slots[si];
            if (s.active && s.group < 0 && s.pages.size() <= host_free.size() && (v < 0 || s.id > slots[v].id)) {
                v = si;
            }
        }
        return v;
    }
    // the slot's request leaves for the swap space.  swap_out(si, pages, host_pages, draws, cum) is the device half: copies the
    // pages out, reads the draw counter and the cumulative log-probability back, tells the device the slot is finished.
    template<typename SwapOut>
    void preempt(const int si, SwapOut& swap_out)
    {
        Slot&   s = slots[si];
        Swapped w;
        w.host.assign(host_free.end() - s.pages.size(), host_free.end());
        std::reverse(w.host.begin(), w.host.end());
        swap_out(si, s.pages, w.host, w.draws, w.cum);  // (throws: nothing has changed)
        host_free.resize(host_free.size() - s.pages.size());
        pe_preemptions++;
        pe_pages_out += (long)s.pages.size();
        release(s);
        w.slot_topk = slot_topk[si];
        w.slot_temp = slot_temp[si];
        w.s         = s;
        auto at = std::find_if(swapped.begin(), swapped.end(), [&](const Swapped& x) { return x.s.id > w.s.id; });
        swapped.insert(at, std::move(w));
    }
    // Before a decode step enqueues anything: every running ordinary slot whose next token starts a page takes that page, in slot
    // order; when the pool has none (cached pages nobody holds are evicted first, take_page) victims are swapped out until it
    // has -- the slot itself when it is the latest arrival.  on_grow(si) is the device half of ONE growth -- the slot's page
    // table row gets its new last entry -- and runs the moment the slot has grown: when a later slot throws, the device already
    // knows every page the host has handed out (an on_grow that throws gives its page back first).  Returns how many slots grew.
    // Throws -2 when no victim fits the swap space: whatever grew or left before stays so, on both sides; nothing is half done.
    template<typename SwapOut, typename OnGrow>
    int grow_slots(SwapOut swap_out, OnGrow on_grow)
    {
        int grown = 0;
        if (!overcommit) {
            return grown;
        }
        for (int si = 0; si < max_batch; si++) {
            Slot& s = slots[si];
            if (!s.active || s.group >= 0 || s.len < (int)s.pages.size() * P) {
                continue;
            }
            while (s.active && pages_grantable() < 1) {
                const int v = pick_victim();
                if (v < 0) {
                    throw Error(-2, "batcher: swap space exhausted (no running request fits the free host pages; cancel a request or "
                                    "create the batcher with more swap_pages)");
                }
                preempt(v, swap_out);
            }
            if (s.active) {
                s.pages.push_back(take_page());
                try {
                    on_grow(si);
                }
                catch (...) {
                    drop_page(s.pages.back());
                    s.pages.pop_back();
                    throw;
                }
                grown++;
            }
        }
        return grown;
    }
    // the slot the head of `swapped` may resume in now (the lowest free one), or -1: no request is swapped out, no slot is free
    // or the pool lacks its pages plus the watermark of one page per running ordinary slot (waived when none runs)
    int plan_resume() const
    {
        if (swapped.empty()) {
            return -1;
        }
        int si = 0;
        while (si < max_batch && slots[si].active) {
            si++;
        }
        const int need = (swapped.front().s.len + 1 + P - 1) / P;
        return (si < max_batch && pages_grantable() >= need + running_ordinary()) ? si : -1;
    }
    // ... and does: fresh private pages, the slot's fields as they were.  swap_in(si, swapped_request, pages) is the device half:
    // the host pages into the first pages of the new list, the slot's device state.  No event: nothing was generated.
    template<typename SwapIn>
    void resume(const int si, SwapIn swap_in)
    {
        Swapped& w = swapped.front();
        Slot&    s = slots[si];
        s          = w.s;
        for (int k = 0, need = (s.len + 1 + P - 1) / P; k < need; k++) {
            s.pages.push_back(take_page());
        }
        s.active     = true;
        s.lopt_dirty = s.mask_dirty = true;
        slot_topk[si] = w.slot_topk;
        slot_temp[si] = w.slot_temp;
        try {
            swap_in(si, w, s.pages);
        }
        catch (...) {
            release(s);
            throw;
        }
        host_free.insert(host_free.end(), w.host.rbegin(), w.host.rend());
        pe_resumes++;
        pe_pages_in += (long)w.host.size();
        swapped.pop_front();
    }
    // a swapped-out request is dropped (cancel): its host pages return; false: no such request
    bool drop_swapped(const long id)
    {
        for (auto it = swapped.begin(); it != swapped.end(); ++it) {
            if (it->s.id == id) {
                host_free.insert(host_free.end(), it->host.rbegin(), it->host.rend());
                swapped.erase(it);
                return true;
            }
        }
        return false;
    }

    // ---- stop words --------------------------------------------------------------------------------------------------
    // to_word_list_format (codefuse_example.py:26-53): [0][..] flat ids, [1][..] cumulative end offsets, -1 padded
    static StopWords parse_word_list(const int* stop_words, int stop_len)
    {
        StopWords stop;
        for (int i = 0, start = 0; i < stop_len; i++) {
            const int end = stop_words[stop_len + i];
            if (end < 0) {
                break;
            }
            FTCF_CHECK_ARG(end > start && end <= stop_len, "bad stop word offsets");
            stop.emplace_back(stop_words + start, stop_words + end);
            start = end;
        }
        return stop;
    }
    // ... and back, into a row of [2][STOP_LW]
    static void build_word_list(const StopWords& stop, int* row)
    {
        std::fill(row, row + STOP_LW, 0);
        std::fill(row + STOP_LW, row + 2 * STOP_LW, -1);
        int pos = 0, k = 0;
        for (const auto& wd : stop) {
            std::copy(wd.begin(), wd.end(), row + pos);
            pos += (int)wd.size();
            row[STOP_LW + k++] = pos;
        }
    }
    // stop_criteria_kernels.cu:24-83: does the history END with one of the stop sequences?
    static bool ends_with_stop(const StopWords& stop, const std::vector<int>& hist)
    {
        for (const auto& wd : stop) {
            if (!wd.empty() && hist.size() >= wd.size() && std::equal(wd.begin(), wd.end(), hist.end() - wd.size())) {
                return true;
            }
        }
        return false;
    }
    static bool hits_stop_word(const Slot& s)
    {
        return ends_with_stop(s.stop, s.hist);
    }

    // ---- submit ------------------------------------------------------------------------------------------------------
    // the checks both kinds of request share (K: beam width), then the request itself at the queue's tail
    void check_request(const int* ids, int n, int max_new, int K, float repetition_penalty) const
    {
        // (the decode step stages total_len = max_len + 2 history entries: the same bound as launch_dynamic_decode's)
        FTCF_CHECK_ARG(((std::size_t)max_len + 2) * 8 <= 60 * 1024 || repetition_penalty == 1.f,
                       "max_seq_len too large for the repetition-penalty staging buffer");
        FTCF_CHECK_ARG(ids && n >= 1 && max_new >= 1, "empty prompt or max_new_tokens < 1");
        FTCF_CHECK_ARG(n + max_new <= max_len && n <= max_prompt, "prompt + max_new_tokens exceed the batcher's max_seq_len");
        FTCF_CHECK_ARG(K * pages_needed(n, max_new) <= num_pages, "the request needs more pages than the pool has");
    }
    long enqueue(Request& r, const int* ids, int n, const int* stop_words, int stop_len)
    {
        for (int i = 0; i < n; i++) {
            FTCF_CHECK_ARG(ids[i] >= 0 && ids[i] < vocab, "token id out of range");
        }
        r.prompt.assign(ids, ids + n);
        r.stop = parse_word_list(stop_words, stop_len);
        r.id   = next_id++;
        waiting.push_back(std::move(r));
        return waiting.back().id;
    }
    long submit(const int* ids, int n, int max_new, int top_k, float top_p, float temperature, uint64_t seed,
                float repetition_penalty = 1.f, const int* stop_words = nullptr, int stop_len = 0)
    {
        FTCF_CHECK_ARG(repetition_penalty > 0.f, "repetition_penalty must be positive");
        FTCF_CHECK_ARG(stop_len >= 0 && stop_len <= STOP_LW && (stop_len == 0 || stop_words), "bad stop word list");
        check_request(ids, n, max_new, 1, repetition_penalty);
        FTCF_CHECK_ARG(top_k >= 0 && top_k <= 1024 && top_p >= 0.f && top_p <= 1.f && temperature > 0.f, "bad sampling parameters");
        Request r;
        r.max_new = max_new;
        r.top_k = top_k;
        r.top_p = top_p;
        r.temperature = temperature;
        r.seed = seed;
        r.repetition_penalty = repetition_penalty;
        return enqueue(r, ids, n, stop_words, stop_len);
    }
    // the logit processors of a request, checked (ftcf_batcher_submit_opts: what is invalid)
    LogitOptions make_logit_options(float presence, float frequency, int min_new, const int* bias_ids, const float* bias_values,
                                    int n_bias, const int* bad_words, int bad_len) const
    {
        LogitOptions o;
        FTCF_CHECK_ARG(std::isfinite(presence) && std::isfinite(frequency), "presence_penalty and frequency_penalty must be finite");
        FTCF_CHECK_ARG(min_new >= 0, "min_new_tokens must not be negative");
        FTCF_CHECK_ARG(n_bias >= 0 && n_bias <= BIAS_MAX && (n_bias == 0 || (bias_ids && bias_values)), "logit_bias takes at most 1024 pairs");
        FTCF_CHECK_ARG(bad_len >= 0 && bad_len <= BAD_LW && (bad_len == 0 || bad_words), "bad_words holds at most 256 tokens");
        o.presence  = presence;
        o.frequency = frequency;
        o.min_new   = min_new;
        std::set<int> seen;
        for (int i = 0; i < n_bias; i++) {
            FTCF_CHECK_ARG(bias_ids[i] >= 0 && bias_ids[i] < vocab, "logit_bias: token id out of range");
            FTCF_CHECK_ARG(seen.insert(bias_ids[i]).second, "logit_bias: duplicate token id");
            FTCF_CHECK_ARG(!std::isnan(bias_values[i]) && bias_values[i] != INFINITY, "logit_bias: a value is NaN or +inf");
        }
        o.bias_ids.assign(bias_ids, bias_ids + n_bias);
        o.bias_values.assign(bias_values, bias_values + n_bias);
        const StopWords words = parse_word_list(bad_words, bad_len);
        if (!words.empty()) {
            o.bad.assign(2 * BAD_LW, -1);
            std::fill(o.bad.begin(), o.bad.begin() + BAD_LW, 0);
            int pos = 0, k = 0;
            for (const auto& wd : words) {
                for (const int t : wd) {
                    FTCF_CHECK_ARG(t >= 0 && t < vocab, "bad_words: token id out of range");
                    o.bad[pos++] = t;
                }
                o.bad[BAD_LW + k++] = pos;
            }
        }
        return o;
    }
    long submit_opts(const int* ids, int n, int max_new, int top_k, float top_p, float temperature, uint64_t seed,
                     float repetition_penalty, const int* stop_words, int stop_len, LogitOptions opts)
    {
        const long id       = submit(ids, n, max_new, top_k, top_p, temperature, seed, repetition_penalty, stop_words, stop_len);
        waiting.back().lopt = std::move(opts);
        return id;
    }
    // ---- fork requests (submit_n): n samples of one prompt from ONE prompt phase -------------------------------------------------
    // Page accounting of a fork of n siblings over a prompt of S tokens: the S / P full prompt pages are taken once and every
    // sibling's page list references them; each sibling owns the rest of what the plain request would hold -- its first own page
    // receives the prompt's S % P tail rows (fork_own_pages: at full length under reservation, ONE page under overcommit).
    int fork_shared_pages(const Request& r) const
    {
        return (int)r.prompt.size() / P;
    }
    int fork_own_pages(const Request& r) const
    {
        return admission_pages(r) - fork_shared_pages(r);
    }
    // ONE request of n siblings at the queue's tail; ids[i] = sibling i's id (consecutive).  Refused: n outside [1, max_batch], a
    // fork that can never be admitted -- reservation: shared + n * own pages at full length exceed the pool; overcommit: its
    // admission (shared + n pages) or one sibling at full length does.  n == 1: the plain request.
    void submit_n(const int* ids, int n, int max_new, int top_k, float top_p, float temperature, uint64_t seed, float repetition_penalty,
                  const int* stop_words, int stop_len, LogitOptions opts, int n_samples, long* out_ids)
    {
        FTCF_CHECK_ARG(out_ids, "NULL argument");
        FTCF_CHECK_ARG(n_samples >= 1 && n_samples <= max_batch, "n_samples must be in [1, max_batch]");
        if (n_samples == 1) {
            out_ids[0] = submit_opts(ids, n, max_new, top_k, top_p, temperature, seed, repetition_penalty, stop_words, stop_len, std::move(opts));
            return;
        }
        FTCF_CHECK_ARG(ids && n >= 1 && max_new >= 1, "empty prompt or max_new_tokens < 1");
        const int shared = n / P;
        FTCF_CHECK_ARG(overcommit ? shared + 2 * n_samples - 1 <= num_pages  // (its pages and its watermark, plan_admission)
                                  : (long)shared + (long)n_samples * (pages_needed(n, max_new) - shared) <= (long)num_pages,
                       "the fork request needs more pages than the pool has");
        const long first = next_id;
        submit_opts(ids, n, max_new, top_k, top_p, temperature, seed, repetition_penalty, stop_words, stop_len, std::move(opts));
        Request& r  = waiting.back();
        r.n_samples = n_samples;
        for (int i = 0; i < n_samples; i++) {
            r.sibs.push_back(Request::Sibling{first + i, i, {}});
            out_ids[i] = first + i;
        }
        next_id = first + n_samples;
    }
    // sibling `sib` of fork request r as the plain request it is from the fork on
    static Request sibling_request(const Request& r, const Request::Sibling& sib)
    {
        Request q   = r;
        q.id        = sib.id;
        q.seed      = r.seed + (uint64_t)sib.index;
        q.mask      = sib.mask;
        q.n_samples = 1;
        q.sibs.clear();
        return q;
    }
    // a waiting request leaves (cancel): a plain or beam request as a whole, a fork request's sibling alone -- the last one takes
    // the request with it; false: no waiting request has this id
    bool cancel_waiting(const long id)
    {
        for (auto it = waiting.begin(); it != waiting.end(); ++it) {
            if (!it->is_fork()) {
                if (it->id == id) {
                    waiting.erase(it);
                    return true;
                }
                continue;
            }
            for (auto sb = it->sibs.begin(); sb != it->sibs.end(); ++sb) {
                if (sb->id == id) {
                    it->sibs.erase(sb);
                    it->n_samples = (int)it->sibs.size();
                    if (it->sibs.empty()) {
                        waiting.erase(it);
                    }
                    else {
                        it->id = it->sibs.front().id;
                    }
                    return true;
                }
            }
        }
        return false;
    }
    // the pages of a fork admission's slots `sis` (one per sibling, in sibling order): the shared ones -- the hit's cached pages
    // first -- in sibling 0's list, referenced once more by every other sibling's, then each sibling's own.  Every page is in a
    // slot's list the moment it is taken: a throw half way leaves nothing the rollback's release() does not find.
    void take_fork_pages(const std::vector<int>& sis, const Request& r, const std::vector<int>* hit)
    {
        const int shared = fork_shared_pages(r), own = fork_own_pages(r);
        for (const int si : sis) {
            slots[si].pages.clear();
        }
        std::vector<int>& first = slots[sis[0]].pages;
        if (hit) {
            first = *hit;
            for (const int pg : *hit) {
                page_ref[pg]++;
            }
            pindex.touch(r.prompt.data(), (int)hit->size());
        }
        while ((int)first.size() < shared) {
            first.push_back(take_page());
        }
        for (std::size_t i = 1; i < sis.size(); i++) {
            std::vector<int>& l = slots[sis[i]].pages;
            for (int k = 0; k < shared; k++) {
                l.push_back(first[k]);
                page_ref[first[k]]++;
            }
        }
        for (const int si : sis) {
            for (int k = 0; k < own; k++) {
                slots[si].pages.push_back(take_page());
            }
        }
    }
    // a fork admission has succeeded (before commit()): its counters
    void count_fork(const Request& r, const int hit_tokens)
    {
        fk_requests++;
        fk_siblings += r.n_samples;
        fk_shared_pages += (long)(r.n_samples - 1) * fork_shared_pages(r);
        fk_prompt_tokens += (long)r.prompt.size() - hit_tokens;
    }

    // the allowed-token mask of a waiting or running request (NULL clears it); the slot's device row follows before its next step
    void set_token_mask(long id, const unsigned* bits, int n_words)
    {
        const int W = (vocab + 31) / 32;
        std::vector<unsigned> m;
        if (bits) {
            FTCF_CHECK_ARG(n_words == W, "token mask: n_words must be ceil(vocab_size / 32)");
            m.assign(bits, bits + W);
            if (vocab % 32) {
                m[W - 1] &= (1u << (vocab % 32)) - 1u;
            }
            FTCF_CHECK_ARG(std::any_of(m.begin(), m.end(), [](unsigned w) { return w != 0u; }), "token mask: no token of the vocabulary is allowed");
        }
        for (Request& r : waiting) {
            for (Request::Sibling& sb : r.sibs) {  // (a fork request: the mask is the sibling's own)
                if (sb.id == id) {
                    sb.mask = std::move(m);
                    return;
                }
            }
            if (r.id == id && !r.is_fork()) {
                FTCF_CHECK_ARG(r.beam_width == 1, "token mask: beam requests take no mask");
                r.mask = std::move(m);
                return;
            }
        }
        for (Slot& s : slots) {
            if (s.active && s.id == id) {
                FTCF_CHECK_ARG(s.group < 0, "token mask: beam requests take no mask");
                s.mask       = std::move(m);
                s.mask_dirty = true;
                return;
            }
        }
        for (Swapped& w : swapped) {  // (a swapped-out request: its slot's row follows when it resumes)
            if (w.s.id == id) {
                w.s.mask = std::move(m);
                return;
            }
        }
        FTCF_CHECK_ARG(false, "token mask: no waiting or running request has this id");
    }
    // a beam-search request (GptNeoXOp.forward with beam_width > 1: OnlineBeamSearchLayer): K consecutive slots; one event when
    // it has finished (token = -1), the K hypotheses through beam_result()
    long submit_beam(const int* ids, int n, int max_new, int beam_width, float diversity, float len_penalty, float temperature,
                     float repetition_penalty, int min_length = 0, const int* stop_words = nullptr, int stop_len = 0,
                     bool token_log_probs = false)
    {
        FTCF_CHECK_ARG(min_length >= 0, "min_length must not be negative");
        FTCF_CHECK_ARG(stop_len >= 0 && stop_len <= STOP_LW && (stop_len == 0 || stop_words), "bad stop word list");
        FTCF_CHECK_ARG(beam_width >= 2 && beam_width <= MAX_BEAM_WIDTH && beam_width <= max_batch,
                       "beam_width must be in [2, 64] and fit the batcher's slots");
        FTCF_CHECK_ARG(repetition_penalty > 0.f && temperature > 0.f, "repetition_penalty and temperature must be positive");
        check_request(ids, n, max_new, beam_width, repetition_penalty);
        Request r;
        r.max_new = max_new;
        r.top_k = 1;
        r.top_p = 0.f;
        r.temperature = temperature;
        r.seed = 0;
        r.repetition_penalty = repetition_penalty;
        r.beam_width = beam_width;
        r.diversity = diversity;
        r.len_penalty = len_penalty;
        r.min_length = min_length;
        r.token_log_probs = token_log_probs;
        return enqueue(r, ids, n, stop_words, stop_len);
    }

    // ---- planning ----------------------------------------------------------------------------------------------------
    // The next admission, or kind none when nothing fits.  Called after the iteration's decode step; `any`: slots were running
    // BEFORE that step (a hit and the choice of chunked_one read it; beam and each chunked_one read what runs now).
    //   * FIFO: nobody overtakes the head of the queue;
    //   * a beam request: alone, K consecutive free slots and the group's whole page budget;
    //   * a fork request (submit_n): alone, n free slots, its shared pages once and every sibling's own (take_fork_pages);
    //   * a prefix hit: alone, its budget computed with its own hit pages pinned;
    //   * else as many of the queue's head requests as there are free slots and pages: one at a time (chunked_one, see
    //     next_chunked) when slots were running and one of the prompts is long, else as ONE ragged batch.
    Admission plan_admission(const bool any)
    {
        Admission a;
        if (waiting.empty() || !swapped.empty()) {  // (overcommit: a swapped-out request resumes before anybody is admitted)
            return a;
        }
        int pages_left = pages_available();
        // overcommit: an ordinary admission leaves a watermark of one page per running ordinary slot (the ones this plan has
        // admitted so far included), so that it cannot itself cause a preemption within the next P steps; none runs: waived
        const int running = overcommit ? running_ordinary() : 0;
        if (waiting.front().beam_width > 1) {
            const Request& r = waiting.front();
            const int      K = r.beam_width, need = K * pages_needed((int)r.prompt.size(), r.max_new);
            int            si0 = -1;
            for (int si = 0, run = 0; si < max_batch && si0 < 0; si++) {
                run = slots[si].active ? 0 : run + 1;
                if (run == K) {
                    si0 = si - K + 1;
                }
            }
            if (si0 < 0 || pages_left < need) {
                return a;
            }
            a.kind = Kind::beam;
            for (int k = 0; k < K; k++) {
                a.slots.push_back(si0 + k);
                slot_topk[si0 + k] = 1;
                slot_temp[si0 + k] = 1.f;
            }
            // slots are running and the prompt is long: its prompt phase in chunks, a decode step of the running slots after every
            // chunk (the events of those steps are final whatever happens to the admission)
            a.install_hook = any_active() && prefill_chunk > 0 && (int)r.prompt.size() > prefill_chunk;
            // (overcommit: the hook's decode steps take pages too, and the group opens only after the prompt phase)
            inflight_reserve = overcommit ? need : 0;
            take_head(a);
            return a;
        }
        if (waiting.front().is_fork()) {
            // alone, in n free slots (any n: the siblings are ordinary sequences); the budget with the hit's pages pinned, as a hit's;
            // overcommit: the watermark the last of n plain requests planned together would leave
            const Request&   r = waiting.front();
            const int        n = r.n_samples, S = (int)r.prompt.size();
            std::vector<int> sis;
            for (int si = 0; si < max_batch && (int)sis.size() < n; si++) {
                if (!slots[si].active) {
                    sis.push_back(si);
                }
            }
            if ((int)sis.size() < n) {
                return a;
            }
            std::vector<int> h;
            if (prefix_on) {
                h = pindex.lookup(r.prompt.data(), (S - 1) / P);
            }
            for (const int pg : h) {
                page_ref[pg]++;
            }
            const int avail = pages_available();
            for (const int pg : h) {
                page_ref[pg]--;
            }
            const int need = fork_shared_pages(r) - (int)h.size() + n * fork_own_pages(r);
            if (avail < need + (overcommit ? running + n - 1 : 0)) {
                return a;
            }
            a.kind         = Kind::fork;
            a.install_hook = any && prefill_chunk > 0 && S - (int)h.size() * P > prefill_chunk;
            a.hit          = std::move(h);
            for (const int si : sis) {
                slot_topk[si] = keff(r.top_k, r.top_p);
                slot_temp[si] = r.temperature;
                a.slots.push_back(si);
            }
            take_head(a);
            return a;
        }
        for (int si = 0; si < max_batch && !waiting.empty(); si++) {
            if (slots[si].active) {
                continue;
            }
            const Request& r = waiting.front();
            if (r.beam_width > 1 || r.is_fork()) {
                break;  // (admitted alone, by the next iteration)
            }
            int       need      = admission_pages(r);
            const int watermark = overcommit ? running + (int)a.slots.size() : 0;
            if (prefix_on) {
                // at most floor((S - 1) / P) blocks: the last prompt token is always computed (its logits give the first token)
                // and decode never writes into a cached page
                std::vector<int> h = pindex.lookup(r.prompt.data(), ((int)r.prompt.size() - 1) / P);
                if (!h.empty()) {
                    if (!a.slots.empty()) {
                        break;  // (admitted alone, by the next iteration)
                    }
                    // the budget without the pages this hit pins: they are in use, not evictable
                    for (const int pg : h) {
                        page_ref[pg]++;
                    }
                    const int avail = pages_available();
                    for (const int pg : h) {
                        page_ref[pg]--;
                    }
                    need -= (int)h.size();
                    if (avail < need + watermark) {
                        break;
                    }
                    // the tail's prompt phase from the hit offset, in chunks with decode steps between them when it is long
                    a.kind         = Kind::hit;
                    a.install_hook = any && prefill_chunk > 0 && (int)r.prompt.size() - (int)h.size() * P > prefill_chunk;
                    a.hit          = std::move(h);
                    take_head(a, si);
                    return a;
                }
            }
            if (pages_left < need + watermark) {
                break;  // FIFO: nobody overtakes the head of the queue
            }
            pages_left -= need;
            take_head(a, si);
        }
        if (a.slots.empty()) {
            return a;
        }
        bool any_long = false;
        for (const Request& r : a.requests) {
            any_long |= prefill_chunk > 0 && (int)r.prompt.size() > prefill_chunk;
        }
        // slots are running and a long prompt arrives: one request at a time, its prompt phase in chunks with a decode step of
        // the running slots after every chunk
        a.kind         = any && any_long ? Kind::chunked_one : Kind::ragged;
        a.install_hook = a.kind == Kind::chunked_one && any_active();
        return a;
    }
    // after a chunked_one admission has succeeded: on to the next of its requests (false: that was the last)
    bool next_chunked(Admission& a)
    {
        a.slots.erase(a.slots.begin());
        a.requests.erase(a.requests.begin());
        // overcommit: the decode steps inside the admission took pages and may have swapped somebody out; when the next request
        // no longer fits, or somebody waits to resume, the rest of the plan returns to the queue's head
        if (overcommit && !a.slots.empty()
            && (!swapped.empty() || pages_grantable() < admission_pages(a.requests[0]) + running_ordinary())) {
            for (std::size_t i = a.requests.size(); i-- > 0;) {
                waiting.push_front(std::move(a.requests[i]));
            }
            a.requests.clear();
            a.slots.clear();
        }
        a.install_hook = any_active();
        return !a.slots.empty();
    }
    // a failed admission: what it holds goes back by kind (release_group(si): the group's pages and slots, its parked result;
    // retire(si): the slot's pages -- ftcf_batcher passes its own, which also tell the device), then its requests return to the
    // queue's head in their order
    template<typename Retire, typename ReleaseGroup>
    void rollback(Admission& a, Retire retire, ReleaseGroup release_group)
    {
        inflight_reserve = 0;
        if (a.kind == Kind::beam) {
            release_group(a.slots[0]);
        }
        else {
            for (const int si : a.slots) {  // (chunked_one: this request and the ones not yet admitted)
                retire(si);
            }
        }
        for (std::size_t i = a.requests.size(); i-- > 0;) {
            waiting.push_front(std::move(a.requests[i]));
        }
        a.requests.clear();
    }
    // a successful admission of ordinary requests: their full prompt blocks enter the index (first writer wins), then the slots
    // whose request ended with its first token are released
    void commit(const std::vector<int>& sis, const std::vector<Request>& rs, std::size_t n, int hit_tokens = 0)
    {
        if (!prefix_on) {
            return;
        }
        for (std::size_t i = 0; i < n; i++) {
            const Request& r = rs[i];
            const int      S = (int)r.prompt.size();
            pindex.insert(r.prompt.data(), S / P, slots[sis[i]].pages, page_ref);
            px_lookups++;
            px_prompt_tokens += S;
            px_hit_tokens += hit_tokens;
            px_computed_tokens += S - hit_tokens;
        }
        for (const int si : deferred) {
            release(slots[si]);
        }
        deferred.clear();
    }

    // ---- the host side of an admission's prompt phase and of the decode steps -------------------------------------------
    // the pages of a request's slot: the hit's cached ones (pinned: the slot's page list owns one reference), the rest fresh
    void take_slot_pages(const int si, const Request& r, const std::vector<int>* hit)
    {
        Slot& s = slots[si];
        s.pages.clear();
        if (hit) {
            s.pages = *hit;
            for (const int pg : *hit) {
                page_ref[pg]++;
            }
            pindex.touch(r.prompt.data(), (int)hit->size());
        }
        for (int k = (int)s.pages.size(), need = admission_pages(r); k < need; k++) {
            s.pages.push_back(take_page());
        }
    }
    // the slot runs the request from its first token on; true: that token ended it already
    bool start_slot(const int si, const Request& r, const int first, const int end_id)
    {
        Slot& s = slots[si];
        s.hist.assign(r.prompt.begin(), r.prompt.end());
        s.hist.push_back(first);
        s.stop               = r.stop;
        s.repetition_penalty = r.repetition_penalty;
        s.lopt               = r.lopt;
        s.mask               = r.mask;
        s.lopt_dirty = s.mask_dirty = true;
        s.top_k              = r.top_k;
        s.top_p              = r.top_p;
        s.temperature        = r.temperature;
        s.seed               = r.seed;
        s.active             = true;
        s.id                 = r.id;
        s.len                = (int)r.prompt.size();
        s.generated          = 1;
        s.max_new            = r.max_new;
        return first == end_id || s.generated >= s.max_new || hits_stop_word(s);
    }
    // ... and when it did: the slot leaves now, or (prefix cache: its prompt pages are inserted first) with commit()
    void end_with_first_token(const int si)
    {
        if (prefix_on) {
            deferred.push_back(si);
        }
        else {
            release(slots[si]);
        }
    }
    // a beam request's group: the prompt's pages, shared by every beam
    BeamGroup& open_group(const int si, const Request& r)
    {
        const int n = (int)r.prompt.size();
        inflight_reserve = 0;  // (from here on the group's budget is the promise)
        BeamGroup g;
        g.id        = r.id;
        g.si        = si;
        g.K         = r.beam_width;
        g.n         = n;
        g.max_new   = r.max_new;
        g.budget    = g.K * pages_needed(n, r.max_new);
        g.penalised = r.repetition_penalty != 1.f;
        g.has_min   = r.min_length > 0;
        g.has_stop  = !r.stop.empty();
        g.token_log_probs = r.token_log_probs;
        std::vector<int> shared;
        try {
            for (int i = 0; i < (n + P - 1) / P; i++) {
                shared.push_back(take_page());
            }
        }
        catch (...) {  // (no group owns them yet: drop_group(si) would not find them)
            for (int pg : shared) {
                drop_page(pg);
            }
            throw;
        }
        g.lists.assign(g.K, shared);
        for (int pg : shared) {
            page_ref[pg] = g.K;
        }
        return groups[si] = std::move(g);
    }
    void start_group_slots(BeamGroup& g)
    {
        for (int k = 0; k < g.K; k++) {
            Slot& s  = slots[g.si + k];
            s.active = true;
            s.group  = g.si;
            s.id     = g.id;
            s.len    = g.n;
            s.pages.clear();
            s.hist.clear();
            s.stop.clear();
            s.lopt = LogitOptions{};
            s.mask.clear();
            s.repetition_penalty = 1.f;  // (the beam kernels apply the request's penalty themselves)
        }
        g.generated = 1;
    }
    // every unfinished beam gets a page of its OWN for position `pos` (the next append): a fresh one on a page boundary, a copy
    // of the shared one otherwise; returns the copies to make, {src, dst} page ids
    std::vector<int> take_append_pages(BeamGroup& g, const int pos, const std::vector<uint8_t>& fin)
    {
        std::vector<int> pairs;
        for (int k = 0; k < g.K; k++) {
            if (fin[k]) {
                continue;  // (a finished beam appends nothing: it keeps what it shares)
            }
            std::vector<int>& l = g.lists[k];
            if (pos / P >= (int)l.size()) {
                l.push_back(take_page());
            }
            else if (page_ref[l[pos / P]] > 1) {
                const int old = l[pos / P], pg = take_page();
                pairs.push_back(old);
                pairs.push_back(pg);
                drop_page(old);
                l[pos / P] = pg;
            }
        }
        return pairs;
    }
    // after a beam step: every beam takes over its parent's pages
    void reparent_group(BeamGroup& g, const std::vector<int>& parent)
    {
        std::vector<std::vector<int>> nl(g.K);
        for (int k = 0; k < g.K; k++) {
            nl[k] = g.lists[parent[k] % g.K];
            for (int pg : nl[k]) {
                page_ref[pg]++;
            }
        }
        for (int k = 0; k < g.K; k++) {
            for (int pg : g.lists[k]) {
                drop_page(pg);
            }
        }
        g.lists = std::move(nl);
        g.generated += 1;
    }
    // host view of the running slots' sampling parameters (kernel selection and LDS sizing of the sampling kernels): after every
    // admission, and before a decode step that runs inside an admission (a request admitted a moment ago is already running)
    void refresh_host_flags()
    {
        host_max_top_k = 1;
        host_any_top_p = 0;
        host_any_temperature = false;
        host_any_repetition = false;
        for (int si = 0; si < max_batch; si++) {
            if (slots[si].active) {
                host_any_repetition |= (slots[si].repetition_penalty != 1.f);
                host_max_top_k = std::max(host_max_top_k, slot_topk[si]);
                host_any_top_p |= (slot_topk[si] == 0);
                host_any_temperature |= (slot_temp[si] != 1.f);
            }
        }
    }

private:
    // the queue's head into the admission (ordinary requests: into slot si, with the slot's sampling parameters)
    void take_head(Admission& a, const int si = -1)
    {
        if (si >= 0) {
            const Request& r = waiting.front();
            slot_topk[si]    = keff(r.top_k, r.top_p);
            slot_temp[si]    = r.temperature;
            a.slots.push_back(si);
        }
        a.requests.push_back(std::move(waiting.front()));
        waiting.pop_front();
    }
};

}  // namespace ftcf
