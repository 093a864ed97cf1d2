// Host check of the continuous batcher's scheduler state (fastertransformer4codefuse_amd/csrc/batcher_sched.h;
// tests/test_batcher_sched_host.py).  Drives BatcherSched the way batcher.hip does -- submit / step / cancel / clear -- with a
// FAKE prompt phase that takes pages where admit / admit_beam take them and then succeeds or throws at a seeded point, and fake
// decode steps that finish sequences and make beams diverge (take_append_pages / reparent_group).  After every operation:
//   * page_ref[pg] == the holders of pg (slot page lists, beam page lists, index nodes); the free list is exactly the pages
//     nobody holds, each once;
//   * reserved_pages() + the pages requests hold never exceed the pool;
//   * `slot.active && slot.group >= 0` <=> the slot belongs to a group in `groups` (what lets one "anything live" test serve
//     every chunk hook);
//   * an admitted set is a prefix of the queue; after a failed admission of any kind the queue is in the order it had before
//     planning, none of the admission's slots is active, no group of its id exists (evictions and the free list's order may differ);
//   * take_page never meets an empty pool when planning said the admission fits.
// Prints one "<case>: ok, ..." line per geometry with the admissions and injected failures of every kind; exits non-zero on the
// first violation.
#include "batcher_sim.h"

struct Sim : BatcherSim {
    static constexpr int VOCAB = 6;
    long admitted[5] = {0, 0, 0, 0, 0}, failed[5] = {0, 0, 0, 0, 0}, steps = 0;

    Sim(int pages, int mb, int p, bool cache, unsigned seed): BatcherSim(seed, 5)
    {
        init_sched(mb, p, pages, 4 * p, VOCAB, cache);
        prefill_chunk = p;  // a prompt of more than one page is "long"
    }

    // ---- the fake device side --------------------------------------------------------------------------------------------
    // ftcf_batcher::admit: pages of every slot, the prompt phase (chunks, decode steps between them), first tokens
    void admit(const std::vector<int>& sis, const std::vector<Request>& rs, const int n, const std::vector<int>* hit) override
    {
        deferred.clear();
        for (int i = 0; i < n; i++) {
            take_slot_pages(sis[i], rs[i], hit);
            point();
        }
        hook();
        point();
        hook();
        for (int i = 0; i < n; i++) {
            if (start_slot(sis[i], rs[i], rnd(0, VOCAB - 1), END_ID)) {
                end_with_first_token(sis[i]);
            }
            point();
        }
    }
    // ftcf_batcher::decode + advance_groups, host side
    void decode() override
    {
        for (Slot& s : slots) {
            if (!s.active || s.group >= 0) {
                continue;
            }
            s.len += 1;
            s.generated += 1;
            s.hist.push_back(rnd(0, VOCAB - 1));
            CHECK(s.len <= (int)s.pages.size() * P, "a slot of %d tokens on %zu pages", s.len, s.pages.size());
            if (s.hist.back() == END_ID || s.generated >= s.max_new || hits_stop_word(s)) {
                release(s);
            }
        }
        decode_groups();
    }
    // ftcf_batcher::step / run_admission
    void step(const bool inject)
    {
        steps++;
        const bool any = any_active();
        if (any) {
            decode();
            check_pages("a decode step");
        }
        const std::vector<long> before = queue_ids();
        Admission               a      = plan_admission(any);
        if (a.kind == Kind::none) {
            CHECK(queue_ids() == before, "planning nothing changed the queue");
            refresh_host_flags();
            return;
        }
        const std::vector<long> rest = queue_ids();
        CHECK(a.requests.size() + rest.size() == before.size(), "planning lost a request");
        for (size_t i = 0; i < before.size(); i++) {
            CHECK(before[i] == (i < a.requests.size() ? a.requests[i].id : rest[i - a.requests.size()]), "the admitted set is no prefix");
        }
        CHECK(a.kind != Kind::hit || prefix_on, "a hit without a cache");
        size_t done = 0;  // requests of this plan that are in
        do {
            const Kind             kind = a.kind;
            const std::vector<int> sis  = a.slots;
            const long             id   = a.requests[0].id;
            const int              n    = kind == Kind::chunked_one ? 1 : (int)a.requests.size();
            try {
                prompt_phase(a, n, inject);
            }
            catch (const Injected&) {
                roll_back(a, sis, id, std::vector<long>(before.begin() + done, before.end()));
                failed[(int)kind]++;
                check_pages("a failed admission");
                return;  // (the exception leaves step(): no refresh_host_flags)
            }
            if (kind != Kind::beam) {
                commit(a.slots, a.requests, n, (int)a.hit.size() * P);
            }
            admitted[(int)kind]++;
            done += n;
            check_pages("an admission");
        } while (a.kind == Kind::chunked_one && next_chunked(a));
        refresh_host_flags();
    }

    // ---- the callers -----------------------------------------------------------------------------------------------------
    void submit_random()
    {
        // prompts share stems (prefix hits), token 0 is the end id
        const int        n = rnd(1, 3 * P), stem = rnd(1, 2), max_new = rnd(1, 2 * P);
        std::vector<int> ids(n);
        for (int i = 0; i < n; i++) {
            ids[i] = 1 + (stem * (i / 3 + 1) + i) % (VOCAB - 1);
        }
        if (rnd(0, 3) == 0) {
            ids[rnd(0, n - 1)] = rnd(1, VOCAB - 1);
        }
        // a word list of two tokens (to_word_list_format: ids, then end offsets): two words of one token, or one of two
        const bool with_stop = rnd(0, 3) == 0, two_words = rnd(0, 1) == 1;
        const int  stop_list[4] = {rnd(1, VOCAB - 1), rnd(1, VOCAB - 1), two_words ? 1 : 2, two_words ? 2 : -1};
        const bool beam = max_batch >= 2 && rnd(0, 3) == 0;
        try {
            if (beam) {
                submit_beam(ids.data(), n, max_new, rnd(2, std::min(4, max_batch)), 0.f, 0.f, 1.f, 1.f, 0, with_stop ? stop_list : nullptr,
                            with_stop ? 2 : 0);
            }
            else {
                submit(ids.data(), n, max_new, rnd(0, 2), 0.f, 1.f, 7, 1.f, with_stop ? stop_list : nullptr, with_stop ? 2 : 0);
            }
        }
        catch (const ftcf::Error& e) {
            CHECK(e.code == -1, "submit: %s", e.what());  // (a request the geometry cannot hold)
            return;
        }
        const Request& r = waiting.back();
        int            row[2 * STOP_LW];
        build_word_list(r.stop, row);
        CHECK(parse_word_list(row, STOP_LW) == r.stop && r.stop.size() == (with_stop ? (two_words ? 2u : 1u) : 0u),
              "the word list does not round-trip");
    }
    void cancel_random()  // ftcf_batcher_cancel, host side
    {
        if (!waiting.empty() && rnd(0, 1)) {
            waiting.erase(waiting.begin() + rnd(0, (int)waiting.size() - 1));
            return;
        }
        Slot& s = slots[rnd(0, max_batch - 1)];
        if (s.active && s.group >= 0) {
            drop_group(s.group);
        }
        else if (s.active) {
            release(s);
        }
    }
};

static void run_case(const char* name, int pages, int mb, int p, bool cache, unsigned seed)
{
    Sim sim(pages, mb, p, cache, seed);
    try {
        for (int op = 0; op < 6000; op++) {
            const int what = sim.rnd(0, 99);
            if (what < 40) {
                sim.submit_random();
                sim.check_pages("submit");
            }
            else if (what < 92) {
                sim.step(sim.rnd(0, 3) == 0);
            }
            else if (what < 98) {
                sim.cancel_random();
                sim.check_pages("cancel");
            }
            else {
                sim.clear_prefix_cache();
                sim.check_pages("clear_prefix_cache");
            }
        }
        // drain: everything leaves, the pool has all its pages back
        sim.waiting.clear();
        for (int i = 0; i < 8 * p && sim.any_active(); i++) {
            sim.step(false);
        }
        sim.clear_prefix_cache();
        sim.check_pages("the drain");
        CHECK(!sim.any_active() && (int)sim.free_pages.size() == pages, "%zu of %d pages are back", sim.free_pages.size(), pages);
    }
    catch (const ftcf::Error& e) {
        CHECK(false, "%s", e.what());  // ("the page pool is exhausted (a reservation was wrong)")
    }
    const long *a = sim.admitted, *f = sim.failed;
    std::printf("%s: ok, %ld steps, admitted beam %ld hit %ld chunked_one %ld ragged %ld, failed beam %ld hit %ld chunked_one %ld ragged %ld, "
                "%ld decode steps inside admissions, %ld evictions\n",
                name, sim.steps, a[1], a[2], a[3], a[4], f[1], f[2], f[3], f[4], sim.decodes_in_hook, sim.px_evictions);
}

int main()
{
    run_case("6 pages 2 slots P8", 6, 2, 8, false, 1);
    run_case("6 pages 2 slots P8 cache", 6, 2, 8, true, 2);
    run_case("10 pages 4 slots P8", 10, 4, 8, false, 3);
    run_case("12 pages 4 slots P16 cache", 12, 4, 16, true, 4);
    run_case("16 pages 3 slots P16", 16, 3, 16, false, 5);
    run_case("16 pages 3 slots P16 cache", 16, 3, 16, true, 6);
    run_case("24 pages 8 slots P8", 24, 8, 8, false, 7);
    run_case("24 pages 8 slots P8 cache", 24, 8, 8, true, 8);
    return 0;
}
