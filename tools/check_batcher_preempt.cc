// Host check of the continuous batcher's OVERCOMMIT policy (fastertransformer4codefuse_amd/csrc/batcher_sched.h, DESIGN.md §4e;
// tests/test_batcher_preempt_host.py): pages on demand, preemption of the latest arrival by swap, resume before admission.
// Drives BatcherSched with overcommit on the way batcher.hip does -- submit / step / cancel / clear -- with FAKE prompt phases
// that take pages where admit / admit_beam take them and succeed or throw at a seeded point, fake decode steps that grow, finish
// and make beams diverge, and fake device halves of swap-out and swap-in.  After every operation:
//   * page_ref[pg] == the holders of pg (slot page lists, beam page lists, index nodes); the free list is exactly the pages
//     nobody holds, each once;
//   * the host pages held == the sum over `swapped`, each once; the host free list is exactly the others;
//   * every request id ever given is in exactly one place -- the queue, `swapped`, a slot (a group's slots count once) -- or has
//     left for good (finished or cancelled); none is lost, none is twice;
//   * `swapped` is in id order; every admission starts with `swapped` empty;
//   * a victim is an active ordinary slot (never a beam, never a slot of an admission in flight) and is the LATEST arrival among
//     the running ordinary slots the free host pages can take: with swap space that cannot fill, never older than one that stayed;
//   * a resumed request finds the draw counter and cumulative log-probability it left with, and pages for all it brings back;
//   * the device's page table row of every running ordinary slot (kept by the fake device halves) is the slot's page list, also
//     after a step that failed for want of swap space when slots had already grown;
//   * a decode step never appends beyond a slot's pages; take_page never throws; "swap space exhausted" only where the swap
//     space is smaller than max_batch * ceil(max_seq_len / P);
//   * after the last submit every geometry drains within (requests left + max_batch) * (max_seq_len + 2) steps.
// Prints one "<case>: ok, ..." line per geometry with the preemptions, the resumes and the resumes into another slot (all > 0);
// exits non-zero on the first violation.
#include "batcher_sim.h"

#include <cstring>

struct Sim : BatcherSim {
    static constexpr int VOCAB = 14;
    bool         can_fill = false; // the swap space is smaller than max_batch * max_pages
    long         steps = 0, admissions = 0, failed = 0, exhausted = 0, resumed_elsewhere = 0, grown = 0;
    std::set<long>      gone;      // ids that finished or were cancelled
    std::map<long, int> left_slot; // a swapped-out request's old slot
    std::vector<std::vector<int>> dev_pt;  // the device's page table rows of ordinary slots, as the device halves leave them
    std::vector<long>   pending;   // requests of a chunked_one plan that are not in yet (they are in the plan, not in the queue)

    Sim(int pages, int mb, int p, bool cache, int swap_pages, unsigned seed): BatcherSim(seed, 7)
    {
        init_sched(mb, p, pages, 4 * p, VOCAB, cache);
        init_overcommit(swap_pages);
        dev_pt.assign(mb, {});
        can_fill      = swap_total < mb * max_pages;
        prefill_chunk = p;  // a prompt of more than one page is "long"
    }
    static uint64_t draws_of(long id)
    {
        return 1000u + 7u * (uint64_t)id;
    }

    // ---- the invariants ------------------------------------------------------------------------------------------------
    void check_all(const char* after)
    {
        check_pages(after);
        std::map<long, int> places;  // id -> places it is in
        for (const Request& r : waiting) {
            places[r.id]++;
        }
        for (const long id : pending) {
            places[id]++;
        }
        long prev = 0;
        for (const Swapped& w : swapped) {
            places[w.s.id]++;
            CHECK(w.s.id > prev, "after %s: `swapped` is not in id order", after);
            prev = w.s.id;
            CHECK(!w.s.active && w.s.pages.empty() && w.s.group < 0, "after %s: a swapped-out request holds pool pages", after);
            CHECK(!w.host.empty() && w.draws == draws_of(w.s.id), "after %s: request %ld lost its device state", after, w.s.id);
        }
        for (const Slot& s : slots) {
            if (s.active && s.group < 0) {
                places[s.id]++;
                CHECK(dev_pt[&s - slots.data()] == s.pages, "after %s: the device's page table row of slot %d is not the slot's page list", after,
                      (int)(&s - slots.data()));
            }
        }
        for (const auto& kv : groups) {
            places[kv.second.id]++;
        }
        for (long id = 1; id < next_id; id++) {
            const int n = places.count(id) ? places[id] : 0;
            CHECK(n + (int)gone.count(id) == 1, "after %s: request %ld is in %d places and %s", after, id, n, gone.count(id) ? "gone" : "not gone");
        }
        // the swap space
        std::vector<int> host_holders(swap_total, 0), host_in_free(swap_total, 0);
        for (const Swapped& w : swapped) {
            for (int hp : w.host) {
                CHECK(hp >= 0 && hp < swap_total && ++host_holders[hp] == 1, "after %s: host page %d is held twice", after, hp);
            }
        }
        for (int hp : host_free) {
            CHECK(hp >= 0 && hp < swap_total && ++host_in_free[hp] == 1, "after %s: host page %d is twice in the free list", after, hp);
        }
        for (int hp = 0; hp < swap_total; hp++) {
            CHECK(host_holders[hp] + host_in_free[hp] == 1, "after %s: host page %d: %d holders, free list %d", after, hp, host_holders[hp],
                  host_in_free[hp]);
        }
        CHECK(inflight_reserve == 0, "after %s: a promise to an admission that is not in flight", after);
    }

    // ---- the fake device side --------------------------------------------------------------------------------------------
    void fake_swap_out(int si, const std::vector<int>& pages, const std::vector<int>& host, uint64_t& draws, float& cum)
    {
        const Slot& s = slots[si];
        CHECK(s.active && s.group < 0, "the victim in slot %d is a beam or not running", si);
        CHECK(&pages == &s.pages && host.size() == pages.size() && !pages.empty(), "a victim's host pages do not match its list");
        for (int o = 0; o < max_batch; o++) {
            const Slot& t = slots[o];
            if (o != si && t.active && t.group < 0 && (!can_fill || t.pages.size() <= host_free.size())) {
                CHECK(t.id < s.id, "victim %ld is older than request %ld, which stays", s.id, t.id);
            }
        }
        for (std::size_t i = 0; i < host.size(); i++) {
            CHECK(std::count(host_free.begin(), host_free.end(), host[i]) == 1, "a victim got a host page that is not free");
        }
        left_slot[s.id] = si;
        draws           = draws_of(s.id);
        cum             = -0.5f * (float)s.id;
    }
    void fake_swap_in(int si, const Swapped& w, const std::vector<int>& pages)
    {
        CHECK(slots[si].active && slots[si].id == w.s.id && slots[si].hist == w.s.hist && slots[si].len == w.s.len, "a resumed slot differs");
        CHECK(pages.size() >= w.host.size() && (int)pages.size() * P > w.s.len, "request %ld resumes on too few pages", w.s.id);
        CHECK(w.draws == draws_of(w.s.id) && w.cum == -0.5f * (float)w.s.id, "request %ld lost its device state", w.s.id);
        CHECK(slots[si].lopt_dirty && slots[si].mask_dirty, "a resumed slot's logit rows are not marked dirty");
        for (int o = 0; o < max_batch; o++) {
            CHECK(o >= si || slots[o].active, "slot %d is free and lower than %d", o, si);
        }
        resumed_elsewhere += left_slot.at(w.s.id) != si ? 1 : 0;
        dev_pt[si] = pages;
    }
    void admit(const std::vector<int>& sis, const std::vector<Request>& rs, const int n, const std::vector<int>* hit) override
    {
        deferred.clear();
        for (int i = 0; i < n; i++) {
            take_slot_pages(sis[i], rs[i], hit);
            CHECK((int)slots[sis[i]].pages.size() == ((int)rs[i].prompt.size() + P) / P, "an admission took other pages than its prompt needs");
            point();
        }
        hook();
        point();
        hook();
        for (int i = 0; i < n; i++) {
            dev_pt[sis[i]] = slots[sis[i]].pages;  // (the row goes up with the slot's state)
            if (start_slot(sis[i], rs[i], rnd(0, VOCAB - 1), END_ID)) {
                end_with_first_token(sis[i]);
                if (!prefix_on) {
                    gone.insert(rs[i].id);
                }
            }
            point();
        }
    }
    void group_finished(const long id) override
    {
        gone.insert(id);
    }
    // ftcf_batcher::decode + advance_groups, host side
    void decode() override
    {
        grown += grow_slots(
            [this](int si, const std::vector<int>& pages, const std::vector<int>& host, uint64_t& draws, float& cum) {
                fake_swap_out(si, pages, host, draws, cum);
            },
            [this](int si) {  // (the row's new last entry, the moment the slot has grown: a later slot may throw)
                CHECK(dev_pt[si].size() + 1 == slots[si].pages.size(), "slot %d grew by other than one page", si);
                dev_pt[si].push_back(slots[si].pages.back());
            });
        for (Slot& s : slots) {
            if (!s.active || s.group >= 0) {
                continue;
            }
            CHECK(s.len < (int)s.pages.size() * P, "request %ld appends token %d beyond its %zu pages", s.id, s.len, s.pages.size());
            s.len += 1;
            s.generated += 1;
            s.hist.push_back(rnd(0, VOCAB - 1));
            if (s.hist.back() == END_ID || s.generated >= s.max_new || hits_stop_word(s)) {
                gone.insert(s.id);
                release(s);
            }
        }
        decode_groups();
    }
    static bool is_exhausted(const ftcf::Error& e)
    {
        return e.code == -2 && std::strstr(e.what(), "swap space exhausted") != nullptr;
    }
    // "swap space exhausted": the caller cancels somebody and calls again
    void on_exhausted(const ftcf::Error& e)
    {
        CHECK(is_exhausted(e), "%s", e.what());
        CHECK(can_fill, "a swap space of max_batch * max_pages pages filled up");
        exhausted++;
        if (!swapped.empty()) {
            const long id = swapped[rnd(0, (int)swapped.size() - 1)].s.id;
            CHECK(drop_swapped(id), "a swapped-out request cannot be cancelled");
            gone.insert(id);
            return;
        }
        int v = -1;  // (nobody is swapped out: every running request is larger than the swap space; the latest arrival goes)
        for (int si = 0; si < max_batch; si++) {
            if (slots[si].active && slots[si].group < 0 && (v < 0 || slots[si].id > slots[v].id)) {
                v = si;
            }
        }
        CHECK(v >= 0, "no swap space, and nobody to cancel");
        gone.insert(slots[v].id);
        release(slots[v]);
    }
    // ftcf_batcher::step / run_admission
    void step(const bool inject)
    {
        steps++;
        const bool any = any_active();
        if (any) {
            try {
                decode();
            }
            catch (const ftcf::Error& e) {
                on_exhausted(e);
                check_all("a decode step without swap space");
                return;
            }
            check_all("a decode step");
        }
        for (int si; (si = plan_resume()) >= 0;) {
            resume(si, [this](int s2, const Swapped& w, const std::vector<int>& pages) { fake_swap_in(s2, w, pages); });
            check_all("a resume");
        }
        const std::vector<long> before = queue_ids();
        Admission               a      = plan_admission(any);
        if (a.kind == Kind::none) {
            CHECK(queue_ids() == before, "planning nothing changed the queue");
            refresh_host_flags();
            return;
        }
        size_t done = 0;  // requests of this plan that are in
        do {
            CHECK(swapped.empty(), "an admission while request %ld is swapped out", swapped.front().s.id);
            const Kind             kind = a.kind;
            const std::vector<int> sis  = a.slots;
            const int              n    = kind == Kind::chunked_one ? 1 : (int)a.requests.size();
            std::vector<long>      ids, ended;
            for (const Request& r : a.requests) {
                ids.push_back(r.id);
            }
            bool ok = true;
            try {
                prompt_phase(a, n, inject);
            }
            catch (const Injected&) {
                ok = false;
            }
            catch (const ftcf::Error& e) {  // (a decode step between the chunks found no swap space)
                on_exhausted(e);
                ok = false;
            }
            pending.assign(ids.begin() + n, ids.end());
            if (!ok) {
                pending.clear();
                roll_back(a, sis, ids[0], std::vector<long>(before.begin() + done, before.end()));
                for (const long id : ids) {
                    gone.erase(id);  // (a request that ended with its first token is back in the queue)
                }
                failed++;
                check_all("a failed admission");
                return;
            }
            for (const int si : deferred) {
                ended.push_back(slots[si].id);
            }
            if (kind != Kind::beam) {
                commit(a.slots, a.requests, n, (int)a.hit.size() * P);
            }
            gone.insert(ended.begin(), ended.end());
            admissions++;
            done += n;
            check_all("an admission");
        } while (a.kind == Kind::chunked_one && next_chunked(a));
        pending.clear();
        check_all("the admissions of a step");
        refresh_host_flags();
    }

    // ---- the callers -----------------------------------------------------------------------------------------------------
    void submit_random()
    {
        // prompts share stems (prefix hits), token 0 is the end id; most requests declare far more than they will use
        const int        n = rnd(1, 2 * P + 2), stem = rnd(1, 2), max_new = rnd(1, 4 * P - n);
        std::vector<int> ids(n);
        for (int i = 0; i < n; i++) {
            ids[i] = 1 + (stem * (i / 3 + 1) + i) % (VOCAB - 1);
        }
        if (rnd(0, 3) == 0) {
            ids[rnd(0, n - 1)] = rnd(1, VOCAB - 1);
        }
        const bool with_stop = rnd(0, 5) == 0;
        const int  stop_list[4] = {rnd(1, VOCAB - 1), rnd(1, VOCAB - 1), 2, -1};
        const bool beam = max_batch >= 3 && rnd(0, 7) == 0;
        try {
            if (beam) {
                submit_beam(ids.data(), n, std::min(max_new, P), 2, 0.f, 0.f, 1.f, 1.f, 0, with_stop ? stop_list : nullptr, with_stop ? 2 : 0);
            }
            else {
                submit(ids.data(), n, max_new, rnd(0, 2), 0.f, 1.f, 7, 1.f, with_stop ? stop_list : nullptr, with_stop ? 2 : 0);
            }
        }
        catch (const ftcf::Error& e) {
            CHECK(e.code == -1, "submit: %s", e.what());  // (a request the geometry cannot hold)
        }
    }
    void cancel_random()  // ftcf_batcher_cancel, host side
    {
        const int what = rnd(0, 2);
        if (what == 0 && !waiting.empty()) {
            auto it = waiting.begin() + rnd(0, (int)waiting.size() - 1);
            gone.insert(it->id);
            waiting.erase(it);
            return;
        }
        if (what == 1 && !swapped.empty()) {
            const long   id   = swapped[rnd(0, (int)swapped.size() - 1)].s.id;
            const size_t free = host_free.size();
            CHECK(drop_swapped(id) && host_free.size() > free, "cancelling a swapped-out request returned no host page");
            gone.insert(id);
            return;
        }
        Slot& s = slots[rnd(0, max_batch - 1)];
        if (s.active && s.group >= 0) {
            gone.insert(s.id);
            drop_group(s.group);
        }
        else if (s.active) {
            gone.insert(s.id);
            release(s);
        }
    }
};

static void run_case(const char* name, int pages, int mb, int p, bool cache, int swap_pages, unsigned seed)
{
    Sim sim(pages, mb, p, cache, swap_pages, seed);
    try {
        for (int op = 0; op < 8000; op++) {
            const int what = sim.rnd(0, 99);
            if (what < 30) {
                sim.submit_random();
                sim.check_all("submit");
            }
            else if (what < 94) {
                sim.step(sim.rnd(0, 5) == 0);
            }
            else if (what < 99) {
                sim.cancel_random();
                sim.check_all("cancel");
            }
            else {
                sim.clear_prefix_cache();
                sim.check_all("clear_prefix_cache");
            }
        }
        // drain: nobody submits any more; everything leaves within the bound, the pool and the swap space have all their pages back
        const long bound = (long)(sim.waiting.size() + sim.swapped.size() + sim.max_batch) * (sim.max_len + 2);
        long       n     = 0;
        while (sim.any_active() || !sim.waiting.empty() || !sim.swapped.empty()) {
            CHECK(n++ < bound, "not drained after %ld steps: %zu waiting, %zu swapped out", bound, sim.waiting.size(), sim.swapped.size());
            sim.step(false);
        }
        sim.clear_prefix_cache();
        sim.check_all("the drain");
        CHECK((int)sim.free_pages.size() == pages && (int)sim.host_free.size() == sim.swap_total, "%zu of %d pages and %zu of %d host pages are back",
              sim.free_pages.size(), pages, sim.host_free.size(), sim.swap_total);
    }
    catch (const ftcf::Error& e) {
        CHECK(false, "%s", e.what());  // ("the page pool is exhausted (a reservation was wrong)")
    }
    CHECK(sim.pe_preemptions > 0 && sim.pe_resumes > 0 && sim.resumed_elsewhere > 0 && sim.pe_pages_in <= sim.pe_pages_out,
          "%s: %ld preemptions, %ld resumes, %ld into another slot", name, sim.pe_preemptions, sim.pe_resumes, sim.resumed_elsewhere);
    std::printf("%s: ok, %ld steps, %ld admissions, %ld failed, %ld pages grown, preemptions %ld, resumes %ld, resumes into another slot %ld, "
                "%ld decode steps inside admissions, %ld evictions, %ld times without swap space\n",
                name, sim.steps, sim.admissions, sim.failed, sim.grown, sim.pe_preemptions, sim.pe_resumes, sim.resumed_elsewhere,
                sim.decodes_in_hook, sim.px_evictions, sim.exhausted);
}

int main()
{
    // (swap space: 0 = as many host pages as the pool has; max_batch * 4 cannot fill; the small ones do)
    run_case("6 pages 2 slots P8", 6, 2, 8, false, 8, 1);
    run_case("6 pages 2 slots P8 cache", 6, 2, 8, true, 0, 2);
    run_case("8 pages 4 slots P8", 8, 4, 8, false, 16, 3);
    run_case("8 pages 4 slots P16 cache", 8, 4, 16, true, 16, 4);
    run_case("9 pages 4 slots P8 swap 2", 9, 4, 8, false, 2, 5);
    run_case("10 pages 6 slots P16 cache swap 2", 10, 6, 16, true, 2, 6);
    run_case("14 pages 8 slots P8", 14, 8, 8, false, 32, 7);
    run_case("14 pages 8 slots P8 cache", 14, 8, 8, true, 0, 8);
    return 0;
}
