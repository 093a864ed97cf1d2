// Host check of the continuous batcher's FORK requests (ftcf_batcher_submit_n: n samples of one prompt from one prompt phase;
// fastertransformer4codefuse_amd/csrc/batcher_sched.h; tests/test_batcher_fork_host.py).  Drives BatcherSched the
// way batcher.hip does -- submit / submit_n / submit_beam / set_token_mask / step / cancel / clear -- with random mixes of plain,
// beam and fork requests, prompt lengths whose tail len % P is 0, 1 and P - 1 among others, under reservation and under
// overcommit, with the prefix cache on and off, and a FAKE prompt phase that takes pages where admit / admit_fork / admit_beam take
// them and succeeds or throws at a seeded point.  After every operation:
//   * page_ref[pg] == the page lists and index entries that hold pg; the free list is exactly the pages nobody holds, each once:
//     free + held == num_pages;
//   * every request id ever given -- a fork's sibling ids each -- is in exactly one place (the queue, a plan not yet admitted,
//     `swapped`, a slot, a group) or has left for good; none is lost, none is twice;
//   * a fork admission gives sibling i the slot's page list {the S / P shared pages, the same for all} + {own pages nobody else
//     holds}: admission_pages(request) in all, of which sibling i's seed is seed + index, its id its own, its mask the one set on
//     that id while it waited; the fork counters move by 1 request, n siblings, (n - 1) * shared pages, S - hit tokens;
//   * a FAILED fork admission leaves none of its slots active, every page back (the accounting above) and the request at the
//     queue's head with the ids and masks it had;
//   * cancelling a waiting sibling shrinks its request by that id alone, the last one removes it;
//   * after the last submit every geometry drains and the pool (and the swap space) is whole.
// Prints one "<case>: ok, ..." line per geometry; fork admissions both succeed and fail in every one (checked here too); exits
// non-zero on the first violation.
#include "batcher_sim.h"

#include <cstring>

struct Sim : BatcherSim {
    static constexpr int VOCAB = 14;
    long                steps = 0, admitted[6] = {0, 0, 0, 0, 0, 0}, failed[6] = {0, 0, 0, 0, 0, 0};
    long                fork_hits = 0, fork_tail[3] = {0, 0, 0}, sib_cancelled = 0, sib_first_token_end = 0, refused = 0;
    std::set<long>      gone;     // ids that finished or were cancelled
    std::vector<long>   pending;  // ids of a chunked_one plan's requests that are not in yet
    const Admission*    cur = nullptr;  // the admission whose prompt phase runs

    Sim(int pages, int mb, int p, bool cache, bool over, unsigned seed): BatcherSim(seed, 5)
    {
        init_sched(mb, p, pages, 4 * p, VOCAB, cache);
        if (over) {
            init_overcommit(mb * 4);  // (max_batch * max_pages host pages: the swap space cannot fill)
        }
        prefill_chunk = p;  // a prompt of more than one page is "long"
    }
    static unsigned mask_of(long id)
    {
        return 2u + (unsigned)(id % 8);  // (bits within the vocabulary, never empty)
    }
    static std::vector<long> ids_of(const Request& r)
    {
        std::vector<long> ids;
        if (!r.is_fork()) {
            ids.push_back(r.id);
        }
        for (const Request::Sibling& sb : r.sibs) {
            ids.push_back(sb.id);
        }
        return ids;
    }

    // ---- the invariants ----------------------------------------------------------------------------------------------------
    void check_all(const char* after)
    {
        check_pages(after);
        std::set<int> held;
        for (const Slot& s : slots) {
            held.insert(s.pages.begin(), s.pages.end());
        }
        for (const auto& kv : groups) {
            for (const auto& l : kv.second.lists) {
                held.insert(l.begin(), l.end());
            }
        }
        for (const auto& n : pindex.nodes) {
            if (n.live && n.page >= 0) {
                held.insert(n.page);
            }
        }
        CHECK((int)free_pages.size() + (int)held.size() == num_pages, "after %s: %zu free + %zu held of %d pages", after, free_pages.size(),
              held.size(), num_pages);
        std::map<long, int> places;
        for (const Request& r : waiting) {
            CHECK(r.is_fork() ? (r.n_samples == (int)r.sibs.size() && r.id == r.sibs.front().id) : r.n_samples == 1,
                  "after %s: request %ld has n_samples %d and %zu siblings", after, r.id, r.n_samples, r.sibs.size());
            for (const long id : ids_of(r)) {
                places[id]++;
            }
        }
        for (const long id : pending) {
            places[id]++;
        }
        for (const Swapped& w : swapped) {
            places[w.s.id]++;
        }
        for (const Slot& s : slots) {
            if (s.active && s.group < 0) {
                places[s.id]++;
            }
        }
        for (const auto& kv : groups) {
            places[kv.second.id]++;
        }
        for (long id = 1; id < next_id; id++) {
            const int n = places.count(id) ? places[id] : 0;
            CHECK(n + (int)gone.count(id) == 1, "after %s: request %ld is in %d places and %s", after, id, n, gone.count(id) ? "gone" : "not gone");
        }
        std::vector<int> host_seen(swap_total, 0);
        for (const Swapped& w : swapped) {
            for (int hp : w.host) {
                CHECK(hp >= 0 && hp < swap_total && ++host_seen[hp] == 1, "after %s: host page %d is held twice", after, hp);
            }
        }
        for (int hp : host_free) {
            CHECK(hp >= 0 && hp < swap_total && ++host_seen[hp] == 1, "after %s: host page %d is free and held", after, hp);
        }
        CHECK(inflight_reserve == 0, "after %s: a promise to an admission that is not in flight", after);
    }

    // ---- the fake device side ----------------------------------------------------------------------------------------------
    // ftcf_batcher::admit_fork: the pages of all siblings, ONE prompt phase, n first tokens
    void admit_fork(const std::vector<int>& sis, const Request& r)
    {
        const int n = r.n_samples, S = (int)r.prompt.size(), shared = fork_shared_pages(r), own = fork_own_pages(r);
        CHECK((int)sis.size() == n && (int)r.sibs.size() == n && n >= 1, "a fork of %d siblings in %zu slots", n, sis.size());
        CHECK(std::set<int>(sis.begin(), sis.end()).size() == sis.size(), "a fork admission names a slot twice");
        deferred.clear();
        take_fork_pages(sis, r, cur->hit.empty() ? nullptr : &cur->hit);
        point();
        hook();
        point();
        hook();
        // every sibling: the shared pages first, the same for all; then pages of its own
        const std::vector<int>& first = slots[sis[0]].pages;
        CHECK(shared + own == admission_pages(r) && own >= 1, "%d shared + %d own pages, a plain request takes %d", shared, own, admission_pages(r));
        for (int i = 0; i < n; i++) {
            const std::vector<int>& l = slots[sis[i]].pages;
            CHECK((int)l.size() == shared + own && (int)l.size() * P > S, "sibling %d holds %zu pages", i, l.size());
            CHECK(std::equal(l.begin(), l.begin() + shared, first.begin()), "sibling %d does not share the prompt's pages", i);
            for (int k = 0; k < shared; k++) {
                CHECK(page_ref[l[k]] >= n, "a shared page has %d references for %d siblings", page_ref[l[k]], n);
                CHECK(k >= (int)cur->hit.size() || l[k] == cur->hit[k], "a sibling's first pages are not the hit's");
            }
            for (int k = shared; k < shared + own; k++) {
                CHECK(page_ref[l[k]] == 1, "a sibling's own page has %d references", page_ref[l[k]]);
            }
        }
        for (int i = 0; i < n; i++) {
            const Request q = sibling_request(r, r.sibs[i]);
            CHECK(q.id == r.sibs[i].id && q.seed == r.seed + (uint64_t)r.sibs[i].index && !q.is_fork() && q.n_samples == 1,
                  "sibling %d is not the plain request of seed + index", i);
            const bool ended = start_slot(sis[i], q, rnd(0, VOCAB - 1), END_ID);
            const Slot& s = slots[sis[i]];
            CHECK(s.active && s.group < 0 && s.id == q.id && s.seed == q.seed && s.len == S && s.generated == 1, "sibling %d's slot", i);
            CHECK(s.mask == ((q.id % 3 == 0) ? std::vector<unsigned>(1, mask_of(q.id)) : std::vector<unsigned>()), "sibling %ld's mask", q.id);
            if (ended) {
                sib_first_token_end++;
                end_with_first_token(sis[i]);
                if (!prefix_on) {
                    gone.insert(q.id);
                }
            }
            point();
        }
    }
    void admit(const std::vector<int>& sis, const std::vector<Request>& rs, const int n, const std::vector<int>* hit) override
    {
        if (cur->kind == Kind::fork) {
            CHECK(n == 1 && rs.size() == 1 && rs[0].is_fork(), "a fork admission of %d requests", n);
            admit_fork(sis, rs[0]);
            return;
        }
        deferred.clear();
        for (int i = 0; i < n; i++) {
            CHECK(!rs[i].is_fork(), "a fork request in a batch of plain ones");
            take_slot_pages(sis[i], rs[i], hit);
            point();
        }
        hook();
        point();
        hook();
        for (int i = 0; i < n; i++) {
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
        grow_slots([](int, const std::vector<int>&, const std::vector<int>&, uint64_t& draws, float& cum) { draws = 1, cum = 0.f; }, [](int) {});
        for (Slot& s : slots) {
            if (!s.active || s.group >= 0) {
                continue;
            }
            CHECK(s.len < (int)s.pages.size() * P, "request %ld appends token %d beyond its %zu pages", s.id, s.len, s.pages.size());
            // (a sequence never writes into a page somebody else holds: the shared prompt pages are full)
            CHECK(page_ref[s.pages[s.len / P]] == 1, "request %ld appends into a page of %d references", s.id, page_ref[s.pages[s.len / P]]);
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
    // ftcf_batcher::step / run_admission
    void step(const bool inject)
    {
        steps++;
        const bool any = any_active();
        if (any) {
            decode();
            check_all("a decode step");
        }
        for (int si; (si = plan_resume()) >= 0;) {
            resume(si, [](int, const Swapped&, const std::vector<int>&) {});
            check_all("a resume");
        }
        const std::vector<long> before = queue_ids();
        const Request           head   = waiting.empty() ? Request{} : waiting.front();
        Admission               a      = plan_admission(any);
        if (a.kind == Kind::none) {
            CHECK(queue_ids() == before, "planning nothing changed the queue");
            refresh_host_flags();
            return;
        }
        CHECK((a.kind == Kind::fork) == head.is_fork(), "the queue's head is%s a fork request, the plan is of kind %d", head.is_fork() ? "" : " not",
              (int)a.kind);
        if (a.kind == Kind::fork) {
            CHECK(a.requests.size() == 1 && (int)a.slots.size() == head.n_samples, "a fork plan of %zu requests in %zu slots", a.requests.size(),
                  a.slots.size());
            for (const int si : a.slots) {
                CHECK(!slots[si].active, "a fork plan takes a running slot");
            }
        }
        size_t done = 0;  // requests of this plan that are in
        do {
            CHECK(swapped.empty(), "an admission while request %ld is swapped out", swapped.front().s.id);
            const Kind             kind = a.kind;
            const std::vector<int> sis  = a.slots;
            const int              n    = (kind == Kind::chunked_one) ? 1 : (int)a.requests.size();
            std::vector<long>      all, ended;
            pending.clear();
            for (std::size_t i = 0; i < a.requests.size(); i++) {
                for (const long id : ids_of(a.requests[i])) {
                    all.push_back(id);
                    if ((int)i >= n) {
                        pending.push_back(id);
                    }
                }
            }
            const long fk[4] = {fk_requests, fk_siblings, fk_shared_pages, fk_prompt_tokens};
            bool       ok    = true;
            cur              = &a;
            try {
                prompt_phase(a, n, inject);
            }
            catch (const Injected&) {
                ok = false;
            }
            cur = nullptr;
            if (!ok) {
                pending.clear();
                roll_back(a, sis, all[0], std::vector<long>(before.begin() + done, before.end()));
                for (const long id : all) {
                    gone.erase(id);  // (a request that ended with its first token is back in the queue)
                }
                if (kind == Kind::fork) {  // the one request, at the head, with every id and mask it had
                    const Request& r = waiting.front();
                    CHECK(ids_of(r) == ids_of(head) && r.n_samples == head.n_samples && r.prompt == head.prompt && r.seed == head.seed,
                          "a failed fork admission did not return its request");
                    for (std::size_t i = 0; i < r.sibs.size(); i++) {
                        CHECK(r.sibs[i].mask == head.sibs[i].mask && r.sibs[i].index == head.sibs[i].index, "a failed fork lost sibling %zu's mask", i);
                    }
                    CHECK(fk[0] == fk_requests && fk[1] == fk_siblings, "a failed fork admission was counted");
                }
                failed[(int)kind]++;
                check_all("a failed admission");
                return;  // (the exception leaves step())
            }
            for (const int si : deferred) {
                ended.push_back(slots[si].id);
            }
            if (kind == Kind::fork) {
                const Request& r = a.requests[0];
                count_fork(r, (int)a.hit.size() * P);
                CHECK(fk_requests == fk[0] + 1 && fk_siblings == fk[1] + r.n_samples
                          && fk_shared_pages == fk[2] + (long)(r.n_samples - 1) * ((long)r.prompt.size() / P)
                          && fk_prompt_tokens == fk[3] + (long)r.prompt.size() - (long)a.hit.size() * P,
                      "the fork counters");
                fork_hits += a.hit.empty() ? 0 : 1;
                const int tail = (int)r.prompt.size() % P;
                fork_tail[tail == 0 ? 0 : (tail == 1 ? 1 : 2)] += (tail <= 1 || tail == P - 1) ? 1 : 0;
            }
            if (kind != Kind::beam) {
                commit(a.slots, a.requests, n, (int)a.hit.size() * P);
            }
            gone.insert(ended.begin(), ended.end());
            admitted[(int)kind]++;
            done += n;
            pending.clear();
            for (std::size_t i = n; i < a.requests.size(); i++) {
                const std::vector<long> ids = ids_of(a.requests[i]);
                pending.insert(pending.end(), ids.begin(), ids.end());
            }
            check_all("an admission");
        } while (a.kind == Kind::chunked_one && next_chunked(a));
        pending.clear();
        check_all("the admissions of a step");
        refresh_host_flags();
    }

    // ---- the callers -------------------------------------------------------------------------------------------------------
    void submit_random()
    {
        // prompts share stems (prefix hits), token 0 is the end id; the lengths: whole pages, one token more, one less, anything
        static const int shape[7][2] = {{1, 0}, {2, 0}, {1, 1}, {2, 1}, {1, -1}, {2, -1}, {0, 1}};
        const int        pick = rnd(0, 9);
        const int        n = pick < 7 ? shape[pick][0] * P + shape[pick][1] : rnd(1, 2 * P + 2), stem = rnd(1, 2);
        const int        max_new = rnd(1, overcommit ? 4 * P - n : 2 * P);
        std::vector<int> ids(n);
        for (int i = 0; i < n; i++) {
            ids[i] = 1 + (stem * (i / 3 + 1) + i) % (VOCAB - 1);
        }
        if (rnd(0, 3) == 0) {
            ids[rnd(0, n - 1)] = rnd(1, VOCAB - 1);
        }
        const bool with_stop = rnd(0, 5) == 0;
        const int  stop_list[4] = {rnd(1, VOCAB - 1), rnd(1, VOCAB - 1), 2, -1};
        const int  kind = rnd(0, 9);  // 0: beam, 1..4: fork, else plain
        const long first = next_id;
        try {
            if (kind == 0 && max_batch >= 3) {
                submit_beam(ids.data(), n, std::min(max_new, P), 2, 0.f, 0.f, 1.f, 1.f, 0, with_stop ? stop_list : nullptr, with_stop ? 2 : 0);
            }
            else if (kind <= 4) {
                const int         ns = rnd(0, max_batch + 1);  // (0 and max_batch + 1 are refused)
                std::vector<long> out(ns + 1, -1);
                const size_t      q = waiting.size();
                try {
                    submit_n(ids.data(), n, max_new, rnd(0, 2), 0.f, 1.f, 7 + (uint64_t)first, 1.f, with_stop ? stop_list : nullptr, with_stop ? 2 : 0,
                             LogitOptions{}, ns, out.data());
                }
                catch (const ftcf::Error&) {
                    CHECK(waiting.size() == q && next_id == first, "a refused fork request queued something");
                    refused++;
                    throw;
                }
                CHECK(ns >= 1 && ns <= max_batch && waiting.size() == q + 1 && next_id == first + ns, "submit_n of %d gave %ld ids", ns, next_id - first);
                for (int i = 0; i < ns; i++) {
                    CHECK(out[i] == first + i, "sibling %d has id %ld", i, out[i]);
                    if (out[i] % 3 == 0) {  // a mask of its own while it waits (checked when it runs)
                        const unsigned m = mask_of(out[i]);
                        set_token_mask(out[i], &m, 1);
                    }
                }
                CHECK(waiting.back().is_fork() == (ns > 1), "n_samples %d queued a %s request", ns, waiting.back().is_fork() ? "fork" : "plain");
                if (ns == 1 && out[0] % 3 == 0) {
                    waiting.back().mask.clear();  // (plain requests carry no mask in this program: admit_fork's check is about siblings)
                }
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
            std::vector<long> ids;
            for (const Request& r : waiting) {
                const std::vector<long> x = ids_of(r);
                ids.insert(ids.end(), x.begin(), x.end());
            }
            const long   id = ids[rnd(0, (int)ids.size() - 1)];
            const size_t q  = waiting.size();
            size_t       sibs = 0;
            for (const Request& r : waiting) {
                const std::vector<long> x = ids_of(r);
                sibs += (r.is_fork() && std::count(x.begin(), x.end(), id)) ? r.sibs.size() : 0;
            }
            CHECK(cancel_waiting(id), "a waiting id cannot be cancelled");
            CHECK(waiting.size() == q - (sibs > 1 ? 0 : 1), "cancelling id %ld of a request of %zu siblings left %zu of %zu requests", id, sibs,
                  waiting.size(), q);
            CHECK(!cancel_waiting(id), "an id was cancelled twice");
            sib_cancelled += sibs > 0 ? 1 : 0;
            gone.insert(id);
            return;
        }
        if (what == 1 && !swapped.empty()) {
            const long id = swapped[rnd(0, (int)swapped.size() - 1)].s.id;
            CHECK(drop_swapped(id), "a swapped-out request cannot be cancelled");
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

static void run_case(const char* name, int pages, int mb, int p, bool cache, bool over, unsigned seed)
{
    Sim sim(pages, mb, p, cache, over, seed);
    try {
        for (int op = 0; op < 8000; op++) {
            const int what = sim.rnd(0, 99);
            if (what < 30) {
                sim.submit_random();
                sim.check_all("submit");
            }
            else if (what < 93) {
                sim.step(sim.rnd(0, 4) == 0);
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
        // drain: nobody submits any more; everything leaves within the bound, the pool and the swap space are whole
        long bound = (long)(sim.swapped.size() + sim.max_batch) * (sim.max_len + 2), n = 0;
        for (const auto& r : sim.waiting) {
            bound += (long)r.n_samples * (sim.max_len + 2);
        }
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
    const long *a = sim.admitted, *f = sim.failed;
    const int  fk = (int)Kind::fork;
    CHECK(a[fk] > 0 && f[fk] > 0, "%s: %ld fork admissions succeeded and %ld failed", name, a[fk], f[fk]);
    CHECK(sim.fk_requests == a[fk] && sim.fk_siblings >= a[fk], "%s: %ld fork admissions, %ld counted", name, a[fk], sim.fk_requests);
    CHECK(sim.fork_tail[0] > 0 && sim.fork_tail[1] > 0 && sim.fork_tail[2] > 0, "%s: forks with a tail of 0 / 1 / P - 1 rows: %ld / %ld / %ld", name,
          sim.fork_tail[0], sim.fork_tail[1], sim.fork_tail[2]);
    CHECK(!over || sim.pe_preemptions > 0, "%s: overcommit without a preemption", name);
    CHECK(!cache || sim.fork_hits > 0, "%s: the cache without a fork that hit", name);
    std::printf("%s: ok, %ld steps, fork admitted %ld failed %ld (tail 0 / 1 / P-1: %ld / %ld / %ld, with a hit %ld), siblings %ld, shared pages saved %ld, "
                "siblings cancelled waiting %ld, ended with the first token %ld, refused %ld, other admitted %ld failed %ld, preemptions %ld, "
                "%ld decode steps inside admissions, %ld evictions\n",
                name, sim.steps, a[fk], f[fk], sim.fork_tail[0], sim.fork_tail[1], sim.fork_tail[2], sim.fork_hits, sim.fk_siblings,
                sim.fk_shared_pages, sim.sib_cancelled, sim.sib_first_token_end, sim.refused, a[1] + a[2] + a[3] + a[4], f[1] + f[2] + f[3] + f[4],
                sim.pe_preemptions, sim.decodes_in_hook, sim.px_evictions);
}

int main()
{
    //                                             pages slots P   cache  overcommit
    run_case("12 pages 4 slots P8", 12, 4, 8, false, false, 1);
    run_case("12 pages 4 slots P8 cache", 12, 4, 8, true, false, 2);
    run_case("10 pages 4 slots P8 overcommit", 10, 4, 8, false, true, 3);
    run_case("10 pages 6 slots P16 cache overcommit", 10, 6, 16, true, true, 4);
    run_case("20 pages 8 slots P16 cache", 20, 8, 16, true, false, 5);
    run_case("14 pages 8 slots P8 overcommit", 14, 8, 8, false, true, 6);
    return 0;
}
