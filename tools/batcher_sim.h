// What the host checks of the continuous batcher's scheduler share (check_batcher_sched.cc, check_batcher_preempt.cc): a
// BatcherSched driven the way batcher.hip drives it, with a FAKE prompt phase that succeeds or throws at a seeded point and the
// beam half of a fake decode step.  A program derives its Sim from BatcherSim and adds what is its own: its invariants, its
// fake device halves (admit, decode), its request mix.  Every draw comes from the one seeded generator, in the order of the calls.
#pragma once
#include "batcher_sched.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using ftcf::BatcherSched;
typedef BatcherSched::Kind Kind;

#define CHECK(c, ...)                                                                                                                 \
    do {                                                                                                                              \
        if (!(c)) {                                                                                                                   \
            std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c);                                                                  \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

struct Injected {};  // the fake prompt phase's failure

struct BatcherSim : BatcherSched {
    static constexpr int END_ID = 0;
    std::mt19937 rng;
    const int    fin_one_in;       // a beam finishes in a step with probability 1 / fin_one_in
    int          fail_in = -1;     // the fake prompt phase throws at its fail_in-th point (-1: never)
    bool         hook_on = false;  // decode steps run between the chunks of the prompt phase
    long         decodes_in_hook = 0;

    BatcherSim(unsigned seed, int fin_rate): rng(seed), fin_one_in(fin_rate) {}
    virtual ~BatcherSim() = default;

    // ---- the program's own ---------------------------------------------------------------------------------------------------
    // ftcf_batcher::admit: pages of every slot, the prompt phase (chunks, decode steps between them), first tokens
    virtual void admit(const std::vector<int>& sis, const std::vector<Request>& rs, int n, const std::vector<int>* hit) = 0;
    // ftcf_batcher::decode + advance_groups, host side (its beam half: decode_groups)
    virtual void decode() = 0;
    virtual void group_finished(long) {}

    int rnd(int lo, int hi)  // [lo, hi]
    {
        return std::uniform_int_distribution<int>(lo, hi)(rng);
    }
    void point()
    {
        if (fail_in >= 0 && fail_in-- == 0) {
            throw Injected{};
        }
    }
    std::vector<long> queue_ids() const
    {
        std::vector<long> ids;
        for (const Request& r : waiting) {
            ids.push_back(r.id);
        }
        return ids;
    }

    // ---- the fake device side ------------------------------------------------------------------------------------------------
    void hook()  // run_admission's chunk hook
    {
        if (hook_on && any_active()) {
            refresh_host_flags();
            decode();
            decodes_in_hook++;
        }
    }
    void finish_or_append(BeamGroup& g, const std::vector<uint8_t>& fin)
    {
        bool all_fin = true;
        for (int k = 0; k < g.K; k++) {
            all_fin &= fin[k] != 0;
        }
        if (all_fin || g.generated >= g.max_new) {
            group_finished(g.id);
            drop_group(g.si);  // finish_group
        }
        else {
            take_append_pages(g, g.n + g.generated - 1, fin);  // prepare_append
        }
    }
    std::vector<uint8_t> random_fin(int K, int one_in)
    {
        std::vector<uint8_t> fin(K);
        for (auto& f : fin) {
            f = rnd(0, one_in - 1) == 0;
        }
        return fin;
    }
    // ftcf_batcher::admit_beam: the prompt phase first, then the group and its shared pages, the beams' own pages
    void admit_beam(const int si, const Request& r)
    {
        point();
        hook();
        point();
        BeamGroup& g = open_group(si, r);
        point();
        start_group_slots(g);
        finish_or_append(g, random_fin(g.K, fin_one_in));
        point();
    }
    // the beam half of a decode step: every beam takes over a random parent's pages, finished groups leave
    void decode_groups()
    {
        std::vector<int> leaders;
        for (const auto& kv : groups) {
            leaders.push_back(kv.first);
        }
        for (const int si : leaders) {
            BeamGroup&       g = groups.at(si);
            std::vector<int> parent(g.K);
            for (int& p : parent) {
                p = rnd(0, g.K - 1);
            }
            reparent_group(g, parent);
            for (int k = 0; k < g.K; k++) {
                slots[si + k].len += 1;
            }
            finish_or_append(g, random_fin(g.K, fin_one_in));
        }
    }
    // ONE admission of a plan as run_admission tries it: the fake prompt phase of its kind, throwing at a seeded point when
    // `inject` says so (or what a decode step between the chunks throws)
    void prompt_phase(Admission& a, const int n, const bool inject)
    {
        struct Off {
            BatcherSim& s;
            ~Off()
            {
                s.hook_on = false;
                s.fail_in = -1;
            }
        } off{*this};
        fail_in = inject ? rnd(0, 5) : -1;
        hook_on = a.install_hook;
        if (a.kind == Kind::beam) {
            admit_beam(a.slots[0], a.requests[0]);
        }
        else {
            admit(a.slots, a.requests, n, a.kind == Kind::hit ? &a.hit : nullptr);
        }
    }
    // ... and its rollback with what must hold afterwards: none of its slots (`sis`) is active, no group of its first request's
    // id exists, the queue is `queue` again
    void roll_back(Admission& a, const std::vector<int>& sis, const long id, const std::vector<long>& queue)
    {
        rollback(
            a, [this](int si) { release(slots[si]); }, [this](int si) { drop_group(si); });
        for (const int si : sis) {
            CHECK(!slots[si].active, "slot %d of a failed admission is active", si);
        }
        for (const auto& kv : groups) {
            CHECK(kv.second.id != id, "the group of a failed beam admission exists");
        }
        CHECK(queue_ids() == queue, "a failed admission reordered the queue");
    }

    // ---- the invariants both programs hold: page accounting, well-formed groups ------------------------------------------------
    void check_pages(const char* after)
    {
        std::vector<int> holders(num_pages, 0);
        std::set<int>    by_requests;
        for (const Slot& s : slots) {
            CHECK(s.active || s.pages.empty(), "after %s: a free slot holds pages", after);
            for (int pg : s.pages) {
                holders[pg]++;
                by_requests.insert(pg);
            }
        }
        for (const auto& kv : groups) {
            const BeamGroup& g = kv.second;
            CHECK(kv.first == g.si && (int)g.lists.size() == g.K, "after %s: a malformed group", after);
            for (int k = 0; k < g.K; k++) {
                const Slot& s = slots[g.si + k];
                CHECK(s.active && s.group == g.si && s.id == g.id, "after %s: group %d's slot %d is not its own", after, g.si, g.si + k);
                for (int pg : g.lists[k]) {
                    holders[pg]++;
                    by_requests.insert(pg);
                }
            }
        }
        for (int si = 0; si < max_batch; si++) {
            const Slot& s = slots[si];
            if (s.active && s.group >= 0) {
                auto it = groups.find(s.group);
                CHECK(it != groups.end() && si >= it->second.si && si < it->second.si + it->second.K,
                      "after %s: slot %d is a beam of a group that does not exist", after, si);
            }
        }
        for (const auto& n : pindex.nodes) {
            if (n.live && n.page >= 0) {
                holders[n.page]++;
            }
        }
        std::vector<int> in_free(num_pages, 0);
        for (int pg : free_pages) {
            CHECK(pg >= 0 && pg < num_pages && ++in_free[pg] == 1, "after %s: page %d is twice in the free list", after, pg);
        }
        for (int pg = 0; pg < num_pages; pg++) {
            CHECK(page_ref[pg] == holders[pg], "after %s: page %d has %d references and %d holders", after, pg, page_ref[pg], holders[pg]);
            CHECK(in_free[pg] == (holders[pg] == 0 ? 1 : 0), "after %s: page %d, %d holders, free list %d", after, pg, holders[pg], in_free[pg]);
        }
        CHECK(reserved_pages() + (int)by_requests.size() <= num_pages, "after %s: %d pages promised and %zu held of %d", after,
              reserved_pages(), by_requests.size(), num_pages);
    }
};
