// Host check of the batcher's prefix index (fastertransformer4codefuse_amd/csrc/prefix_index.h; tests/test_prefix_index_host.py).
// Replays random admit / finish / evict / clear sequences the way batcher.hip drives the index, over a small token alphabet
// (many shared prefixes and colliding blocks), and checks after every operation:
//   * page_ref[pg] == running requests holding pg + index nodes owning pg; the free list is exactly the unreferenced pages;
//   * eviction only ever takes a live leaf whose page has no other reference, the least recently used of them;
//   * evictable() == what repeated eviction frees;
//   * no two nodes own a page, no parent has two children for one block, every cached page holds the K/V of its own path;
//   * a lookup never serves a page whose K/V belong to other tokens (the model's "K/V" of a page is the prefix it was
//     computed after).
// Prints one "<case>: ok, ..." line per configuration; exits non-zero on the first violation.
#include "prefix_index.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using ftcf::PrefixIndex;

#define CHECK(c, ...)                                                                                                                 \
    do {                                                                                                                              \
        if (!(c)) {                                                                                                                   \
            std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #c);                                                                  \
            std::printf(__VA_ARGS__);                                                                                                 \
            std::printf("\n");                                                                                                        \
            std::exit(1);                                                                                                             \
        }                                                                                                                             \
    } while (0)

struct Sim {
    int                            P, num_pages;
    PrefixIndex                    idx;
    std::vector<int>               ref, free_list;
    std::vector<std::vector<int>>  content;  // content[pg]: the token prefix whose last block's K/V the page holds
    std::vector<std::vector<int>>  running;  // page lists of running requests
    long                           evictions = 0, hits = 0, lookups = 0;

    Sim(int p, int n) : P(p), num_pages(n), idx(p), ref(n, 0), content(n)
    {
        for (int i = n - 1; i >= 0; i--) {
            free_list.push_back(i);
        }
    }
    // live leaves whose page only the index references, with their last use
    std::vector<std::pair<int, uint64_t>> eligible() const
    {
        std::vector<std::pair<int, uint64_t>> s;
        for (const auto& n : idx.nodes) {
            if (n.live && n.page >= 0 && n.children.empty() && ref[n.page] == 1) {
                s.emplace_back(n.page, n.last_use);
            }
        }
        return s;
    }
    int evict()
    {
        const auto ok = eligible();
        const int  pg = idx.evict_one(ref);
        if (pg < 0) {
            CHECK(ok.empty(), "evict_one found nothing among %zu candidates", ok.size());
            return -1;
        }
        uint64_t lru = ~0ull, mine = ~0ull;
        for (const auto& x : ok) {
            lru = std::min(lru, x.second);
            mine = x.first == pg ? x.second : mine;
        }
        CHECK(mine != ~0ull, "evicted page %d is not an unreferenced leaf", pg);
        CHECK(mine == lru, "a more recently used leaf was evicted before an older one");
        if (--ref[pg] == 0) {
            free_list.push_back(pg);
        }
        return pg;
    }
    int take()
    {
        if (free_list.empty()) {
            if (evict() >= 0) {
                evictions++;
            }
        }
        CHECK(!free_list.empty(), "pool exhausted although the budget admitted the request");
        int pg = free_list.back();
        free_list.pop_back();
        CHECK(ref[pg] == 0, "free page %d has references", pg);
        ref[pg] = 1;
        return pg;
    }
    // what the batcher does for one ordinary request: lookup, budget, pin, allocate, "compute", insert
    bool admit(const std::vector<int>& prompt, int max_new)
    {
        const int S = (int)prompt.size();
        std::vector<int> hit = idx.lookup(prompt.data(), (S - 1) / P);
        CHECK((int)hit.size() <= (S - 1) / P, "lookup returned too many blocks");
        for (size_t b = 0; b < hit.size(); b++) {  // nothing but the prompt's own K/V may be served
            std::vector<int> want(prompt.begin(), prompt.begin() + (b + 1) * P);
            CHECK(content[hit[b]] == want, "block %zu served a page computed for other tokens", b);
        }
        for (int pg : hit) {
            ref[pg]++;
        }
        const int need  = (S + max_new + P - 1) / P - (int)hit.size();
        const int avail = (int)free_list.size() + idx.evictable(ref);
        if (avail < need) {
            for (int pg : hit) {
                ref[pg]--;
            }
            return false;
        }
        lookups++;
        hits += hit.empty() ? 0 : 1;
        idx.touch(prompt.data(), (int)hit.size());
        std::vector<int> pages = hit;
        while ((int)pages.size() < (S + max_new + P - 1) / P) {
            pages.push_back(take());
        }
        for (int b = (int)hit.size(); b < S / P; b++) {  // the tail's full blocks: computed after their own prefix
            content[pages[b]].assign(prompt.begin(), prompt.begin() + (b + 1) * P);
        }
        for (int b = S / P; b < (int)pages.size(); b++) {
            content[pages[b]].assign(1, -1);  // a page decode writes into: never a full prompt block
        }
        idx.insert(prompt.data(), S / P, pages, ref);
        running.push_back(pages);
        return true;
    }
    void finish(size_t i)
    {
        for (int pg : running[i]) {
            CHECK(ref[pg] > 0, "double release of page %d", pg);
            if (--ref[pg] == 0) {
                free_list.push_back(pg);
            }
        }
        running.erase(running.begin() + i);
    }
    void clear()
    {
        for (int pg; (pg = idx.evict_one(ref)) >= 0;) {
            if (--ref[pg] == 0) {
                free_list.push_back(pg);
            }
        }
    }
    void path(int nd, std::vector<int>& toks) const
    {
        if (nd == 0) {
            return;
        }
        path(idx.nodes[nd].parent, toks);
        const auto& ch = idx.nodes[idx.nodes[nd].parent].children;
        for (const auto& kv : ch) {
            if (kv.second == nd) {
                toks.insert(toks.end(), kv.first.begin(), kv.first.end());
            }
        }
    }
    void invariants()
    {
        std::vector<int> holders(num_pages, 0);
        for (const auto& r : running) {
            for (int pg : r) {
                holders[pg]++;
            }
        }
        std::vector<int> owners(num_pages, 0);
        int              live = 0;
        for (int i = 1; i < (int)idx.nodes.size(); i++) {
            const auto& n = idx.nodes[i];
            if (!n.live) {
                continue;
            }
            live++;
            owners[n.page]++;
            CHECK(idx.nodes[n.parent].live, "node %d hangs off a dead parent", i);
            int found = 0;
            for (const auto& kv : idx.nodes[n.parent].children) {
                found += kv.second == i;
                CHECK((int)kv.first.size() == P, "an edge is not one block");
            }
            CHECK(found == 1, "node %d is its parent's child %d times", i, found);
            std::vector<int> toks;
            path(i, toks);
            CHECK(content[n.page] == toks, "node %d's page holds the K/V of other tokens", i);
        }
        CHECK(live == idx.n_cached, "n_cached %d != live nodes %d", idx.n_cached, live);
        std::set<int> fl(free_list.begin(), free_list.end());
        CHECK(fl.size() == free_list.size(), "a page is on the free list twice");
        for (int pg = 0; pg < num_pages; pg++) {
            CHECK(owners[pg] <= 1, "page %d is owned by %d nodes", pg, owners[pg]);
            CHECK(ref[pg] == holders[pg] + owners[pg], "page %d: ref %d, holders %d + index %d", pg, ref[pg], holders[pg], owners[pg]);
            CHECK((ref[pg] == 0) == (fl.count(pg) == 1), "page %d: ref %d but free-list membership %d", pg, ref[pg], (int)fl.count(pg));
        }
        // evictable() == what repeated eviction frees
        PrefixIndex      copy = idx;
        std::vector<int> r2   = ref;
        int              n    = 0;
        for (int pg; (pg = copy.evict_one(r2)) >= 0;) {
            r2[pg]--;
            n++;
        }
        CHECK(n == idx.evictable(ref), "evictable() %d, eviction frees %d", idx.evictable(ref), n);
    }
};

int main()
{
    struct Case {
        int P, pages, alphabet, base_len, ops;
        unsigned seed;
    };
    const Case cases[] = {{2, 12, 2, 9, 4000, 1}, {3, 20, 3, 14, 4000, 2}, {4, 16, 2, 17, 4000, 3}, {8, 40, 4, 40, 3000, 4},
                          {2, 64, 2, 24, 6000, 5}, {4, 9, 3, 12, 4000, 6}, {8, 24, 2, 33, 3000, 7}, {16, 30, 5, 70, 2000, 8}};
    for (const Case& c : cases) {
        std::mt19937     rng(c.seed);
        Sim              sim(c.P, c.pages);
        std::vector<std::vector<int>> bases(4);
        for (auto& b : bases) {
            for (int i = 0; i < c.base_len; i++) {
                b.push_back((int)(rng() % c.alphabet));
            }
        }
        long admitted = 0, refused = 0, cleared = 0;
        for (int op = 0; op < c.ops; op++) {
            const int kind = (int)(rng() % 10);
            if (kind < 5) {  // a request: a base prompt, cut and with a private tail of random length
                std::vector<int> p = bases[rng() % bases.size()];
                p.resize(1 + rng() % p.size());
                const int tail = (int)(rng() % (2 * c.P + 1));
                for (int i = 0; i < tail; i++) {
                    p.push_back((int)(rng() % c.alphabet));
                }
                const int max_new = 1 + (int)(rng() % (c.P + 2));
                if ((int)((p.size() + max_new + c.P - 1) / c.P) > c.pages) {
                    continue;
                }
                if (sim.admit(p, max_new)) {
                    admitted++;
                }
                else {
                    refused++;
                    if (!sim.running.empty()) {  // nothing waits forever: running requests finish and free their pages
                        sim.finish(rng() % sim.running.size());
                    }
                }
            }
            else if (kind < 9) {
                if (!sim.running.empty()) {
                    sim.finish(rng() % sim.running.size());
                }
            }
            else if (rng() % 8 == 0) {
                sim.clear();
                cleared++;
            }
            else {
                sim.evict();
            }
            sim.invariants();
        }
        while (!sim.running.empty()) {
            sim.finish(0);
        }
        sim.invariants();
        sim.clear();
        sim.invariants();
        CHECK((int)sim.free_list.size() == c.pages && sim.idx.n_cached == 0, "pages lost after the final clear");
        std::printf("P %d pages %d alphabet %d: ok, %ld admitted (%ld with a hit), %ld refused, %ld evictions, %ld clears\n", c.P, c.pages,
                    c.alphabet, admitted, sim.hits, refused, sim.evictions, cleared);
    }
    return 0;
}
