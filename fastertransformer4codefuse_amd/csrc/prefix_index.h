// Prefix index of the continuous batcher (batcher.hip): which pool pages hold the K/V of finished prompt blocks.
// Plain C++ (no HIP): tools/check_prefix_index.cc replays random operation sequences against it on the host.
//
// A trie whose edges are blocks of P tokens.  Node i (i > 0; node 0 is the root and holds nothing) stands for the prompt prefix
// spelled by the path to it and owns ONE pool page: the K/V of its block, computed after exactly that prefix.  Children are
// keyed by the block's actual tokens (std::map over the token vector), so two different prefixes can never share a node, hash
// collisions or not.  The index holds one reference to every page it owns in the caller's `ref` array (page_ref of the
// batcher); a request that uses a cached page holds one more.  Cached pages are immutable: a request only takes full prompt
// blocks from the index, and decode appends behind them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace ftcf {

struct PrefixIndex {
    struct Node {
        int                              parent = -1, page = -1;
        uint64_t                         last_use = 0;
        bool                             live = false;
        std::map<std::vector<int>, int>  children;  // block tokens -> node
    };
    int               P = 0;
    std::vector<Node> nodes;
    std::vector<int>  spare;  // indices of dead nodes, reused
    uint64_t          tick = 0;
    int               n_cached = 0;

    explicit PrefixIndex(int page_tokens = 0) : P(page_tokens)
    {
        nodes.emplace_back();
        nodes[0].live = true;
    }

    // the longest chain of cached full blocks that starts the prompt, at most max_blocks long: the pages, in order
    std::vector<int> lookup(const int* ids, int max_blocks) const
    {
        std::vector<int> pages;
        int              cur = 0;
        for (int b = 0; b < max_blocks; b++) {
            const std::vector<int> key(ids + (std::size_t)b * P, ids + (std::size_t)(b + 1) * P);
            auto                   it = nodes[cur].children.find(key);
            if (it == nodes[cur].children.end()) {
                break;
            }
            cur = it->second;
            pages.push_back(nodes[cur].page);
        }
        return pages;
    }
    // marks the first n blocks' nodes as used now (the chain a request has just taken)
    void touch(const int* ids, int n)
    {
        tick++;
        int cur = 0;
        for (int b = 0; b < n; b++) {
            auto it = nodes[cur].children.find(std::vector<int>(ids + (std::size_t)b * P, ids + (std::size_t)(b + 1) * P));
            if (it == nodes[cur].children.end()) {
                return;
            }
            cur                = it->second;
            nodes[cur].last_use = tick;
        }
    }
    // the first n_blocks full blocks of a prompt whose K/V are in `pages` (pages[b] holds block b).  Blocks already in the index
    // keep their node (first writer wins: the request keeps its private page for them); every new node takes one reference to
    // its page.  Returns how many nodes were added.
    int insert(const int* ids, int n_blocks, const std::vector<int>& pages, std::vector<int>& ref)
    {
        tick++;
        int cur = 0, added = 0;
        for (int b = 0; b < n_blocks; b++) {
            std::vector<int> key(ids + (std::size_t)b * P, ids + (std::size_t)(b + 1) * P);
            auto             it = nodes[cur].children.find(key);
            if (it != nodes[cur].children.end()) {
                cur                 = it->second;
                nodes[cur].last_use = tick;
                continue;
            }
            int nd;
            if (!spare.empty()) {
                nd = spare.back();
                spare.pop_back();
            }
            else {
                nd = (int)nodes.size();
                nodes.emplace_back();
            }
            Node& n    = nodes[nd];
            n.parent   = cur;
            n.page     = pages[b];
            n.last_use = tick;
            n.live     = true;
            n.children.clear();
            ref[n.page]++;
            nodes[cur].children.emplace(std::move(key), nd);
            cur = nd;
            added++;
            n_cached++;
        }
        return added;
    }
    // pages that eviction could free now: nodes whose page only the index references and whose whole subtree is the same
    // (a leaf goes first, then possibly its parent)
    int evictable(const std::vector<int>& ref) const
    {
        int n = 0;
        count_free(0, ref, n);
        return n;
    }
    // the least recently used leaf whose page only the index references leaves the index; returns its page (the caller
    // drops the index's reference) or -1 when there is none
    int evict_one(const std::vector<int>& ref)
    {
        int best = -1;
        for (int i = 1; i < (int)nodes.size(); i++) {
            const Node& n = nodes[i];
            if (n.live && n.children.empty() && ref[n.page] == 1 && (best < 0 || n.last_use < nodes[best].last_use)) {
                best = i;
            }
        }
        if (best < 0) {
            return -1;
        }
        Node& n = nodes[best];
        auto& siblings = nodes[n.parent].children;
        for (auto it = siblings.begin(); it != siblings.end(); ++it) {
            if (it->second == best) {
                siblings.erase(it);
                break;
            }
        }
        const int page = n.page;
        n.live   = false;
        n.parent = -1;
        n.page   = -1;
        spare.push_back(best);
        n_cached--;
        return page;
    }

private:
    bool count_free(int i, const std::vector<int>& ref, int& n) const
    {
        bool all = true;
        for (const auto& kv : nodes[i].children) {
            all &= count_free(kv.second, ref, n);
        }
        if (i == 0) {
            return all;
        }
        if (all && ref[nodes[i].page] == 1) {
            n++;
            return true;
        }
        return false;
    }
};

}  // namespace ftcf
