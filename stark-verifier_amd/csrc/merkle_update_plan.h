// The host plan of an in-place Merkle update (gl355_merkle_tree_update): which nodes a set of changed leaves dirties, and which kernel takes
// each layer.  Pure host code, no HIP: merkle.hip's launch code reads it, and tests/merkle_update_plan_check.cpp runs it under host sanitizers.
//
// A tree of n_leaves = 2^(sub_bits + cap_height) leaves is 2^cap_height cap subtrees of 2^sub_bits leaves.  Node g of layer l (1 .. sub_bits, counted
// over all subtrees, exactly the g of merkle_common.cuh's merkle_node(digests, cap, sub_bits, l, g)) is dirty when a changed leaf lies below it:
// g = leaf >> l.  Layer sub_bits holds the subtree roots, whose digests are the cap entries.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace gl355 {

constexpr uint32_t MERKLE_CLIMB_MAX = 64;      // dirty nodes per layer merkle_update_climb_kernel takes: one 16-lane group each, 1024 threads

struct MerkleUpdatePlan {
    std::vector<uint64_t> leaves;     // the changed leaf indices, sorted, each once
    std::vector<uint64_t> src;        // src[r]: the position in the caller's arrays of the LAST pair that names leaves[r] (pairs apply in order)
    std::vector<uint64_t> nodes;      // the dirty node ids of layers 1 .. sub_bits, sorted within a layer, one flat array
    std::vector<uint64_t> offset;     // layer l's ids are nodes[offset[l] .. offset[l + 1]); sub_bits + 2 entries, offset[0] = offset[1] = 0
    uint32_t sub_bits = 0;
    uint32_t climb_layer = 0;         // the first layer with at most MERKLE_CLIMB_MAX dirty nodes (the counts never grow upwards); sub_bits + 1: none
    uint64_t count(uint32_t layer) const { return offset[layer + 1] - offset[layer]; }
};

// indices[0 .. n_idx) in the caller's order, every one below n_leaves -> p.leaves, p.src.  Three ways to the same answer: indices that already
// increase are taken as they are; an update of at least 1/16 of the tree marks a table of the leaves with each one's last position and reads it
// off in order (a sort of 2^22 pairs costs several rebuilds of the whole tree on the device; the table costs its n_leaves words, which a sort of
// fewer pairs undercuts: profiles/merkle_update.txt); a smaller one sorts its (index, position) pairs.
inline void merkle_update_dedup(const uint64_t* indices, uint64_t n_idx, uint64_t n_leaves, MerkleUpdatePlan& p) {
    p.leaves.clear(); p.src.clear();
    p.leaves.reserve(n_idx); p.src.reserve(n_idx);
    bool increasing = true;
    for (uint64_t j = 1; increasing && j < n_idx; j++) increasing = indices[j - 1] < indices[j];
    if (increasing) {
        for (uint64_t j = 0; j < n_idx; j++) { p.leaves.push_back(indices[j]); p.src.push_back(j); }
        return;
    }
    if (n_idx >= (n_leaves >> 4)) {
        const uint64_t none = ~0ull;
        std::vector<uint64_t> last(n_leaves, none);
        for (uint64_t j = 0; j < n_idx; j++) last[indices[j]] = j;      // a later pair overwrites an earlier one
        for (uint64_t i = 0; i < n_leaves; i++)
            if (last[i] != none) { p.leaves.push_back(i); p.src.push_back(last[i]); }
        return;
    }
    std::vector<std::pair<uint64_t, uint64_t>> v(n_idx);
    for (uint64_t j = 0; j < n_idx; j++) v[j] = {indices[j], j};
    std::sort(v.begin(), v.end());      // by index, then by position: the last pair of a run is the last occurrence
    for (uint64_t j = 0; j < n_idx; j++)
        if (j + 1 == n_idx || v[j + 1].first != v[j].first) { p.leaves.push_back(v[j].first); p.src.push_back(v[j].second); }
}

// p.leaves (sorted, unique) of a tree of n_leaves leaves in cap subtrees of 2^sub_bits -> the dirty lists and the climb layer
inline void merkle_update_layers(uint32_t sub_bits, uint64_t n_leaves, MerkleUpdatePlan& p) {
    p.sub_bits = sub_bits;
    p.nodes.clear();
    p.offset.assign(sub_bits + 2, 0);
    p.climb_layer = sub_bits + 1;
    uint64_t n_prev = p.leaves.size(), bound = 0;
    for (uint32_t layer = 1; layer <= sub_bits; layer++) bound += std::min<uint64_t>(n_prev, n_leaves >> layer);
    p.nodes.reserve(bound);      // once: a layer is read from p.nodes while the next is appended, and growing by layers copies the list over and over
    for (uint32_t layer = 1; layer <= sub_bits; layer++) {
        const uint64_t first = p.nodes.size();
        const uint64_t* prev = layer == 1 ? p.leaves.data() : p.nodes.data() + p.offset[layer - 1];
        for (uint64_t j = 0; j < n_prev; j++) {
            const uint64_t g = prev[j] >> 1;
            if (p.nodes.size() == first || p.nodes.back() != g) p.nodes.push_back(g);
        }
        p.offset[layer] = first;
        p.offset[layer + 1] = p.nodes.size();
        n_prev = p.nodes.size() - first;
        if (p.climb_layer > sub_bits && n_prev <= MERKLE_CLIMB_MAX) p.climb_layer = layer;
    }
}

// An update of at least n_leaves >> full_log leaves rebuilds every level (GL355_OPT_MERKLE_UPDATE_FULL_LOG): no dirty lists are planned.
inline bool merkle_update_is_full(uint64_t n_unique, uint64_t n_leaves, uint32_t full_log) { return n_unique >= (n_leaves >> std::min<uint32_t>(full_log, 63)); }

// the kernel that takes a layer of the dirty path
enum MerkleUpdateKernel { MERKLE_UPDATE_LEVEL = 0, MERKLE_UPDATE_LANES = 1, MERKLE_UPDATE_CLIMB = 2 };
// lanes16: the hasher has the 16-lane forms (Poseidon); without them every layer takes the one-lane kernel.  The climb takes its layer and all above it.
inline MerkleUpdateKernel merkle_update_kernel_of(const MerkleUpdatePlan& p, uint32_t layer, uint32_t lanes_log, bool lanes16) {
    if (!lanes16) return MERKLE_UPDATE_LEVEL;
    if (layer >= p.climb_layer) return MERKLE_UPDATE_CLIMB;
    return p.count(layer) <= (1ull << lanes_log) ? MERKLE_UPDATE_LANES : MERKLE_UPDATE_LEVEL;
}

// every launch's grid fits 32 bits (as fri_wide_leaves_tree_dev checks its own): 256 leaves or nodes per block, or 4 nodes per block
inline bool merkle_update_grids_fit(const MerkleUpdatePlan& p) {
    uint64_t widest = p.leaves.size();
    for (uint32_t layer = 1; layer <= p.sub_bits; layer++) widest = std::max(widest, p.count(layer));
    return (widest + 3) / 4 <= 0x7FFFFFFFull;
}

}  // namespace gl355
