// What the two hash back-ends share (merkle.hip: Poseidon-Goldilocks, merkle_bn254.hip: the reference's Bn254PoseidonHash): plonky2's
// digest layout, the launch arguments, and the bodies of the one-lane-per-state kernels as templates over a hasher policy.  A policy H
// is a struct of statics, defined next to its permutation:
//   permute(s)       the permutation of a 12-word sponge state
//   out(x)           a word leaving the state: gl_canon for Goldilocks (its permutation returns any representative), nothing for BN254
//   in2(x)           a digest word entering two_to_one: BN254 reduces it (its packing needs canonical words), Goldilocks takes any u64
//   wide_digests     digests move as 16-byte accesses in the leaf and level kernels (Goldilocks); BN254 keeps the 8-byte ones it was
//                    written and measured with
// Every __global__ entry point stays a named function in its own file and instantiates a body: tools, tests and profile records find
// kernels by name, and each keeps its own launch bounds.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/gl355.h"
#include "gl_field.cuh"

namespace gl355 {

// index of node k of layer `layer` (0 = leaf digests) inside one cap-subtree's digest buffer:
// pair p = k>>1 of layer i sits at pair slot (p << (i+1)) + 2^i - 1 (MerkleTree::prove's formula).
__host__ __device__ __forceinline__ uint64_t digest_slot(uint32_t layer, uint64_t k) {
    return 2 * (((k >> 1) << (layer + 1)) + (1ull << layer) - 1) + (k & 1);
}

// where the digest of leaf i (over all cap subtrees) goes: slot i of a plain array (linear), cap entry i when the tree is all cap
// (sub_bits == 0), else digest_slot(0, k) of subtree t
__device__ __forceinline__ uint64_t* leaf_digest_dst(uint64_t* out, uint64_t* cap, uint32_t linear, uint32_t sub_bits, uint64_t i) {
    if (linear) return out + i * 4;
    if (sub_bits == 0) return cap + i * 4;
    const uint64_t sub_leaves = 1ull << sub_bits;
    const uint64_t t = i >> sub_bits, k = i & (sub_leaves - 1);
    return out + (t * 2 * (sub_leaves - 1) + digest_slot(0, k)) * 4;
}

// Node k of layer `layer` (>= 1) of cap subtree t: the subtree's digests, the slot of its left child in them (the right child is the next
// slot) and where its own digest goes (the cap entry when the node is the subtree's root).  child() and dst() are worked out where they
// are called: a kernel asks for dst() after its permutation, so the address is not carried through it in registers.
struct MerkleNode {
    uint64_t* tree; uint64_t* cap; uint32_t sub_bits, layer; uint64_t t, k;
    __device__ __forceinline__ uint64_t child() const { return digest_slot(layer - 1, 2 * k); }
    __device__ __forceinline__ uint64_t* dst() const { return (layer == sub_bits) ? cap + t * 4 : tree + digest_slot(layer, k) * 4; }
};
__device__ __forceinline__ MerkleNode merkle_node(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, uint64_t t, uint64_t k) {
    const uint64_t sub_leaves = 1ull << sub_bits;
    return {digests + t * 2 * (sub_leaves - 1) * 4, cap, sub_bits, layer, t, k};
}
// the same for node g of the layer counted over all subtrees
__device__ __forceinline__ MerkleNode merkle_node(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, uint64_t g) {
    const uint64_t per = (1ull << sub_bits) >> layer;
    return merkle_node(digests, cap, sub_bits, layer, g / per, g % per);
}

struct LeafArgs {
    const uint64_t* leaves;
    uint64_t n_leaves;      // all units together
    uint32_t leaf_len;
    uint32_t col_major;
    uint64_t stride;        // col-major: elements between columns; row-major: elements between rows
    uint64_t* out;          // digest destination
    uint32_t sub_bits;      // log2(leaves per cap subtree); layout = subtree t at out + t*sub_dig*4
    uint32_t linear;        // 1: out[i*4..] (no layout)
    uint32_t always_hash;   // hash_no_pad semantics (no <=4 shortcut)
    uint64_t* cap;          // used when sub_bits == 0 (tree is all cap)
    // several units (independent trees of 2^unit_log leaves each, the lock-step proofs of one prover context) in one launch:
    // leaf g belongs to unit g >> unit_log; its columns [0, n_main) come from `leaves + unit * unit_stride`, the remaining ones
    // (the salt columns of a blinded oracle) from `salt + unit * salt_unit_stride`.  unit_log == 0 means one unit, no salt segment.
    uint32_t unit_log;
    uint32_t n_main;
    uint64_t unit_stride;
    const uint64_t* salt;
    uint64_t salt_unit_stride;
};

// element k of leaf g
__device__ __forceinline__ uint64_t leaf_elem(const LeafArgs& a, uint64_t g, uint32_t k) {
    if (a.unit_log == 0) return a.col_major ? a.leaves[(uint64_t)k * a.stride + g] : a.leaves[g * a.stride + k];
    const uint64_t u = g >> a.unit_log, i = g & ((1ull << a.unit_log) - 1);
    if (k < a.n_main) {
        const uint64_t* base = a.leaves + u * a.unit_stride;
        return a.col_major ? base[(uint64_t)k * a.stride + i] : base[i * a.stride + k];
    }
    return a.salt[u * a.salt_unit_stride + (uint64_t)(k - a.n_main) * a.stride + i];     // salt columns are always column-major
}

// An in-place update of a resident tree (gl355_merkle_tree_update): leaf idx[r] takes the leaf_len words of row src[r] of the caller's new leaves
// (`rows`, uploaded as they came).  The host has sorted the indices and removed duplicates, keeping each one's last row (merkle_update_plan.h), so no
// two lanes write one slot.
struct UpdateLeafArgs {
    const uint64_t* idx; const uint64_t* src; const uint64_t* rows; uint64_t n_idx, n_rows;
    uint64_t* leaves;       // the resident row-major leaf array
    uint32_t leaf_len, sub_bits;
    uint64_t* digests; uint64_t* cap;
};

// what merkle_update_climb_kernel walks: the dirty counts (1 .. 64) of its layers, whose node ids follow one another in its list
struct ClimbCounts { uint8_t n[64]; };

// proof of work of every unit that still lacks a witness: candidates start + g, the smallest passing one of the launch wins
struct PowArgs { uint64_t state[GL355_MAX_UNITS * 12]; uint32_t pos[GL355_MAX_UNITS]; uint32_t todo[GL355_MAX_UNITS]; uint32_t bits; uint64_t start; unsigned long long* best; };

#if defined(__HIPCC__)
// the 16 or 32 lanes sharing a state sit in ONE wave, and a wave's LDS instructions complete in issue order: the exchange through LDS
// only needs the compiler (and the LGKM counter) to keep write -> read -> next write ordered, not s_barrier
#define GL_WAVE_LDS_SYNC()                                      \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
    } while (0)

template <class H> GL_DEV void store_digest(uint64_t* dst, const uint64_t (&d)[4]) {
    if constexpr (H::wide_digests) {
        *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(d[0], d[1]);
        *reinterpret_cast<ulonglong2*>(dst + 2) = make_ulonglong2(d[2], d[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = d[k];
    }
}

template <class H> GL_DEV void permute_body(uint64_t* states, uint64_t count) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = states[i * 12 + k];
    H::permute(s);
#pragma unroll
    for (int k = 0; k < 12; k++) states[i * 12 + k] = H::out(s[k]);
}

// one lane = one leaf: overwrite-mode sponge over ceil(len/8) chunks.  Leaf i of `a` is hashed, its digest goes where leaf `dst` of the tree belongs
// (the same leaf when a tree is built, another one when an update's new rows are hashed)
template <class H> GL_DEV void hash_leaf(const LeafArgs& a, uint64_t i, uint64_t dst) {
    uint64_t s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = 0;
    const uint32_t len = a.leaf_len;
    uint64_t d[4];
    if (len <= 4 && !a.always_hash) {
        for (uint32_t k = 0; k < 4; k++) {
            uint64_t v = 0;
            if (k < len) v = leaf_elem(a, i, k);
            d[k] = gl_canon(v);
        }
    } else {
        // kept rolled: one inlined copy of the permutation (it changes nothing for Goldilocks, whose loop the compiler leaves rolled anyway)
#pragma unroll 1
        for (uint32_t off = 0; off < len; off += 8) {
            const uint32_t m = min(8u, len - off);
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                if (k < m) s[k] = leaf_elem(a, i, off + k);
            }
            H::permute(s);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = H::out(s[k]);
    }
    store_digest<H>(leaf_digest_dst(a.out, a.cap, a.linear, a.sub_bits, dst), d);
}

template <class H> GL_DEV void hash_leaves_body(const LeafArgs& a) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= a.n_leaves) return;
    hash_leaf<H>(a, i, i);
}

// one lane = one updated leaf: its words into the resident leaf array, its digest where hash_leaves_body puts it
template <class H> GL_DEV void update_leaves_body(const UpdateLeafArgs& u) {
    const uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (r >= u.n_idx) return;
    const uint64_t i = u.idx[r], from = u.src[r];
    for (uint32_t k = 0; k < u.leaf_len; k++) u.leaves[i * u.leaf_len + k] = u.rows[from * u.leaf_len + k];
    LeafArgs a;      // the new rows as a row-major leaf array of one unit
    a.leaves = u.rows; a.n_leaves = u.n_rows; a.leaf_len = u.leaf_len; a.col_major = 0; a.stride = u.leaf_len;
    a.out = u.digests; a.sub_bits = u.sub_bits; a.linear = 0; a.always_hash = 0; a.cap = u.cap;
    a.unit_log = 0; a.n_main = 0; a.unit_stride = 0; a.salt = nullptr; a.salt_unit_stride = 0;
    hash_leaf<H>(a, from, i);
}

// node g of layer `layer` (>= 1), counted over all subtrees: two_to_one of its children in layer - 1, by one lane
template <class H> GL_DEV void merkle_node_hash(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, uint64_t g) {
    const MerkleNode nd = merkle_node(digests, cap, sub_bits, layer, g);
    const uint64_t* in = nd.tree + nd.child() * 4;      // left child; right child is +1
    uint64_t s[12];
    if constexpr (H::wide_digests) {
        const ulonglong2 l0 = *reinterpret_cast<const ulonglong2*>(in);
        const ulonglong2 l1 = *reinterpret_cast<const ulonglong2*>(in + 2);
        const ulonglong2 r0 = *reinterpret_cast<const ulonglong2*>(in + 4);
        const ulonglong2 r1 = *reinterpret_cast<const ulonglong2*>(in + 6);
        s[0] = l0.x; s[1] = l0.y; s[2] = l1.x; s[3] = l1.y; s[4] = r0.x; s[5] = r0.y; s[6] = r1.x; s[7] = r1.y;
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) s[e] = in[e];
    }
#pragma unroll
    for (int e = 8; e < 12; e++) s[e] = 0;
    H::permute(s);
    const uint64_t d[4] = {H::out(s[0]), H::out(s[1]), H::out(s[2]), H::out(s[3])};
    store_digest<H>(nd.dst(), d);
}

// one lane = one parent node of layer `layer`
template <class H> GL_DEV void merkle_level_body(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, uint64_t n_nodes /* all subtrees */) {
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (g >= n_nodes) return;
    merkle_node_hash<H>(digests, cap, sub_bits, layer, g);
}

// the same for the dirty nodes of an update: lane e takes node list[e]
template <class H> GL_DEV void merkle_update_level_body(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, const uint64_t* list, uint64_t n_list) {
    const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (e >= n_list) return;
    merkle_node_hash<H>(digests, cap, sub_bits, layer, list[e]);
}

// one thread per (index q, layer i): the sibling MerkleTree::prove reads on the way from leaf idx[q] to its cap entry, 32 bytes into out [n_idx][layers][4]
__device__ __forceinline__ void merkle_paths_body(const uint64_t* digests, uint32_t layers, const uint64_t* idx, uint64_t n_idx, uint64_t* out) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n_idx * layers) return;
    const uint64_t q = j / layers, leaf = idx[q];
    const uint32_t i = (uint32_t)(j % layers);
    const uint64_t tree_len = 2 * ((1ull << layers) - 1);
    const uint64_t pair = (leaf & ((1ull << layers) - 1)) >> i;      // the node of layer i on the path; its sibling is pair ^ 1
    const uint64_t* src = digests + ((leaf >> layers) * tree_len + digest_slot(i, pair ^ 1)) * 4;
    const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(src), hi = *reinterpret_cast<const ulonglong2*>(src + 2);
    *reinterpret_cast<ulonglong2*>(out + j * 4) = lo;
    *reinterpret_cast<ulonglong2*>(out + j * 4 + 2) = hi;
}

template <class H> GL_DEV void two_to_one_body(const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t* out) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s[12] = {H::in2(l[4 * i]), H::in2(l[4 * i + 1]), H::in2(l[4 * i + 2]), H::in2(l[4 * i + 3]),
                      H::in2(r[4 * i]), H::in2(r[4 * i + 1]), H::in2(r[4 * i + 2]), H::in2(r[4 * i + 3]), 0, 0, 0, 0};
    H::permute(s);
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * i + k] = H::out(s[k]);
}

template <class H> GL_DEV void pow_grind_units_body(const PowArgs& a) {
    const uint32_t u = blockIdx.y;
    if (!a.todo[u]) return;
    const uint64_t w = a.start + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    // the smallest witness wins, so a candidate above the best one found so far cannot matter: workgroups are dispatched in
    // roughly increasing order, and once a witness is known the rest of the launch exits here (expected work ~2^bits instead of the
    // 2^(bits+1) candidates of the launch); candidates below the current best are never skipped, so the result is still the minimum
    if (w > __hip_atomic_load(a.best + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    uint64_t s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = a.state[u * 12 + k];
#pragma unroll
    for (int k = 0; k < 12; k++) if ((uint32_t)k == a.pos[u]) s[k] = w;
    H::permute(s);
    const uint64_t resp = H::out(s[7]);
    if (a.bits == 0 || (resp >> (64 - a.bits)) == 0) atomicMin(a.best + u, (unsigned long long)w);
}
#endif  // __HIPCC__

}  // namespace gl355
