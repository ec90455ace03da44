// Poseidon sponge, Merkle tree with cap and proof-of-work grinding for gfx950 (a6, a7, a8, a13).
//
// Replaces plonky2::hash::hashing::{hash_n_to_m_no_pad, compress}, Hasher::{hash_or_noop,
// two_to_one}, plonky2::hash::merkle_tree::{MerkleTree::new, fill_digests_buf, fill_subtree} and
// plonky2::fri::prover::fri_proof_of_work; reached from the reference at
// src/plonky2_semaphore/signal.rs:40, access_set.rs:67,205, recursion.rs:360 and inside every
// PolynomialBatch commitment.  Semantics pinned by chip/hasher_chip.rs:122-148 (overwrite sponge,
// rate 8), chip/merkle_proof_chip.rs:39-87 (leaf <= 4 elements is its own digest; bit k of the
// index = 1 means "current node is the right child") and chip/fri_chip.rs:364-376 (PoW).
//
// Design: these kernels are integer-VALU bound (one permutation ~ 1.1 k 64-bit modmuls), not HBM
// bound, so the layout goal is only "never waste a load": leaves are read straight from the
// column-major LDE the NTT wrote (lane i reads element i of a column: perfectly coalesced; the
// row-major transpose plonky2 performs is never materialised on the commit path), and the digests
// are written directly into plonky2's recursive `digests` layout so no later shuffle is needed.
#include "gl355_internal.h"
#include "poseidon.cuh"
#include "merkle_common.cuh"
#include "poseidon_lanes.cuh"

namespace gl355 {

// levels with at most this many nodes use the lane-parallel kernel (4 nodes per wave): beyond ~2^14 nodes
// the chip is full of waves either way and the one-lane-per-node kernel wins on instruction count
// the default of Ctx::merkle_lanes_log (gl355_ctx_set_option) is 14: see the lane-parallel permutation (poseidon_lanes.cuh)

// the Poseidon-Goldilocks policy of merkle_common.cuh's kernel bodies
struct PoseidonHasher {
    static constexpr bool wide_digests = true;
    static GL_DEV void permute(uint64_t (&s)[12]) { psd_permute(s); }
    static GL_DEV uint64_t out(uint64_t x) { return gl_canon(x); }
    static GL_DEV uint64_t in2(uint64_t x) { return x; }
};

__global__ void __launch_bounds__(256) poseidon_permute_kernel(uint64_t* states, uint64_t count) { permute_body<PoseidonHasher>(states, count); }

constexpr int psd_leaf_waves = 4;
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(psd_leaf_waves))) hash_leaves_kernel(LeafArgs a) { hash_leaves_body<PoseidonHasher>(a); }

__global__ void __launch_bounds__(256) merkle_level_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits,
                                                          uint32_t layer, uint64_t n_nodes /* all subtrees */) {
    merkle_level_body<PoseidonHasher>(digests, cap, sub_bits, layer, n_nodes);
}

// one 16-lane group = one parent node g of layer `layer` (counted over all subtrees): lane li < 8 loads word li of the two children, lanes 0 .. 3 store the
// digest.  A group without a node of its own is given any node and valid = false: it goes through the permutation (the ring exchange and the DPP
// broadcast need the whole wave) and skips only its store.
template <int FORM>
GL_DEV void merkle_node_lanes(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer, uint64_t g, bool valid, int li, uint64_t* ring) {
    const MerkleNode nd = merkle_node(digests, cap, sub_bits, layer, g);
    uint64_t s = (li < 8) ? nd.tree[nd.child() * 4 + li] : 0;      // left child, then the right one
    s = psd_permute_lanes<FORM>(s, li, ring);
    if (valid && li < 4) nd.dst()[li] = gl_canon(s);
}

// one 16-lane group = one parent node of layer `layer`; block = 64 threads = 4 nodes
template <int FORM>
__global__ void __launch_bounds__(64) merkle_level_lanes_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits,
                                                               uint32_t layer, uint64_t n_nodes) {
    __shared__ uint64_t rings[4][24];
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    uint64_t g = blockIdx.x * 4ull + grp;
    const bool valid = g < n_nodes;
    if (!valid) g = 0;  // keep the whole wave in the barriers
    merkle_node_lanes<FORM>(digests, cap, sub_bits, layer, g, valid, li, rings[grp]);
}

// ---- in-place update of a resident tree (gl355_merkle_tree_update; the dirty lists: merkle_update_plan.h) ----
__global__ void __launch_bounds__(256) merkle_update_leaves_kernel(UpdateLeafArgs a) { update_leaves_body<PoseidonHasher>(a); }

__global__ void __launch_bounds__(256) merkle_update_level_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer,
                                                                 const uint64_t* list, uint64_t n_list) {
    merkle_update_level_body<PoseidonHasher>(digests, cap, sub_bits, layer, list, n_list);
}

// merkle_level_lanes_kernel over a dirty list: group e takes node list[e]; a group past the end clamps to entry 0 and skips only its store
template <int FORM>
__global__ void __launch_bounds__(64) merkle_update_level_lanes_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer,
                                                                      const uint64_t* list, uint64_t n_list) {
    __shared__ uint64_t rings[4][24];
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    uint64_t e = blockIdx.x * 4ull + grp;
    const bool valid = e < n_list;
    if (!valid) e = 0;
    merkle_node_lanes<FORM>(digests, cap, sub_bits, layer, list[e], valid, li, rings[grp]);
}

// The top of the dirty path in ONE launch of ONE workgroup: 1024 threads = 64 groups of 16 lanes take the at most 64 dirty nodes of layer layer0, then
// of every layer above it up to the subtree roots (n_layers layers; their ids follow one another in `list`, counts.n[l] of them in layer layer0 + l).  A
// dirty child's digest was written to HBM by this workgroup one layer earlier and is read back behind the __syncthreads() between the layers: the
// workgroup-scope release / barrier / acquire of DESIGN 4.9 "Visibility" -- one workgroup's vector memory operations go through its CU's one L1 in
// order.  Nothing wider is relied on: the layers below were written by earlier launches on the same stream.  Hang safety: n_layers and the counts are
// kernel arguments, every thread reaches every barrier, a group without a node clamps to entry 0 of its layer and still arrives, a wave none of whose
// groups has a node skips the permutation (a wave-uniform branch without a barrier inside) and arrives too, and no thread returns early.
template <int FORM>
__global__ void __launch_bounds__(1024) merkle_update_climb_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer0, uint32_t n_layers,
                                                                  const uint64_t* list, ClimbCounts counts) {
    __shared__ uint64_t rings[64][24];
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int wave_first_grp = (threadIdx.x >> 6) << 2;
    uint32_t first = 0;
    for (uint32_t l = 0; l < n_layers; l++) {
        const int cnt = counts.n[l];
        if (wave_first_grp < cnt) {
            const bool valid = grp < cnt;
            merkle_node_lanes<FORM>(digests, cap, sub_bits, layer0 + l, list[first + (valid ? grp : 0)], valid, li, rings[grp]);
        }
        first += cnt;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) merkle_paths_kernel(const uint64_t* digests, uint32_t layers, const uint64_t* idx, uint64_t n_idx, uint64_t* out) {
    merkle_paths_body(digests, layers, idx, n_idx, out);
}

// leaf idx[q] of the resident row-major leaf array into out [n_idx][leaf_len]: one thread per word
__global__ void __launch_bounds__(256) merkle_gather_leaves_kernel(const uint64_t* leaves, uint32_t leaf_len, const uint64_t* idx, uint64_t n_idx, uint64_t* out) {
    const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (j >= n_idx * leaf_len) return;
    out[j] = leaves[idx[j / leaf_len] * leaf_len + j % leaf_len];
}

// FRI layer leaves of 2A = 2 << AB words (A = 4, 8, 16), one 16-lane group per leaf, four leaves per wave.  Word w of leaf i is column w & 1,
// element A i + (w >> 1) of the unit's two value columns, so for chunk c of the overwrite sponge lane li < 8 loads word li of the chunk from
// column li & 1, element A i + 4 c + (li >> 1): 32 contiguous bytes per column and group.  The same lanes write the chunk into the row-major
// leaf array [B][nl][2A] the layer openings read (64 contiguous bytes per group), so these layers need no copy launch.  1 / 2 / 4
// permutations for AB = 2 / 3 / 4.  g = leaf over all units; a group past the end clamps to leaf 0 and skips its stores only: the ring
// exchange needs the whole wave.  Digest where hash_leaves_kernel puts it.
template <int AB, int FORM>
__global__ void __launch_bounds__(64) fri_wide_leaves_units_kernel(const uint64_t* vals /* [B][2][len_v] */, uint64_t len_v, uint32_t log_nl,
                                                                  uint64_t* leaves /* [B][nl][2A] */, uint64_t n_groups /* B nl */,
                                                                  uint64_t* digests, uint64_t* cap, uint32_t sub_bits) {
    __shared__ uint64_t rings[4][24];
    constexpr int CHUNKS = 1 << (AB - 2);
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    uint64_t g = blockIdx.x * 4ull + grp;
    const bool valid = g < n_groups;
    if (!valid) g = 0;
    const uint64_t u = g >> log_nl, i = g & ((1ull << log_nl) - 1);
    const uint64_t* src = vals + (u * 2 + (li & 1)) * len_v + (i << AB) + (li >> 1);
    uint64_t* row = leaves + (g << (AB + 1)) + li;
    uint64_t s = 0;
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        if (li < 8) {
            s = src[4 * c];
            if (valid) row[8 * c] = s;
        }
        s = psd_permute_lanes<FORM>(s, li, rings[grp]);
    }
    if (valid && li < 4) leaf_digest_dst(digests, cap, 0, sub_bits, g)[li] = gl_canon(s);
}

// The top of every cap subtree in ONE launch: one 1024-thread block per subtree takes its 2^(n_levels - 1) nodes of layer `layer0` (at most
// 128) and climbs n_levels levels to the cap entry, the digests of a level staying in LDS for the next one (and going to the plonky2
// layout in HBM).  Each of those levels is one lane-parallel permutation deep (two for the 128-node level: 64 groups of 16 lanes); as
// separate launches they cost ~20 us apiece, mostly launch latency -- round 2 ran the last six levels here and two more as separate
// lane-parallel launches (12.7 % of the kernel time of the 8-context profile between them); with eight levels a tree is leaf hashing,
// its wide levels, and this.  Trees of at most 2^8 leaves per cap entry are built whole.  Waves whose groups have no node on a level skip it.
#define MERKLE_TOP_LEVELS 8
template <int FORM>
__global__ void __launch_bounds__(1024) merkle_top_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer0, uint32_t n_levels) {
    __shared__ uint64_t rings[64][24];
    __shared__ uint64_t lvl[2][(1 << (MERKLE_TOP_LEVELS - 1)) * 4];
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int wave_first_grp = (threadIdx.x >> 6) << 2;
    const uint64_t t = blockIdx.x;
    int cur = 0;
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint32_t layer = layer0 + l;
        const int cnt = 1 << (n_levels - 1 - l);
        for (int base = 0; base < cnt; base += 64) {
            if (base + wave_first_grp < cnt) {                // wave-uniform: this wave owns at least one node of the round
                const bool valid = base + grp < cnt;
                const int j = valid ? base + grp : 0;
                const MerkleNode nd = merkle_node(digests, cap, sub_bits, layer, t, (uint64_t)j);
                uint64_t s = 0;
                if (li < 8) s = (l == 0) ? nd.tree[nd.child() * 4 + li] : lvl[cur][(2 * j) * 4 + li];
                s = psd_permute_lanes<FORM>(s, li, rings[grp]);
                if (valid && li < 4) {
                    const uint64_t v = gl_canon(s);
                    lvl[cur ^ 1][j * 4 + li] = v;
                    nd.dst()[li] = v;
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

__global__ void __launch_bounds__(256) two_to_one_kernel(const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t* out) { two_to_one_body<PoseidonHasher>(l, r, n, out); }

__global__ void __launch_bounds__(256) pow_grind_units_kernel(PowArgs a) { pow_grind_units_body<PoseidonHasher>(a); }

// ------------------------------------------------------------------------------------------------
// The launch code of both back-ends: `hasher` picks the table (GL355_HASH_*, checked at the C ABI).
static const HasherLaunch& launch_of(int32_t hasher) {
    static const HasherLaunch poseidon = {
        poseidon_permute_kernel, hash_leaves_kernel, two_to_one_kernel, pow_grind_units_kernel,
        "poseidon_permute_kernel", "hash_leaves_kernel", "two_to_one_kernel", "pow_grind", 22, merkle_build_above_leaves,
        merkle_update_leaves_kernel, merkle_update_level_kernel, "merkle_update_leaves_kernel", "merkle_update_level_kernel", true};
    return hasher == GL355_HASH_BN254_POSEIDON ? bn254_hasher_launch() : poseidon;
}

int32_t permute_dev(Ctx* ctx, int32_t hasher, uint64_t* states, uint64_t count) {
    if (count == 0) return GL355_OK;
    const HasherLaunch& h = launch_of(hasher);
    ProfScope ps(ctx, h.permute_scope, count * 192);
    hipLaunchKernelGGL(h.permute, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, ctx->stream, states, count);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

static int32_t launch_leaves(Ctx* ctx, const HasherLaunch& h, const LeafArgs& a) {
    if (a.n_leaves == 0) return GL355_OK;
    ProfScope ps(ctx, h.leaves_scope, a.n_leaves * ((uint64_t)a.leaf_len * 8 + 32));
    hipLaunchKernelGGL(h.leaves, dim3((uint32_t)((a.n_leaves + 255) / 256)), dim3(256), 0, ctx->stream, a);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

static LeafArgs leaf_args(const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, bool col_major, uint64_t col_stride) {
    LeafArgs a;
    memset(&a, 0, sizeof a);
    a.leaves = leaves; a.n_leaves = n_leaves; a.leaf_len = leaf_len; a.col_major = col_major;
    a.stride = col_major ? col_stride : leaf_len;
    return a;
}

int32_t hash_leaves_dev(Ctx* ctx, int32_t hasher, const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, bool col_major,
                        uint64_t col_stride, uint64_t* digests, bool always_hash) {
    LeafArgs a = leaf_args(leaves, n_leaves, leaf_len, col_major, col_stride);
    a.out = digests; a.linear = 1; a.always_hash = always_hash;
    return launch_leaves(ctx, launch_of(hasher), a);
}

int32_t two_to_one_dev(Ctx* ctx, int32_t hasher, const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t* out) {
    if (n == 0) return GL355_OK;
    const HasherLaunch& h = launch_of(hasher);
    ProfScope ps(ctx, h.two_to_one_scope, n * 96);
    hipLaunchKernelGGL(h.two_to_one, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, l, r, n, out);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

int32_t merkle_build_dev(Ctx* ctx, int32_t hasher, const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, bool col_major,
                         uint64_t col_stride, uint32_t cap_height, uint64_t* digests, uint64_t* cap) {
    const uint32_t log_n = log2_u64(n_leaves);
    if ((1ull << log_n) != n_leaves) return ctx->fail(GL355_E_INVALID_ARG, "merkle: n_leaves must be a power of two");
    if (cap_height > log_n) return ctx->fail(GL355_E_INVALID_ARG, "merkle: cap_height > log2(n_leaves)");
    return merkle_build_args(ctx, hasher, leaf_args(leaves, n_leaves, leaf_len, col_major, col_stride), log_n - cap_height, digests, cap);
}

// a.n_leaves leaves (any multiple of 2^sub_bits: the cap subtrees of one tree, or of several units' trees laid out one after
// the other) -> per-subtree digests in plonky2's layout + one cap entry per subtree.  `a` describes where the leaves are.
int32_t merkle_build_args(Ctx* ctx, int32_t hasher, LeafArgs a, uint32_t sub_bits, uint64_t* digests, uint64_t* cap) {
    const uint64_t n_leaves = a.n_leaves;
    if (n_leaves == 0 || (n_leaves & ((1ull << sub_bits) - 1))) return ctx->fail(GL355_E_INVALID_ARG, "merkle: leaves do not fill whole cap subtrees");
    const HasherLaunch& h = launch_of(hasher);
    a.out = digests; a.cap = cap; a.sub_bits = sub_bits; a.linear = 0;
    GL355_TRY(launch_leaves(ctx, h, a));
    return h.above_leaves(ctx, n_leaves, sub_bits, digests, cap);
}

int32_t fri_wide_leaves_tree_dev(Ctx* ctx, uint32_t ab, uint32_t B, const uint64_t* vals, uint64_t len_v, uint64_t* leaves, uint32_t sub_bits,
                                 uint64_t* digests, uint64_t* cap) {
    const uint64_t nl = len_v >> ab, n_groups = (uint64_t)B * nl;
    if (ab < 2 || ab > 4 || nl == 0 || (nl & (nl - 1)) || (nl << ab) != len_v || (nl & ((1ull << sub_bits) - 1)) || (n_groups + 3) / 4 > 0x7FFFFFFFull)
        return ctx->fail(GL355_E_INVALID_ARG, "fri: wide leaves need 4, 8 or 16 values per leaf and whole cap subtrees");
    const uint32_t log_nl = log2_u64(nl);
    const dim3 grid((uint32_t)((n_groups + 3) / 4)), block(64);
    const bool fast_lanes = (n_groups >> sub_bits) < 64;      // as merkle_build_above_leaves: form 3 for a lone unit's few subtrees, form 0 for lock-step batches
    {
        ProfScope ps(ctx, "fri_wide_leaves_units_kernel", n_groups * ((32ull << ab) + 32));
#define GL355_WIDE_LEAVES(AB)                                                                                                                         \
        if (fast_lanes) hipLaunchKernelGGL((fri_wide_leaves_units_kernel<AB, 3>), grid, block, 0, ctx->stream, vals, len_v, log_nl, leaves, n_groups, \
                                           digests, cap, sub_bits);                                                                                   \
        else hipLaunchKernelGGL((fri_wide_leaves_units_kernel<AB, 0>), grid, block, 0, ctx->stream, vals, len_v, log_nl, leaves, n_groups, digests,   \
                                cap, sub_bits)
        switch (ab) {
            case 2: GL355_WIDE_LEAVES(2); break;
            case 3: GL355_WIDE_LEAVES(3); break;
            default: GL355_WIDE_LEAVES(4); break;
        }
#undef GL355_WIDE_LEAVES
        GL355_HIP(ctx, hipGetLastError());
    }
    return merkle_build_above_leaves(ctx, n_groups, sub_bits, digests, cap);
}

int32_t merkle_build_above_leaves(Ctx* ctx, uint64_t n_leaves, uint32_t sub_bits, uint64_t* digests, uint64_t* cap) {
    const uint64_t lanes_max = 1ull << ctx->merkle_lanes_log;
    // the last MERKLE_TOP_LEVELS levels of every cap subtree go to merkle_top_kernel (when they are lane-parallel levels anyway: at most
    // lanes_max nodes enter it over the whole forest)
    // Eight levels per block cost three dependent permutations more than six levels behind two forest-wide lane-parallel launches: with
    // few subtrees (one proof: 16) the separate launches spread over the whole chip and the tree is done sooner (single-unit latency 17.0 vs
    // 17.6 ms); with a lock-step batch (>= 64 subtrees) the chip is full either way and four launches fewer per unit win
    // (profiles/r03_merkle_top_ab.txt).
    const uint32_t top_levels_max = (n_leaves >> sub_bits) < 64 ? 6 : MERKLE_TOP_LEVELS;
    // a lone proof's forest (16 cap subtrees) is latency-bound: the partial rounds with the row inside the S-box (psd_permute_lanes<3>); a lock-step batch
    // shares the chip with other contexts' hash kernels, where the 16 extra registers of that form cost more than its shorter chain gains
    const bool fast_lanes = (n_leaves >> sub_bits) < 64;
    uint32_t top_levels = std::min<uint32_t>(top_levels_max, sub_bits);
    while (top_levels > 1 && ((n_leaves >> (sub_bits - top_levels + 1)) > lanes_max)) top_levels--;      // a forest of many subtrees: fewer levels each
    uint32_t top_from = sub_bits + 1;
    if (top_levels >= 1 && ((n_leaves >> (sub_bits - top_levels + 1)) <= lanes_max)) top_from = sub_bits - top_levels + 1;
    for (uint32_t layer = 1; layer <= sub_bits; layer++) {
        const uint64_t n_nodes = n_leaves >> layer;
        if (layer == top_from) {
            ProfScope ps(ctx, "merkle_top_kernel", (2 * n_nodes - (n_leaves >> sub_bits)) * 96);
            if (fast_lanes) hipLaunchKernelGGL(merkle_top_kernel<3>, dim3((uint32_t)(n_leaves >> sub_bits)), dim3(1024), 0, ctx->stream, digests, cap, sub_bits, layer, top_levels);
            else hipLaunchKernelGGL(merkle_top_kernel<0>, dim3((uint32_t)(n_leaves >> sub_bits)), dim3(1024), 0, ctx->stream, digests, cap, sub_bits, layer, top_levels);
            GL355_HIP(ctx, hipGetLastError());
            break;
        }
        // one scope per level (= per launch): 2 child digests in, 1 out per node
        ProfScope ps(ctx, n_nodes <= lanes_max ? "merkle_level_lanes_kernel" : "merkle_level_kernel", n_nodes * 96);
        if (n_nodes <= lanes_max) {
            // small level: 16 lanes per node (latency ~10x lower than one lane per node)
            if (fast_lanes) hipLaunchKernelGGL(merkle_level_lanes_kernel<3>, dim3((uint32_t)((n_nodes + 3) / 4)), dim3(64), 0, ctx->stream,
                                               digests, cap, sub_bits, layer, n_nodes);
            else hipLaunchKernelGGL(merkle_level_lanes_kernel<0>, dim3((uint32_t)((n_nodes + 3) / 4)), dim3(64), 0, ctx->stream,
                                    digests, cap, sub_bits, layer, n_nodes);
        } else {
            hipLaunchKernelGGL(merkle_level_kernel, dim3((uint32_t)((n_nodes + 255) / 256)), dim3(256), 0, ctx->stream,
                               digests, cap, sub_bits, layer, n_nodes);
        }
        GL355_HIP(ctx, hipGetLastError());
    }
    return GL355_OK;
}

// The resident tree's update.  The caller's n_rows new rows go up as they came; the k = p.leaves.size() leaves to write, the row each one takes
// (p.src) and, unless `full`, the plan's dirty lists go up in one more copy.  Then leaf words + digests, then layer by layer the kernel
// merkle_update_kernel_of names -- or, for a full update, the hasher's whole above_leaves.  The 16-lane form is merkle_build_above_leaves' choice:
// form 3 below 64 cap subtrees, form 0 from there.  Ends with a wait for the stream: the staging is a local of this call.
int32_t merkle_update_dev(Ctx* ctx, const gl355_merkle_tree* t, const MerkleUpdatePlan& p, const uint64_t* rows_host, uint64_t n_rows, bool full) {
    const HasherLaunch& h = launch_of(t->hasher);
    const uint64_t k = p.leaves.size(), row_words = n_rows * t->leaf_len, n_nodes = full ? 0 : p.nodes.size();
    if (k == 0) return GL355_OK;
    if ((k + 255) / 256 > 0x7FFFFFFFull || (!full && !merkle_update_grids_fit(p))) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree_update: too many leaves for one launch");
    std::vector<uint64_t> stage(2 * k + n_nodes);
    std::copy(p.leaves.begin(), p.leaves.end(), stage.begin());
    std::copy(p.src.begin(), p.src.end(), stage.begin() + k);
    std::copy(p.nodes.begin(), p.nodes.begin() + n_nodes, stage.begin() + 2 * k);
    Scratch sc(ctx);
    GL355_TRY(sc.get((stage.size() + row_words) * 8));
    uint64_t* d_idx = sc.as<uint64_t>();
    const uint64_t* d_nodes = d_idx + 2 * k;
    uint64_t* d_rows = d_idx + stage.size();
    GL355_HIP(ctx, hipMemcpyAsync(d_idx, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    GL355_HIP(ctx, hipMemcpyAsync(d_rows, rows_host, row_words * 8, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, h.update_leaves_scope, k * ((uint64_t)t->leaf_len * 16 + 48));
        const UpdateLeafArgs a{d_idx, d_idx + k, d_rows, k, n_rows, t->leaves, t->leaf_len, t->sub_bits, t->digests, t->cap};
        hipLaunchKernelGGL(h.update_leaves, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, ctx->stream, a);
        GL355_HIP(ctx, hipGetLastError());
    }
    if (full) GL355_TRY(h.above_leaves(ctx, t->n_leaves, t->sub_bits, t->digests, t->cap));
    const bool fast_lanes = (t->n_leaves >> t->sub_bits) < 64;
    for (uint32_t layer = 1; !full && layer <= t->sub_bits; layer++) {
        const uint64_t cnt = p.count(layer);
        const uint64_t* list = d_nodes + p.offset[layer];
        const MerkleUpdateKernel which = merkle_update_kernel_of(p, layer, ctx->merkle_lanes_log, h.lanes16);
        if (which == MERKLE_UPDATE_CLIMB) {
            const uint32_t n_layers = t->sub_bits - layer + 1;
            ClimbCounts counts;
            memset(&counts, 0, sizeof counts);
            for (uint32_t l = 0; l < n_layers; l++) counts.n[l] = (uint8_t)p.count(layer + l);
            ProfScope ps(ctx, "merkle_update_climb_kernel", (p.nodes.size() - p.offset[layer]) * 104);
            if (fast_lanes) hipLaunchKernelGGL(merkle_update_climb_kernel<3>, dim3(1), dim3(1024), 0, ctx->stream, t->digests, t->cap, t->sub_bits, layer, n_layers, list, counts);
            else hipLaunchKernelGGL(merkle_update_climb_kernel<0>, dim3(1), dim3(1024), 0, ctx->stream, t->digests, t->cap, t->sub_bits, layer, n_layers, list, counts);
            GL355_HIP(ctx, hipGetLastError());
            break;
        }
        // 2 child digests and the node id in, 1 digest out per node
        ProfScope ps(ctx, which == MERKLE_UPDATE_LANES ? "merkle_update_level_lanes_kernel" : h.update_level_scope, cnt * 104);
        if (which == MERKLE_UPDATE_LANES) {
            if (fast_lanes) hipLaunchKernelGGL(merkle_update_level_lanes_kernel<3>, dim3((uint32_t)((cnt + 3) / 4)), dim3(64), 0, ctx->stream, t->digests, t->cap, t->sub_bits, layer, list, cnt);
            else hipLaunchKernelGGL(merkle_update_level_lanes_kernel<0>, dim3((uint32_t)((cnt + 3) / 4)), dim3(64), 0, ctx->stream, t->digests, t->cap, t->sub_bits, layer, list, cnt);
        } else {
            hipLaunchKernelGGL(h.update_level, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, t->digests, t->cap, t->sub_bits, layer, list, cnt);
        }
        GL355_HIP(ctx, hipGetLastError());
    }
    GL355_HIP(ctx, ctx->wait());
    return GL355_OK;
}

// rows of a resident array picked by index, into a host buffer: the indices go up, one kernel gathers, one copy comes back, and the call waits for it.
// what = 0: the Merkle paths (layers x 4 words per index, any hasher: digests are copied, not hashed); what = 1: the leaves (leaf_len words per index)
int32_t merkle_tree_gather_dev(Ctx* ctx, const gl355_merkle_tree* t, int what, const uint64_t* indices_host, uint64_t n_idx, uint64_t* out_host) {
    const uint32_t per = what == 0 ? t->sub_bits * 4 : t->leaf_len;
    const uint64_t n_out = n_idx * per;
    if (n_out == 0) return GL355_OK;
    const uint64_t n_threads = what == 0 ? n_idx * t->sub_bits : n_out;
    if ((n_threads + 255) / 256 > 0x7FFFFFFFull) return ctx->fail(GL355_E_INVALID_ARG, "merkle_tree: too many indices for one launch");
    Scratch sc(ctx);
    GL355_TRY(sc.get((n_out + n_idx) * 8));
    uint64_t* d_out = sc.as<uint64_t>();      // first: the paths move as 16-byte words
    uint64_t* d_idx = d_out + n_out;
    GL355_HIP(ctx, hipMemcpyAsync(d_idx, indices_host, n_idx * 8, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, what == 0 ? "merkle_paths_kernel" : "merkle_gather_leaves_kernel", n_out * 16 + n_idx * 8);
        const dim3 grid((uint32_t)((n_threads + 255) / 256)), block(256);
        if (what == 0) hipLaunchKernelGGL(merkle_paths_kernel, grid, block, 0, ctx->stream, t->digests, t->sub_bits, d_idx, n_idx, d_out);
        else hipLaunchKernelGGL(merkle_gather_leaves_kernel, grid, block, 0, ctx->stream, t->leaves, t->leaf_len, d_idx, n_idx, d_out);
        GL355_HIP(ctx, hipGetLastError());
    }
    GL355_HIP(ctx, ctx->d2h(out_host, d_out, n_out * 8));
    GL355_HIP(ctx, ctx->wait());
    return GL355_OK;
}

int32_t pow_grind_units_dev(Ctx* ctx, int32_t hasher, uint32_t B, const uint64_t* states, const uint32_t* pos, uint32_t bits, uint64_t start, uint64_t* landing,
                            uint64_t* const* witness_host) {
    if (bits > 40) return ctx->fail(GL355_E_UNSUPPORTED, "pow: more than 40 bits of grinding refused");
    const HasherLaunch& h = launch_of(hasher);
    PowArgs pa;
    memset(&pa, 0, sizeof pa);
    for (uint32_t u = 0; u < B; u++) {
        for (int k = 0; k < 12; k++) pa.state[u * 12 + k] = gl_canon(states[u * 12 + k]);
        pa.pos[u] = pos[u]; pa.todo[u] = 1;
    }
    Scratch pb(ctx);
    GL355_TRY(pb.get(GL355_MAX_UNITS * 8));
    pa.best = reinterpret_cast<unsigned long long*>(pb.p);
    pa.bits = bits;
    GL355_HIP(ctx, hipMemsetAsync(pb.p, 0xFF, GL355_MAX_UNITS * 8, ctx->stream));
    // within a launch the minimum wins, and earlier launches found nothing for that unit, so the result is the global minimum.
    // a launch of 2^(bits+1) candidates holds a solution with probability 1 - e^-2; units without one go again, with a larger window
    // (up to the hasher's largest window: 2^22 candidates, 2^20 of the 35x longer BN254 permutation; the window sizes do not change the witness)
    uint64_t per_launch = 1ull << std::min<uint32_t>(std::max<uint32_t>(bits + 1, 12), h.grind_window_log);
    uint64_t base = start;
    for (uint32_t left = B; left;) {
        ProfScope ps(ctx, h.grind_scope, 0);   // pure compute: one permutation per candidate, no HBM traffic
        pa.start = base;
        hipLaunchKernelGGL(h.grind, dim3((uint32_t)(per_launch / 256), B), dim3(256), 0, ctx->stream, pa);
        GL355_HIP(ctx, hipGetLastError());
        GL355_HIP(ctx, ctx->d2h(landing, pb.p, (uint64_t)B * 8));
        GL355_HIP(ctx, ctx->wait());
        for (uint32_t u = 0; u < B; u++)
            if (pa.todo[u] && landing[u] != ~0ull) { *witness_host[u] = landing[u]; pa.todo[u] = 0; left--; }
        base += per_launch;
        if (per_launch < (1ull << h.grind_window_log)) per_launch <<= 1;
        if (base - start > (1ull << 44)) return ctx->fail(GL355_E_UNSUPPORTED, "pow: no witness found in 2^44 candidates");
    }
    return GL355_OK;
}

int32_t pow_grind_dev(Ctx* ctx, int32_t hasher, const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t start,
                      uint64_t* witness_host) {
    if (pos >= 8) return ctx->fail(GL355_E_INVALID_ARG, "pow: witness position must be in the rate part");
    uint64_t landing;
    return pow_grind_units_dev(ctx, hasher, 1, state, &pos, bits, start, &landing, &witness_host);
}

}  // namespace gl355
