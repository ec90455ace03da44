// Second hash back-end: the reference's Bn254PoseidonHash (src/plonky2_verifier/bn245_poseidon/plonky2_config.rs:57-75
// over native.rs:16-77) for permutation batches, leaf hashing, Merkle levels, two_to_one and PoW -- the hasher of the
// final wrap proof (wrapper.rs:35-56 with OuterC = Bn254PoseidonGoldilocksConfig).  SURVEY 8(f) N1.
//
// The one-lane-per-state kernels are merkle_common.cuh's bodies with this file's policy (the permutation of bn254.cuh: ~2 000 254-bit
// Montgomery products, ~35x the Goldilocks Poseidon), launched by merkle.hip's launch code through the table at the end of this
// file; what is this hasher's own are the lane-parallel level kernel and the choice of kernel per level (bn254_above_leaves).
#include "gl355_internal.h"
#include "bn254.cuh"
#include "merkle_common.cuh"

namespace gl355 {

// the BN254-Poseidon policy of merkle_common.cuh's kernel bodies
struct Bn254Hasher {
    static constexpr bool wide_digests = false;
    static GL_DEV void permute(uint64_t (&s)[12]) { bn254_permute(s); }
    static GL_DEV uint64_t out(uint64_t x) { return x; }
    static GL_DEV uint64_t in2(uint64_t x) { return gl_canon(x); }
};

__global__ void __launch_bounds__(256) bn254_permute_kernel(uint64_t* states, uint64_t count) { permute_body<Bn254Hasher>(states, count); }

__global__ void __launch_bounds__(256) bn254_hash_leaves_kernel(LeafArgs a) { hash_leaves_body<Bn254Hasher>(a); }

__global__ void __launch_bounds__(256) bn254_merkle_level_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer,
                                                                uint64_t n_nodes) {
    merkle_level_body<Bn254Hasher>(digests, cap, sub_bits, layer, n_nodes);
}

// in-place update of a resident tree: this hasher has no 16-lane form, so every dirty layer takes the one-lane kernel
__global__ void __launch_bounds__(256) bn254_merkle_update_leaves_kernel(UpdateLeafArgs a) { update_leaves_body<Bn254Hasher>(a); }

__global__ void __launch_bounds__(256) bn254_merkle_update_level_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer,
                                                                       const uint64_t* list, uint64_t n_list) {
    merkle_update_level_body<Bn254Hasher>(digests, cap, sub_bits, layer, list, n_list);
}

// ------------------------------------------------------------------------------------------------------------------
// Lane-parallel permutation for SMALL levels.  With one lane per node a level costs one full permutation latency
// (~2.4 ms: 2 000 dependent Montgomery products) however few nodes it has, and a proof walks ~140 such levels.  Here 32
// lanes share one state as a 5 x 5 grid: lane (i, j) holds s_j (every lane of column j computes the same round-constant
// addition and S-box), forms the single product M[i][j] * s_j, and the five products of row j are summed back into s_j
// through a 25-slot LDS tile -- 4 products + 4 additions per round on the critical path instead of 28..40 products:
// ~7x lower latency at ~4.6x the instruction count, so it is used only below 2^13 nodes (BN254_LANES_MAX_LOG).
// ------------------------------------------------------------------------------------------------------------------
#define BN254_LANES_MAX_LOG 13

GL_DEV fr8 lds_load_fr(const uint32_t* p) {
    fr8 r;
#pragma unroll
    for (int k = 0; k < FR_W; k++) r.l[k] = p[k];
    return r;
}

// block = 64 threads = two 32-lane groups = two parent nodes of layer `layer`
__global__ void __launch_bounds__(64) bn254_merkle_level_lanes_kernel(uint64_t* digests, uint64_t* cap, uint32_t sub_bits, uint32_t layer,
                                                                     uint64_t n_nodes) {
    __shared__ uint32_t tile[2][25 * FR_W];
    const int grp = threadIdx.x >> 5, l = threadIdx.x & 31;
    const bool act = l < 25;
    const int i = act ? l / 5 : 0, j = act ? l % 5 : 0;
    uint64_t g = blockIdx.x * 2ull + grp;
    const bool valid = g < n_nodes;
    if (!valid) g = 0;
    const MerkleNode nd = merkle_node(digests, cap, sub_bits, layer, g);
    // column j packs sponge elements 3j .. 3j+2 of (left digest | right digest | 0^4)
    uint64_t e[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int idx = 3 * j + q;
        e[q] = idx < 8 ? nd.tree[nd.child() * 4 + idx] : 0;
    }
    fr8 s = fr_encode3(e[0], e[1], e[2]);            // column 4 (and the padding of column 2, 3) encodes zeros
    const fr8 m = fr_const(BN254F_MDS[5 * i + j]);
    uint32_t* my = tile[grp];
    fr8 rc = fr_const(BN254F_RC[j]);
#pragma unroll 1
    for (int rnd = 0; rnd < 68; rnd++) {
        const fr8 rc_next = fr_const(BN254F_RC[5 * (rnd < 67 ? rnd + 1 : 67) + j]);   // prefetch: the index depends on the lane
        s = fr_add(s, rc);
        rc = rc_next;
        const fr8 sb = fr_pow5(s);
        const bool full = rnd < 4 || rnd >= 64;
        if (full || j == 0) s = sb;
        const fr8 p = fr_mul(s, m);
        if (act) {
#pragma unroll
            for (int q = 0; q < FR_W; q++) my[(5 * i + j) * FR_W + q] = p.l[q];
        }
        GL_WAVE_LDS_SYNC();
        fr8 acc = lds_load_fr(my + (5 * j) * FR_W);     // new s_j = sum_c M[j][c] s_c: row j of the product tile
#pragma unroll
        for (int c = 1; c < 5; c++) acc = fr_add(acc, lds_load_fr(my + (5 * j + c) * FR_W));
        GL_WAVE_LDS_SYNC();
        s = acc;
    }
    uint64_t d[3];
    fr_decode3(s, d);
    // digest = sponge elements 0..3 = digits 0..2 of column 0 and digit 0 of column 1 (row 0 lanes write)
    if (valid && act && i == 0) {
        uint64_t* dst = nd.dst();
        if (j == 0) { dst[0] = d[0]; dst[1] = d[1]; dst[2] = d[2]; }
        if (j == 1) dst[3] = d[0];
    }
}

__global__ void __launch_bounds__(256) bn254_two_to_one_kernel(const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t* out) { two_to_one_body<Bn254Hasher>(l, r, n, out); }

__global__ void __launch_bounds__(256) bn254_pow_grind_units_kernel(PowArgs a) { pow_grind_units_body<Bn254Hasher>(a); }

// every level one launch: 32 lanes per node up to lanes_max nodes, one lane per node above
static int32_t bn254_above_leaves(Ctx* ctx, uint64_t n_leaves, uint32_t sub_bits, uint64_t* digests, uint64_t* cap) {
    const uint64_t lanes_max = (1ull << BN254_LANES_MAX_LOG) - 1;
    for (uint32_t layer = 1; layer <= sub_bits; layer++) {
        const uint64_t n_nodes = n_leaves >> layer;
        const bool lanes = n_nodes <= lanes_max;
        ProfScope ps(ctx, lanes ? "bn254_merkle_level_lanes_kernel" : "bn254_merkle_level_kernel", n_nodes * 96);
        if (lanes)
            hipLaunchKernelGGL(bn254_merkle_level_lanes_kernel, dim3((uint32_t)((n_nodes + 1) / 2)), dim3(64), 0, ctx->stream, digests, cap,
                               sub_bits, layer, n_nodes);
        else
            hipLaunchKernelGGL(bn254_merkle_level_kernel, dim3((uint32_t)((n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, digests, cap,
                               sub_bits, layer, n_nodes);
        GL355_HIP(ctx, hipGetLastError());
    }
    return GL355_OK;
}

const HasherLaunch& bn254_hasher_launch() {
    static const HasherLaunch h = {
        bn254_permute_kernel, bn254_hash_leaves_kernel, bn254_two_to_one_kernel, bn254_pow_grind_units_kernel,
        "bn254_permute_kernel", "bn254_hash_leaves_kernel", "bn254_two_to_one_kernel", "bn254_pow_grind_units_kernel", 20, bn254_above_leaves,
        bn254_merkle_update_leaves_kernel, bn254_merkle_update_level_kernel, "bn254_merkle_update_leaves_kernel", "bn254_merkle_update_level_kernel", false};
    return h;
}

// ---- test hook: the hasher's fr_enter / fr_leave on raw 9-word records (gl355_bn254_arith_batch, GL355_BN_HASH_FR_*; device buffers)
__global__ void bn254_hash_fr_hook_kernel(int32_t leave, const uint32_t* a, uint32_t* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* pa = a + 9 * i;
    uint32_t* po = out + 9 * i;
    uint64_t w[4];
    if (!leave) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = (uint64_t)pa[2 * k] | ((uint64_t)pa[2 * k + 1] << 32);
        const fr8 r = fr_enter(w);
#pragma unroll
        for (int j = 0; j < FR_W; j++) po[j] = r.l[j];
    } else {
        fr8 x;
#pragma unroll
        for (int j = 0; j < FR_W; j++) x.l[j] = pa[j];
        fr_leave(x, w);
#pragma unroll
        for (int k = 0; k < 4; k++) { po[2 * k] = (uint32_t)w[k]; po[2 * k + 1] = (uint32_t)(w[k] >> 32); }
        po[8] = 0;
    }
}
int32_t bn254_hash_fr_hook(Ctx* ctx, int32_t leave, const uint32_t* a, uint32_t* out, uint64_t n) {
    hipLaunchKernelGGL(bn254_hash_fr_hook_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, leave, a, out, n);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

}  // namespace gl355
