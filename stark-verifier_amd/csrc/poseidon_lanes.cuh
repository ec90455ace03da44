// The 16-lane Poseidon permutation (one state per 16 lanes of a wave) of the Merkle / FRI wide-leaf kernels (merkle.hip) and of its test hook
// (gl_hook.hip: gl355_poseidon_permute_lanes), and its round, psd_lane_round, which the witness tape's PoseidonGate row (witness_tape_dev.hip) runs too.
// Built on poseidon_rounds.cuh alone: nothing here reads the block tables of poseidon.cuh.
#pragma once
#include "poseidon_rounds.cuh"
#include "merkle_common.cuh"

namespace gl355 {

// ------------------------------------------------------------------------------------------------
// Lane-parallel permutation for SMALL levels.  A thread-per-node launch of a level with few nodes is
// one lonely wave per SIMD running a ~26 k-instruction dependent stream (~75 us) no matter how few
// nodes there are, and a proof walks ~100 such levels (profiles/r01_proof_kernel_stats.csv: 61 % of
// GPU time).  Here 16 lanes share one state (lane i < 12 holds element i): the S-box is one x^7 per
// lane, and the MDS row of lane r is read from a 24-slot LDS ring (state written twice, so slot
// r + j needs no modulo) -- ~10x fewer instructions per wave, i.e. ~10x lower level latency.  All
// 30 rounds use the naive form (constants + S-box + full MDS; the S-box result is kept on lane 0
// only in the 22 partial rounds): with one element per lane the dense MDS is as cheap as the sparse one.
// ------------------------------------------------------------------------------------------------
// gl_field.cuh's GL_PSD_MDS_CIRC, in a symbol of this unit's own: reading the shared table lays the unit's code out differently
// (const at namespace scope: internal linkage, so every unit that includes this header gets its own copy)
__device__ __constant__ const uint32_t PSD_CIRC_DEV[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};

// ONE round of the one-element-per-lane form, the dense round of psd_permute_lanes below and of the witness tape's PoseidonGate row
// (witness_tape_dev.hip): S-box (`sbox`: every lane in a full round, lane 0 alone in a partial one), the state through the ring, row `me` of the MDS
// layer on the 32-bit halves from the NEXT round's constant, psd_recombine.  rc_next = PSD_ALL_RC[12 * (r + 1) + me] is the caller's load: the constant
// index depends on the lane, so it is a vector load, issued before whatever the caller does ahead of the round (a load issued and awaited inside
// the round costs an L2 round trip per round, ~40 % of the latency).
GL_DEV uint64_t psd_lane_round(uint64_t s, uint64_t rc_next, bool sbox, bool active, int me, uint64_t* ring /* 24 u64 of this 16-lane group */) {
    if (sbox) s = psd_sbox(s);
    if (active) { ring[me] = s; ring[me + 12] = s; }
    GL_WAVE_LDS_SYNC();
    uint64_t al = (uint32_t)rc_next, ah = rc_next >> 32;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const uint64_t x = ring[me + j];
        const uint32_t c = PSD_CIRC_DEV[j] + ((me == 0 && j == 0) ? 8u : 0u);
        al += (uint64_t)(uint32_t)x * c;
        ah += (uint64_t)(uint32_t)(x >> 32) * c;
    }
    GL_WAVE_LDS_SYNC();
    return psd_recombine(al, ah);
}

// FORM (round 6): the 22 PARTIAL rounds of the 16-lane permutation.
//   0  as the full rounds: S-box (only lane 0's matters), the state through the ring, the whole MDS row: S-box + LDS round trip + 24 multiply-adds +
//      recombination, one after the other on the critical path;
//   3  only element 0 changes in a partial round's S-box, so the other eleven elements go through the ring BEFORE it (lane 0 publishes a zero), and each
//      lane's row over them is accumulated INSIDE lane 0's x^7: the row's twelve terms (two multiply-adds each) are the fillers of the products' carry
//      wait states (gl_mul_fill / gl_mul2_fill) -- written any other way the compiler queues the row's multiply-adds as a block in front of the S-box
//      chain (forms 1 and 2 of profiles/r06_lanes_partial_rounds_ab.txt: no gain).  x^7 then arrives by a DPP row broadcast (row_newbcast:0: one 16-lane
//      row = one state) for the last two multiply-adds.
// Form 3 is 16 % faster per permutation (tree tops 0.080 -> 0.067 ms, a lone unit 11.7 -> 11.0 ms) and costs 16 more VGPRs: under a lock-step load, where
// these kernels share the CUs with the hash kernels of nine other contexts, the job measured 0.8 % SLOWER with it (320.8 vs 323.3 units/s) -- so the
// launch code takes form 3 for a lone proof's forest (fewer than 64 cap subtrees) and form 0 for lock-step batches.
template <int FORM>
GL_DEV uint64_t psd_permute_lanes(uint64_t s, int li, uint64_t* ring /* 24 u64 of this 16-lane group */) {
    const bool active = li < 12;
    const int me = active ? li : 0;
    s = gl_add_canonical(s, PSD_ALL_RC[me]);
    auto dense_round = [&](int r, bool full) {
        const uint64_t rc_next = PSD_ALL_RC[12 * (r + 1) + me];     // row 30 is zero; consumed by this round's MDS accumulators
        s = psd_lane_round(s, rc_next, full || li == 0, active, me, ring);
    };
    if constexpr (FORM == 0) {
#pragma unroll 1
        for (int r = 0; r < 30; r++) dense_round(r, r < 4 || r >= 26);
        return s;
    }
    // row `me`'s coefficient of element 0: M[me][0] = CIRC[(12 - me) % 12], + 8 on the diagonal
    const uint32_t c_elem0 = PSD_CIRC_DEV[(12 - me) % 12] + (me == 0 ? 8u : 0u);
#pragma unroll 1
    for (int r = 0; r < 4; r++) dense_round(r, true);
#pragma unroll 1
    for (int r = 4; r < 26; r++) {
        const uint64_t rc_next = PSD_ALL_RC[12 * (r + 1) + me];
        if (active) { const uint64_t pub = li == 0 ? 0 : s; ring[me] = pub; ring[me + 12] = pub; }     // element 0 is added below, after its S-box
        GL_WAVE_LDS_SYNC();
        uint64_t xr[12];
#pragma unroll
        for (int j = 0; j < 12; j++) xr[j] = ring[me + j];
        uint64_t al = (uint32_t)rc_next, ah = rc_next >> 32;
        auto term = [&](int j) {                                   // one element of the row: two multiply-adds (the + 8 of row 0 belongs to element 0)
            al += (uint64_t)(uint32_t)xr[j] * PSD_CIRC_DEV[j];
            ah += (uint64_t)(uint32_t)(xr[j] >> 32) * PSD_CIRC_DEV[j];
        };
        // x^7 = (x x^2)(x^2 x^2), every lane computes it (lane 0's is the one used); terms 0 .. 11 ride in the carry wait states of its four products
        const uint64_t x2 = gl_mul_fill(s, s, [&](int k) { term(k); });
        uint64_t p34[2];
        { const uint64_t pa[2] = {s, x2}, pb[2] = {x2, x2}; gl_mul2_fill(pa, pb, p34, [&](int k) { term(5 + k); }); }
        const uint64_t x7 = gl_mul_fill(p34[0], p34[1], [&](int k) { if (k < 2) term(10 + k); else asm volatile("s_nop 1"); });
        const uint32_t x0l = __builtin_amdgcn_update_dpp(0u, (uint32_t)x7, 0x150, 0xf, 0xf, false);           // row_newbcast:0
        const uint32_t x0h = __builtin_amdgcn_update_dpp(0u, (uint32_t)(x7 >> 32), 0x150, 0xf, 0xf, false);
        al += (uint64_t)x0l * c_elem0;
        ah += (uint64_t)x0h * c_elem0;
        GL_WAVE_LDS_SYNC();
        s = psd_recombine(al, ah);
    }
#pragma unroll 1
    for (int r = 26; r < 30; r++) dense_round(r, true);
    return s;
}

}  // namespace gl355
