// The round pieces of the Poseidon permutation over Goldilocks (width 12, x^7, 4 + 22 + 4 rounds) for gfx950 that every form shares: the round
// constants PSD_ALL_RC (read through the scalar cache at a uniform index), the S-boxes, the two ways a row's accumulators become a u64
// (psd_recombine; psd_chain_start / psd_fold) and the dense MDS layer of the one-state-per-lane form.  poseidon.cuh builds the permutation on
// it; the units that only run dense rounds (quotient.hip's PoseidonGate, the witness tape and poseidon_lanes.cuh's lane round) stop here.
//
// Replaces plonky2::hash::poseidon::{Poseidon::poseidon, PoseidonPermutation::permute}, reached from
// the reference at src/plonky2_semaphore/access_set.rs:67, signal.rs:35 and inside every Merkle
// build.  Parameters and round structure: src/plonky2_verifier/chip/plonk/gates/poseidon.rs:26-322
// (constants), :450-486 (MDS row), :504-589 and :634-686 (fast partial rounds).  The tables are
// written by tools/gen_poseidon_tables.py.
#pragma once
#include "gl_field.cuh"
#if GL_MUL_VARIANT != 1
#error "poseidon_rounds.cuh is written on the inline-asm product and its lock-step groups: GL_MUL_VARIANT 1"
#endif

#define PSD_TABLE_QUAL __device__ __constant__ const
#include "poseidon_tables.h"

namespace gl355 {

// x^7 = (x x^2)(x^2 x^2): x^3 and x^4 go through gl_mul_multi, whose products fill each other's carry wait states (round 5)
GL_DEV uint64_t psd_sbox(uint64_t x) {
    const uint64_t x2 = gl_sqr(x);
    const uint64_t a[2] = {x, x2}, b[2] = {x2, x2};
    uint64_t r[2];
    gl_mul_multi<2>(a, b, r);
    return gl_mul(r[0], r[1]);
}

// al + ah * 2^32  ->  u64 representative, for two INDEPENDENT accumulators whose top word ah1 = ah >> 32 satisfies ah1 + 1 < 2^32: the rows of the
// 16-lane permutation (poseidon_lanes.cuh) and of the witness tape, whose chains run side by side (al, ah < 2^44).  The one-state-per-lane
// permutation below chains its rows instead (psd_chain_start / psd_fold) and does not come here.
// = al0 + (al1 + ah0) 2^32 + ah1 2^64: one 32-bit add with carry into the top word, then top * EPS with the carry-out repaid.
GL_DEV uint64_t psd_recombine(uint64_t al, uint64_t ah) {
    uint32_t t1 = (uint32_t)(al >> 32), top;     // t1 is updated in place: (al0, t1) stays the register pair of al
    asm("v_add_co_u32_e32 %0, vcc, %0, %2\n\t" GL_HAZARD_NOP "v_addc_co_u32_e32 %1, vcc, 0, %3, vcc"
        : "+v"(t1), "=v"(top) : "v"((uint32_t)ah), "v"((uint32_t)(ah >> 32)) : "vcc");
    return gl_dev_add_mul_eps(((uint64_t)t1 << 32) | (uint32_t)al, top);
}

// the S-boxes of a full round, four at once: every phase is four products wide, no wait states at all (against two at once: -4 % at one wave per
// SIMD, nothing at full occupancy)
GL_DEV void psd_sbox4(uint64_t& x0, uint64_t& x1, uint64_t& x2, uint64_t& x3) {
    const uint64_t a[4] = {x0, x1, x2, x3};
    uint64_t sq[4], c3[4], c4[4], o[4];
    gl_mul_multi<4>(a, a, sq);
    gl_mul_multi<4>(a, sq, c3);
    gl_mul_multi<4>(sq, sq, c4);
    gl_mul_multi<4>(c3, c4, o);
    x0 = o[0]; x1 = o[1]; x2 = o[2]; x3 = o[3];
}
// The CHAINED row (docs/history/carry_tails.md): a row's low chain al = c_lo + sum coef lo_j runs first and its high chain starts from the ONE 32-bit
// word (al >> 32) + c_hi, zero-extended, so ah' = start + sum coef hi_j already holds the low chain's overflow and the row's value is
// al_0 + ah' 2^32 -- nothing with a carry joins the chains (psd_recombine spends v_add_co, v_addc on that; the start word costs a plain add and a
// move, the pair (al_0, ah'_0) a move into al's dead high register).  Precondition: c_hi + (worst al >> 32) < 2^32.  Dense rows: al >> 32 <= 264
// (the row sum) under a largest published c_hi of 0xfeed4db6; block rows: tightest at block 5, row 12, c_hi = 0xfd1e3e36 under a worst carry of
// 13 098 586, room 35 251 056.  tools/gen_poseidon_tables.py asserts it for every row it emits, tests/test_poseidon_row_chain.py restates it.
// Bounds: ah' < 2^44 + 2^32 in dense rows, < 2^57 in block rows, so top = ah' >> 32 < 2^25 and top * EPS wraps at most once.
GL_DEV uint64_t psd_chain_start(uint64_t al, uint32_t c_hi) { return (uint64_t)((uint32_t)(al >> 32) + c_hi); }
// al_0 + ah' 2^32 -> u64 representative: top * EPS onto (al_0, ah'_0), the carry-out repaid
GL_DEV uint64_t psd_fold(uint64_t al, uint64_t ahp) {
    return gl_dev_add_mul_eps(((uint64_t)(uint32_t)ahp << 32) | (uint32_t)al, (uint32_t)(ahp >> 32));
}
// N folds in lock-step (the others' instructions are the wait states between a multiply-add and the select on its carry: see gl_mul_multi)
template <int N>
GL_DEV void psd_fold_multi(const uint64_t (&al)[N], const uint64_t (&ahp)[N], uint64_t (&out)[N]) {
    static_assert(N >= 3, "three or more: no wait states of their own");
    uint32_t m[N];
    uint64_t c[N], r[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint64_t x = ((uint64_t)(uint32_t)ahp[j] << 32) | (uint32_t)al[j];
        asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(r[j]), "=s"(c[j]) : "v"((uint32_t)(ahp[j] >> 32)), "v"(x));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(m[j]) : "s"(c[j]));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = r[j] + (uint64_t)m[j];
}

// Full MDS layer, plus the NEXT round's constants.  Row r: sum_i s[(i+r)%12] * CIRC[i] + 8*s[0] (r == 0) + rc[r].  The entries
// are < 64, so the 32-bit halves are accumulated separately in u64 (12 * 41 * 2^32 + 2^32 < 2^43: no overflow) with
// v_mad_u64_u32 and folded once per row; the low half of the (canonical) round constant is the initial addend of the low
// chain (a scalar operand), the high half goes into the high chain's start word (psd_chain_start: one 32-bit add per row).
//
// Each chain is written out as 12 multiply-adds: left to itself the compiler re-associates the sums (chains started at 0
// and joined with extra 64-bit adds) and turns the entries 16 and 2 into shift-adds that need the 32-bit half zero-extended
// into a register pair first: 382-445 vector instructions per layer instead of 24 * 12 + 5 * 12 = 348.
#define PSD_MDS_CHAIN(C0)                                                                                  \
    "v_mad_u64_u32 %0, %1, %2, " #C0 ", %14\n\tv_mad_u64_u32 %0, %1, %3, 15, %0\n\tv_mad_u64_u32 %0, %1, %4, 41, %0\n\t" \
    "v_mad_u64_u32 %0, %1, %5, 16, %0\n\tv_mad_u64_u32 %0, %1, %6, 2, %0\n\tv_mad_u64_u32 %0, %1, %7, 28, %0\n\t"      \
    "v_mad_u64_u32 %0, %1, %8, 13, %0\n\tv_mad_u64_u32 %0, %1, %9, 13, %0\n\tv_mad_u64_u32 %0, %1, %10, 39, %0\n\t"    \
    "v_mad_u64_u32 %0, %1, %11, 18, %0\n\tv_mad_u64_u32 %0, %1, %12, 34, %0\n\tv_mad_u64_u32 %0, %1, %13, 20, %0"
// START: the chain's initial addend is a scalar pair (the low chain: the constant's low half) or a register pair (the high chain: psd_chain_start)
template <int R, bool VSTART, class A>
GL_DEV uint64_t psd_mds_chain(const uint32_t (&x)[12], A addend) {
    uint64_t acc, unused;
#define PSD_X(i) "v"(x[((i) + R) % 12])
#define PSD_MDS_ASM(C0, START)                                                                                                      \
    asm(PSD_MDS_CHAIN(C0) : "=&v"(acc), "=&s"(unused) : PSD_X(0), PSD_X(1), PSD_X(2), PSD_X(3), PSD_X(4), PSD_X(5), PSD_X(6), PSD_X(7), \
        PSD_X(8), PSD_X(9), PSD_X(10), PSD_X(11), START((uint64_t)addend))
    if constexpr (R == 0 && VSTART) PSD_MDS_ASM(25, "v");
    else if constexpr (R == 0) PSD_MDS_ASM(25, "s");
    else if constexpr (VSTART) PSD_MDS_ASM(17, "v");
    else PSD_MDS_ASM(17, "s");
#undef PSD_MDS_ASM
#undef PSD_X
    return acc;
}
template <int R, class RC>
GL_DEV void psd_mds_rows(uint64_t (&s)[12], const uint32_t (&lo)[12], const uint32_t (&hi)[12], RC rc) {
    if constexpr (R < 12) {
        // four rows at a time: the four low chains, the four high chains from their start words, then the folds in lock-step
        const uint64_t c0 = rc[R], c1 = rc[R + 1], c2 = rc[R + 2], c3 = rc[R + 3];
        const uint64_t al[4] = {psd_mds_chain<R, false>(lo, (uint32_t)c0), psd_mds_chain<R + 1, false>(lo, (uint32_t)c1),
                                psd_mds_chain<R + 2, false>(lo, (uint32_t)c2), psd_mds_chain<R + 3, false>(lo, (uint32_t)c3)};
        const uint64_t ah[4] = {psd_mds_chain<R, true>(hi, psd_chain_start(al[0], (uint32_t)(c0 >> 32))),
                                psd_mds_chain<R + 1, true>(hi, psd_chain_start(al[1], (uint32_t)(c1 >> 32))),
                                psd_mds_chain<R + 2, true>(hi, psd_chain_start(al[2], (uint32_t)(c2 >> 32))),
                                psd_mds_chain<R + 3, true>(hi, psd_chain_start(al[3], (uint32_t)(c3 >> 32)))};
        uint64_t o[4];
        __builtin_amdgcn_sched_barrier(0);
        psd_fold_multi<4>(al, ah, o);
        s[R] = o[0]; s[R + 1] = o[1]; s[R + 2] = o[2]; s[R + 3] = o[3];
        psd_mds_rows<R + 4, RC>(s, lo, hi, rc);
    }
}
// rc: 12 constants at a wave-uniform address (scalar loads); a pointer into PSD_ALL_RC, generic or in the constant address space
template <class RC>
GL_DEV void psd_mds(uint64_t (&s)[12], RC rc) {
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
    psd_mds_rows<0, RC>(s, lo, hi, rc);
}

}  // namespace gl355
