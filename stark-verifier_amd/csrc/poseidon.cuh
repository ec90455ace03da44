// Poseidon permutation over Goldilocks (width 12, x^7, 4 + 22 + 4 rounds) for gfx950: one state per
// lane, 12 x u64 in VGPRs, round constants read through the scalar cache (uniform index).
//
// Replaces plonky2::hash::poseidon::{Poseidon::poseidon, PoseidonPermutation::permute}, reached from
// the reference at src/plonky2_semaphore/access_set.rs:67, signal.rs:35 and inside every Merkle
// build.  Parameters and round structure: src/plonky2_verifier/chip/plonk/gates/poseidon.rs:26-322
// (constants), :450-486 (MDS row), :504-589 and :634-686 (fast partial rounds).  The fast-partial
// tables are derived by tools/gen_poseidon_tables.py and equal the reference's literals.
#pragma once
#include "gl_field.cuh"
#if GL_MUL_VARIANT != 1
#error "poseidon.cuh is written on the inline-asm product and its lock-step groups: GL_MUL_VARIANT 1"
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


// ---- the partial rounds in blocks of THREE on integer matrix powers ----------------------------------------------------------------------
// Only lane 0 meets the S-box in a partial round, so over a block of three rounds the state is a linear function of the state u that entered the
// block and of the block's S-box outputs x_0, x_1, x_2 (gates/poseidon.rs:504-589 factors the same linearity round by round).  With M the MDS matrix
// as INTEGERS, N = M with column 0 zeroed and m0 = column 0 of M (tools/gen_poseidon_tables.py has the algebra and a half-exact model):
//     x_0 = u_0^7,   y_k = (N^k u)[0] + sum_{i<k} (N^(k-1-i) m0)[0] x_i + g_k[0],   x_k = y_k^7   (k = 1, 2: lane 0 entering the block's next rounds)
//     s'  = N^3 u + sum_{i<3} (N^(2-i) m0) x_i + g_3                                              (the state leaving the block)
// Three rounds of 6-bit entries give coefficients below 2^21 with row sums below 2^24 WITHOUT reduction mod p, so a term is the coefficient times
// the two 32-bit halves the state already lives in: two v_mad_u64_u32 into two accumulators, the low one from the low half of the additive constant
// (below 2^56; asserted on the generated table by tests/test_poseidon_b3_tables.py), the high one chained behind it from the start word (below 2^57:
// psd_chain_start above, tests/test_poseidon_row_chain.py).  Nothing is split
// and the constants are one 32-bit word each: 12 + 13 + 12 x 14 terms per block, the same for all seven blocks of rounds 4 .. 24; round 25 runs
// dense.  (Blocks of eleven on matrix powers reduced mod p, the form before this one, paid six multiply-adds per term for their 64-bit constants:
// docs/history/poseidon_b3.md.  Blocks of four no longer fit 64-bit accumulators.)
// (the tables are NOT const-qualified on the device: with the values visible the compiler strength-reduces the small ones into 64-bit shifts and
// adds on zero-extended register PAIRS and materialises the rest as 32-bit literals with a wait state each)
#undef PSD_TABLE_QUAL
#define PSD_TABLE_QUAL __device__ __constant__
#include "poseidon_b3tables.h"

typedef const __attribute__((address_space(4))) uint32_t* psd_b3tab;      // constant address space: wave-uniform reads become scalar loads
typedef const __attribute__((address_space(4))) uint64_t* psd_b3add;
// K terms of ONE chain in one statement (the compiler puts a wait state between two statements that write scalar pairs): each coefficient c[i] (an
// SGPR, the one constant-bus operand of its multiply-add) times the low or the high half of v[i], which is a register of v itself; the carry-out
// pair is never read.  Written out: in C the compiler zero-extends each half into a register pair of its own.
#define PSD_MA(C, V) "v_mad_u64_u32 %0, %1, %" #C ", %" #V ", %0"
#define PSD_C(i) "s"(c[i])
#define PSD_H(i) "v"(HI ? (uint32_t)(v[i] >> 32) : (uint32_t)v[i])
template <int K, bool HI>
GL_DEV void psd_b3_chain(uint64_t& acc, const uint32_t* c, const uint64_t* v) {
    static_assert(K == 1 || K == 2 || K == 3 || K == 10 || K == 11, "the statement sizes the rows are cut into");
    uint64_t unused;
    if constexpr (K == 1)
        asm(PSD_MA(2, 3) : "+v"(acc), "=&s"(unused) : PSD_C(0), PSD_H(0));
    else if constexpr (K == 2)
        asm(PSD_MA(2, 4) "\n\t" PSD_MA(3, 5) : "+v"(acc), "=&s"(unused) : PSD_C(0), PSD_C(1), PSD_H(0), PSD_H(1));
    else if constexpr (K == 3)
        asm(PSD_MA(2, 5) "\n\t" PSD_MA(3, 6) "\n\t" PSD_MA(4, 7) : "+v"(acc), "=&s"(unused) : PSD_C(0), PSD_C(1), PSD_C(2), PSD_H(0), PSD_H(1), PSD_H(2));
    else if constexpr (K == 10)
        asm(PSD_MA(2, 12) "\n\t" PSD_MA(3, 13) "\n\t" PSD_MA(4, 14) "\n\t" PSD_MA(5, 15) "\n\t" PSD_MA(6, 16) "\n\t"
            PSD_MA(7, 17) "\n\t" PSD_MA(8, 18) "\n\t" PSD_MA(9, 19) "\n\t" PSD_MA(10, 20) "\n\t" PSD_MA(11, 21)
            : "+v"(acc), "=&s"(unused)
            : PSD_C(0), PSD_C(1), PSD_C(2), PSD_C(3), PSD_C(4), PSD_C(5), PSD_C(6), PSD_C(7), PSD_C(8), PSD_C(9),
              PSD_H(0), PSD_H(1), PSD_H(2), PSD_H(3), PSD_H(4), PSD_H(5), PSD_H(6), PSD_H(7), PSD_H(8), PSD_H(9));
    else
        asm(PSD_MA(2, 13) "\n\t" PSD_MA(3, 14) "\n\t" PSD_MA(4, 15) "\n\t" PSD_MA(5, 16) "\n\t" PSD_MA(6, 17) "\n\t" PSD_MA(7, 18) "\n\t"
            PSD_MA(8, 19) "\n\t" PSD_MA(9, 20) "\n\t" PSD_MA(10, 21) "\n\t" PSD_MA(11, 22) "\n\t" PSD_MA(12, 23)
            : "+v"(acc), "=&s"(unused)
            : PSD_C(0), PSD_C(1), PSD_C(2), PSD_C(3), PSD_C(4), PSD_C(5), PSD_C(6), PSD_C(7), PSD_C(8), PSD_C(9), PSD_C(10),
              PSD_H(0), PSD_H(1), PSD_H(2), PSD_H(3), PSD_H(4), PSD_H(5), PSD_H(6), PSD_H(7), PSD_H(8), PSD_H(9), PSD_H(10));
}
#undef PSD_H
#undef PSD_C
#undef PSD_MA
// the first term of an output's low chain: the accumulator starts from the additive constant's low half.  Inside the statement, so that the
// constant is read where the row's coefficients are (a C initialisation is copied to VGPRs right behind its scalar load: a wait of its own).
GL_DEV void psd_b3_first(uint64_t& lo, uint32_t c, uint64_t v, uint64_t add_lo) {
    uint64_t unused;
    asm("v_mov_b64 %0, %4\n\tv_mad_u64_u32 %0, %1, %2, %3, %0" : "=&v"(lo), "=&s"(unused) : "s"(c), "v"((uint32_t)v), "s"(add_lo));
}
// The table is consumed front to back, one row (= one output) per group of scalar loads.  Scalar loads return out of order, so the only wait is
// "all of them": a row's constants are therefore requested one row AHEAD -- the first term of an output waits for its row (requested while the
// previous output was being accumulated, or under an S-box), then the next row's loads are issued, then the remaining terms run under their
// latency.  The scheduling barriers pin that order; without them the scheduler either issues the loads of a whole block (252 SGPRs, spilled into
// VGPR lanes) or waits for each row right after requesting it (a lonely wave then sits through the scalar-cache latency 14 times per block).
struct PsdB3Row {
    uint32_t w[14];                 // the row's coefficients (12 or 13 of them for y_1, y_2: the rest is the row's zero padding and never loaded)
    uint64_t a[2];                  // the output's additive constant (low half, high half)
};
template <int NT>
GL_DEV void psd_b3_load(PsdB3Row& k, psd_b3tab c, psd_b3add add) {
#pragma unroll
    for (int i = 0; i < NT; i++) k.w[i] = c[i];
    k.a[0] = add[0]; k.a[1] = add[1];
}
// -> (lo, hi) of a chained row: lo_0 + hi 2^32 = add + sum_{t < 11} u[t + 1] w[t] + sum_{t < NX} x[t] w[11 + t] (the caller folds it): the low
// terms, the start word, then the high terms over the same scalar row.  k: this output's row (requested earlier); on return the NEXT output's row
// (NT_NEXT terms at `next`, additive constant at `add_next`), requested, unless NT_NEXT is 0.
template <int NX, int NT_NEXT>
GL_DEV void psd_b3_dot(const uint64_t (&u)[12], const uint64_t (&x)[3], PsdB3Row& k, psd_b3tab next, psd_b3add add_next, uint64_t& lo, uint64_t& hi) {
    const PsdB3Row cur = k;
    psd_b3_first(lo, cur.w[0], u[1], cur.a[0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NT_NEXT > 0) psd_b3_load<NT_NEXT>(k, next, add_next);
    __builtin_amdgcn_sched_barrier(0);
    psd_b3_chain<10, false>(lo, &cur.w[1], &u[2]);
    psd_b3_chain<NX, false>(lo, &cur.w[11], &x[0]);
    hi = psd_chain_start(lo, (uint32_t)cur.a[1]);
    psd_b3_chain<11, true>(hi, &cur.w[0], &u[1]);
    psd_b3_chain<NX, true>(hi, &cur.w[11], &x[0]);
    __builtin_amdgcn_sched_barrier(0);
}
// outgoing lanes R .. R + 3: four chained rows, then their folds in lock-step (no wait states of their own)
template <int R>
GL_DEV void psd_b3_out(uint64_t (&o)[12], const uint64_t (&u)[12], const uint64_t (&x)[3], psd_b3tab mac, psd_b3add add, PsdB3Row& k) {
    if constexpr (R < 12) {
        constexpr int W = PSD_B3_ROW_WORDS;
        uint64_t al[4], ah[4], r[4];
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 3), add + 2 * (R + 3), al[0], ah[0]);
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 4), add + 2 * (R + 4), al[1], ah[1]);
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 5), add + 2 * (R + 5), al[2], ah[2]);
        psd_b3_dot<3, (R + 3 < 11 ? 14 : 0)>(u, x, k, mac + W * (R + 6), add + 2 * (R + 6), al[3], ah[3]);
        psd_fold_multi<4>(al, ah, r);
        o[R] = r[0]; o[R + 1] = r[1]; o[R + 2] = r[2]; o[R + 3] = r[3];
        __builtin_amdgcn_sched_barrier(0);
        psd_b3_out<R + 4>(o, u, x, mac, add, k);
    }
}
// rounds 4 .. 25 on the state entering round 4 (its constants added; ANY twelve u64) -> the state entering round 26 (constants added)
GL_DEV void psd_partial_rounds_b3(uint64_t (&s)[12]) {
#pragma unroll 1
    for (int blk = 0; blk < PSD_B3_BLOCKS; blk++) {
        constexpr int W = PSD_B3_ROW_WORDS;
        psd_b3add add = (psd_b3add)PSD_B3_ADD + blk * 2 * 14;
        psd_b3tab mac = (psd_b3tab)PSD_B3_MAC;
        asm volatile("" : "+s"(mac), "+s"(add));      // re-read per block (hoisted out of this loop the table would sit in ~200 SGPRs), at immediate offsets
        PsdB3Row k;
        psd_b3_load<12>(k, mac, add);         // y_1's row, under the first S-box
        __builtin_amdgcn_sched_barrier(0);
        uint64_t x[3], o[12], lo, hi;
        x[0] = psd_sbox(s[0]);
        __builtin_amdgcn_sched_barrier(0);
        psd_b3_dot<1, 13>(s, x, k, mac + W, add + 2, lo, hi);
        x[1] = psd_sbox(psd_fold(lo, hi));
        __builtin_amdgcn_sched_barrier(0);
        psd_b3_dot<2, 14>(s, x, k, mac + 2 * W, add + 4, lo, hi);
        x[2] = psd_sbox(psd_fold(lo, hi));
        __builtin_amdgcn_sched_barrier(0);
        psd_b3_out<0>(o, s, x, mac, add, k);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = o[i];
    }
    // round 25, dense.  Its constants are read here: at a visible address the compiler loads them once per kernel and, in the leaf hasher, keeps
    // them in spilled SGPRs that every permutation reads back lane by lane
    psd_b3add rc26 = (psd_b3add)PSD_ALL_RC + 12 * 26;
    asm volatile("" : "+s"(rc26));
    s[0] = psd_sbox(s[0]);
    psd_mds(s, rc26);
}

// 30 rounds of (constants, S-box on every element [4 + 4 full rounds] or on element 0 [22 partial rounds], MDS); round r's MDS adds round
// r+1's constants (PSD_ALL_RC row 30 is zero).  The full rounds are dense (S-boxes, whole MDS layer), the partial rounds run in blocks of three,
// above (against the dense form for all 30 rounds: profiles/r01_poseidon_dense_vs_sparse.txt; against blocks of eleven: profiles/poseidon_b3.txt).
// Two rounds per iteration (4 + 4: always whole pairs), so the state ping-pongs between two register sets instead of being copied back at the
// loop edge.
constexpr int psd_rounds_per_iter = 2;
GL_DEV void psd_dense_rounds(uint64_t (&s)[12], int r0, int r1) {
#pragma unroll 1
    for (int r = r0; r < r1; r += psd_rounds_per_iter) {
#pragma unroll
        for (int h = 0; h < psd_rounds_per_iter; h++) {
#pragma unroll
            for (int i = 0; i < 12; i += 4) psd_sbox4(s[i], s[i + 1], s[i + 2], s[i + 3]);
            psd_mds(s, &PSD_ALL_RC[12 * (r + h + 1)]);
        }
    }
}
GL_DEV void psd_permute(uint64_t (&s)[12]) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_canonical(s[i], PSD_ALL_RC[i]);
    psd_dense_rounds(s, 0, 4);
    psd_partial_rounds_b3(s);
    psd_dense_rounds(s, 26, 30);
}

// digest of <= 4 elements is the elements themselves, zero padded (chip/merkle_proof_chip.rs:52-57);
// longer inputs go through the overwrite-mode sponge (chip/hasher_chip.rs:122-148).
struct PsdSponge {
    uint64_t s[12];
    GL_DEV void init() {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = 0;
    }
};

}  // namespace gl355
