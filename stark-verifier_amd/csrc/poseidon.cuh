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

// al + ah * 2^32  ->  u64 representative, for accumulators whose top word ah1 = ah >> 32 satisfies ah1 + 1 < 2^32: the two chains of an MDS row
// (al, ah < 2^44) and the dot products of a block of three partial rounds (coefficients summing to < 2^24 times 32-bit halves plus a 32-bit constant:
// al, ah < 2^56, ah1 < 2^24; the bound is asserted on the generated table by tools/gen_poseidon_tables.py and tests/test_poseidon_b3_tables.py).
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
// N recombinations in lock-step (the two carry steps of one fill the wait states of the others: see gl_mul_multi)
template <int N>
GL_DEV void psd_recombine_multi(const uint64_t (&al)[N], const uint64_t (&ah)[N], uint64_t (&out)[N]) {
    static_assert(N >= 3, "three or more: no wait states of their own");
    uint32_t t1[N], top[N], m[N];
    uint64_t c[N], r[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_add_co_u32_e64 %0, %1, %2, %3" : "=v"(t1[j]), "=s"(c[j]) : "v"((uint32_t)(al[j] >> 32)), "v"((uint32_t)ah[j]));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_addc_co_u32_e64 %0, %1, 0, %2, %1" : "=v"(top[j]), "+s"(c[j]) : "v"((uint32_t)(ah[j] >> 32)));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint64_t x = ((uint64_t)t1[j] << 32) | (uint32_t)al[j];
        asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(r[j]), "=s"(c[j]) : "v"(top[j]), "v"(x));
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
// v_mad_u64_u32 and recombined once per row; the two halves of the (canonical) round constant are the initial addends of
// the two chains (scalar operands), so adding the constants costs no vector instruction.
//
// Each chain is written out as 12 multiply-adds: left to itself the compiler re-associates the sums (chains started at 0
// and joined with extra 64-bit adds) and turns the entries 16 and 2 into shift-adds that need the 32-bit half zero-extended
// into a register pair first: 382-445 vector instructions per layer instead of 24 * 12 + 5 * 12 = 348.
#define PSD_MDS_CHAIN(C0)                                                                                  \
    "v_mad_u64_u32 %0, %1, %2, " #C0 ", %14\n\tv_mad_u64_u32 %0, %1, %3, 15, %0\n\tv_mad_u64_u32 %0, %1, %4, 41, %0\n\t" \
    "v_mad_u64_u32 %0, %1, %5, 16, %0\n\tv_mad_u64_u32 %0, %1, %6, 2, %0\n\tv_mad_u64_u32 %0, %1, %7, 28, %0\n\t"      \
    "v_mad_u64_u32 %0, %1, %8, 13, %0\n\tv_mad_u64_u32 %0, %1, %9, 13, %0\n\tv_mad_u64_u32 %0, %1, %10, 39, %0\n\t"    \
    "v_mad_u64_u32 %0, %1, %11, 18, %0\n\tv_mad_u64_u32 %0, %1, %12, 34, %0\n\tv_mad_u64_u32 %0, %1, %13, 20, %0"
template <int R>
GL_DEV uint64_t psd_mds_chain(const uint32_t (&x)[12], uint64_t addend) {
    uint64_t acc, unused;
#define PSD_X(i) "v"(x[((i) + R) % 12])
    if constexpr (R == 0)
        asm(PSD_MDS_CHAIN(25) : "=&v"(acc), "=&s"(unused) : PSD_X(0), PSD_X(1), PSD_X(2), PSD_X(3), PSD_X(4), PSD_X(5), PSD_X(6),
            PSD_X(7), PSD_X(8), PSD_X(9), PSD_X(10), PSD_X(11), "s"(addend));
    else
        asm(PSD_MDS_CHAIN(17) : "=&v"(acc), "=&s"(unused) : PSD_X(0), PSD_X(1), PSD_X(2), PSD_X(3), PSD_X(4), PSD_X(5), PSD_X(6),
            PSD_X(7), PSD_X(8), PSD_X(9), PSD_X(10), PSD_X(11), "s"(addend));
#undef PSD_X
    return acc;
}
template <int R, class RC>
GL_DEV void psd_mds_rows(uint64_t (&s)[12], const uint32_t (&lo)[12], const uint32_t (&hi)[12], RC rc) {
    if constexpr (R < 12) {
        // four rows at a time: eight chains, then their recombinations in lock-step
        const uint64_t c0 = rc[R], c1 = rc[R + 1], c2 = rc[R + 2], c3 = rc[R + 3];
        const uint64_t al[4] = {psd_mds_chain<R>(lo, (uint32_t)c0), psd_mds_chain<R + 1>(lo, (uint32_t)c1), psd_mds_chain<R + 2>(lo, (uint32_t)c2),
                                psd_mds_chain<R + 3>(lo, (uint32_t)c3)};
        const uint64_t ah[4] = {psd_mds_chain<R>(hi, c0 >> 32), psd_mds_chain<R + 1>(hi, c1 >> 32), psd_mds_chain<R + 2>(hi, c2 >> 32),
                                psd_mds_chain<R + 3>(hi, c3 >> 32)};
        uint64_t o[4];
        __builtin_amdgcn_sched_barrier(0);
        psd_recombine_multi<4>(al, ah, o);
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
// the two 32-bit halves the state already lives in: two v_mad_u64_u32 into two accumulators that start from the halves of the additive constant and
// stay below 2^56 (psd_recombine's contract with 2^8 to spare; asserted on the generated table by tests/test_poseidon_b3_tables.py).  Nothing is split
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
// one term: the coefficient c (an SGPR, the one constant-bus operand of both multiply-adds) times the halves of v, which are the registers of v
// themselves; the carry-out pair is never read.  Written out: in C the compiler zero-extends each half into a register pair of its own.
GL_DEV void psd_b3_term(uint64_t& lo, uint64_t& hi, uint32_t c, uint64_t v) {
    uint64_t unused;
    asm("v_mad_u64_u32 %0, %2, %3, %4, %0\n\tv_mad_u64_u32 %1, %2, %3, %5, %1"
        : "+v"(lo), "+v"(hi), "=&s"(unused) : "s"(c), "v"((uint32_t)v), "v"((uint32_t)(v >> 32)));
}
// five terms in one statement (the compiler puts a wait state between two statements that write scalar pairs)
GL_DEV void psd_b3_terms5(uint64_t& lo, uint64_t& hi, const uint32_t* c, const uint64_t* v) {
    uint64_t unused;
#define PSD_V(i) "v"((uint32_t)v[i]), "v"((uint32_t)(v[i] >> 32))
    asm("v_mad_u64_u32 %0, %2, %3, %8, %0\n\tv_mad_u64_u32 %1, %2, %3, %9, %1\n\t"
        "v_mad_u64_u32 %0, %2, %4, %10, %0\n\tv_mad_u64_u32 %1, %2, %4, %11, %1\n\t"
        "v_mad_u64_u32 %0, %2, %5, %12, %0\n\tv_mad_u64_u32 %1, %2, %5, %13, %1\n\t"
        "v_mad_u64_u32 %0, %2, %6, %14, %0\n\tv_mad_u64_u32 %1, %2, %6, %15, %1\n\t"
        "v_mad_u64_u32 %0, %2, %7, %16, %0\n\tv_mad_u64_u32 %1, %2, %7, %17, %1"
        : "+v"(lo), "+v"(hi), "=&s"(unused)
        : "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]), PSD_V(0), PSD_V(1), PSD_V(2), PSD_V(3), PSD_V(4));
#undef PSD_V
}
// the first term of an output: the accumulators start from the additive constant's halves.  Inside the statement, so that the constant is read
// where the row's coefficients are (a C initialisation is copied to VGPRs right behind its scalar load: a wait of its own).
GL_DEV void psd_b3_term_first(uint64_t& lo, uint64_t& hi, uint32_t c, uint64_t v, const uint64_t (&add)[2]) {
    uint64_t unused;
    asm("v_mov_b64 %0, %6\n\tv_mov_b64 %1, %7\n\t"
        "v_mad_u64_u32 %0, %2, %3, %4, %0\n\tv_mad_u64_u32 %1, %2, %3, %5, %1"
        : "=&v"(lo), "=&v"(hi), "=&s"(unused) : "s"(c), "v"((uint32_t)v), "v"((uint32_t)(v >> 32)), "s"(add[0]), "s"(add[1]));
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
// -> (lo, hi): lo + hi 2^32 = add + sum_{t < 11} u[t + 1] w[t] + sum_{t < NX} x[t] w[11 + t] (the caller folds it).  k: this output's row (requested
// earlier); on return the NEXT output's row (NT_NEXT terms at `next`, additive constant at `add_next`), requested, unless NT_NEXT is 0.
template <int NX, int NT_NEXT>
GL_DEV void psd_b3_dot(const uint64_t (&u)[12], const uint64_t (&x)[3], PsdB3Row& k, psd_b3tab next, psd_b3add add_next, uint64_t& lo, uint64_t& hi) {
    const PsdB3Row cur = k;
    psd_b3_term_first(lo, hi, cur.w[0], u[1], cur.a);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NT_NEXT > 0) psd_b3_load<NT_NEXT>(k, next, add_next);
    __builtin_amdgcn_sched_barrier(0);
    psd_b3_terms5(lo, hi, &cur.w[1], &u[2]);
    psd_b3_terms5(lo, hi, &cur.w[6], &u[7]);
#pragma unroll
    for (int t = 0; t < NX; t++) psd_b3_term(lo, hi, cur.w[11 + t], x[t]);
    __builtin_amdgcn_sched_barrier(0);
}
// outgoing lanes R .. R + 3: eight accumulators, then their recombinations in lock-step (no wait states of their own)
template <int R>
GL_DEV void psd_b3_out(uint64_t (&o)[12], const uint64_t (&u)[12], const uint64_t (&x)[3], psd_b3tab mac, psd_b3add add, PsdB3Row& k) {
    if constexpr (R < 12) {
        constexpr int W = PSD_B3_ROW_WORDS;
        uint64_t al[4], ah[4], r[4];
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 3), add + 2 * (R + 3), al[0], ah[0]);
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 4), add + 2 * (R + 4), al[1], ah[1]);
        psd_b3_dot<3, 14>(u, x, k, mac + W * (R + 5), add + 2 * (R + 5), al[2], ah[2]);
        psd_b3_dot<3, (R + 3 < 11 ? 14 : 0)>(u, x, k, mac + W * (R + 6), add + 2 * (R + 6), al[3], ah[3]);
        psd_recombine_multi<4>(al, ah, r);
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
        x[1] = psd_sbox(psd_recombine(lo, hi));
        __builtin_amdgcn_sched_barrier(0);
        psd_b3_dot<2, 14>(s, x, k, mac + 2 * W, add + 4, lo, hi);
        x[2] = psd_sbox(psd_recombine(lo, hi));
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
