// The Poseidon permutation over Goldilocks, one state per lane (12 x u64 in VGPRs): poseidon_rounds.cuh's S-boxes and dense MDS layer for the
// 4 + 4 full rounds, the 22 partial rounds in blocks of three on the tables of poseidon_b3tables.h, and the sponge state.  Included by the units
// that run psd_permute or psd_partial_rounds_b3 (the hash kernels, the VALU probe, the test hook): it DEFINES the two block tables in every unit
// that includes it (they are not const, see below, so the compiler keeps them).  A unit that only runs dense rounds includes poseidon_rounds.cuh.
#pragma once
#include "poseidon_rounds.cuh"

namespace gl355 {

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
