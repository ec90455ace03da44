// BN254-Poseidon over Goldilocks sponge states for gfx950: the reference's second hasher
// (src/plonky2_verifier/bn245_poseidon/native.rs:16-77, plonky2_config.rs:38-75; parameters constants.rs:5-404),
// the hash of the final wrap proof's Merkle trees and transcript (wrapper.rs:35-56 with OuterC).  SURVEY 8(f) N1.
//
// One sponge state (12 Goldilocks elements) per lane.  The permutation packs 3 elements per BN254 scalar
// (x0 + x1 p + x2 p^2, p = the Goldilocks prime), runs Poseidon t = 5 (8 full + 60 partial rounds, x^5, dense 5x5 MDS)
// and splits each of the 5 results back into its three low base-p digits.
//
// Fr arithmetic: nine 29-bit limbs in Montgomery form with radix 2^261 (bn254_f29.cuh; tables bn254_tables29.h, written by tools/gen_bn254_tables.py):
// products as carry-free column sums, INLINED, sums without carries or conditional subtractions (a value may grow to ~85 r over the 60 partial
// rounds; anything below 2^261 ~ 169 r is a legal operand of the next product), and values are canonicalised only when they leave the permutation.
// These kernels run at one wave per SIMD or less -- the small Merkle levels of a wrap proof are chains of dependent products -- and there the form is
// twice as fast per product as the 8 x 32-bit asm product of bn254_field.cuh (tools/ubench/ubench_mont29.hip with 256 blocks: 943 against 1 850
// clocks; round 4, docs/history/round_4.md).
#pragma once
#include "gl_field.cuh"
#include "bn254_f29.cuh"
#define BN254_TABLE_QUAL __device__ __constant__ const
#include "bn254_tables29.h"

namespace gl355 {

constexpr int FR_W = 9;                               // limbs of an fr8
typedef f29 fr8;                                      // (the name stays: "an Fr element of the hasher")
GL_DEV fr8 fr_mul(const fr8& a, const fr8& b) { return f29_mul_fr(a, b); }        // a's limbs < 2^30.6, b's < 2^29
GL_DEV fr8 fr_add(const fr8& a, const fr8& b) { return f29_norm(f29_add(a, b)); }  // limbs back under 2^29; the VALUE is left to grow
GL_DEV fr8 fr_pow5(const fr8& a) {
    const fr8 a2 = fr_mul(a, a), a4 = fr_mul(a2, a2);
    return fr_mul(a4, a);
}
GL_DEV fr8 fr_const(const uint32_t* p) { return f29_const(p); }
GL_DEV fr8 fr_zero() { fr8 r; for (int j = 0; j < FR_W; j++) r.l[j] = 0; return r; }
// a plain integer below 2^256 (four 64-bit words) into the Montgomery form, and a value (< 169 r) back to its canonical integer
GL_DEV fr8 fr_enter(const uint64_t a[4]) {
    u256 x;
#pragma unroll
    for (int i = 0; i < 4; i++) { x.l[2 * i] = (uint32_t)a[i]; x.l[2 * i + 1] = (uint32_t)(a[i] >> 32); }
    return fr_mul(f29_from_u256(x), fr_const(BN254F_R2));
}
GL_DEV void fr_leave(const fr8& xm, uint64_t a[4]) {
    fr8 one = fr_zero();
    one.l[0] = 1;
    fr8 x = fr_mul(xm, one);                          // x 2^-261: < r + 1, i.e. canonical or exactly r (for zero)
    uint32_t e = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) e |= x.l[j] ^ FR29_R[j];
    if (e == 0) x = fr_zero();
    const u256 w = f29_to_u256(x);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = (uint64_t)w.l[2 * i] | ((uint64_t)w.l[2 * i + 1] << 32);
}

// three Goldilocks elements -> x0 + x1 p + x2 p^2 (< 2^192, no reduction needed), then into Montgomery form
GL_DEV fr8 fr_encode3(uint64_t x0, uint64_t x1, uint64_t x2) {
    // a = x2; a = a * p + x1; a = a * p + x0 with p = 2^64 - 2^32 + 1: a * p = (a << 64) - (a << 32) + a
    uint64_t a[4] = {gl_canon(x2), 0, 0, 0};
    const uint64_t add[2] = {gl_canon(x1), gl_canon(x0)};
#pragma unroll
    for (int step = 0; step < 2; step++) {
        unsigned __int128 c = add[step];
        uint64_t o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            c += (unsigned __int128)a[i] * GL_P;
            o[i] = (uint64_t)c;
            c >>= 64;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) a[i] = o[i];
    }
    return fr_enter(a);
}

// canonical Fr value (leaves Montgomery form) -> its three low base-p digits
GL_DEV void fr_decode3(const fr8& xm, uint64_t out[3]) {
    uint64_t a[4];
    fr_leave(xm, a);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        // remainder: Horner over the 64-bit limbs with 2^64 = 2^32 - 1 (mod p)
        uint64_t r = gl_canon(a[3]);
#pragma unroll
        for (int i = 2; i >= 0; i--) r = gl_canon(gl_reduce128(a[i], r));
        out[d] = r;
        if (d == 2) break;
        // exact quotient (a - r) / p = (a - r) * p^-1 mod 2^256
        uint64_t s[4];
        unsigned __int128 br = (unsigned __int128)a[0] - r;
        s[0] = (uint64_t)br;
        uint64_t borrow = (uint64_t)(br >> 64) & 1;
#pragma unroll
        for (int i = 1; i < 4; i++) {
            br = (unsigned __int128)a[i] - borrow;
            s[i] = (uint64_t)br;
            borrow = (uint64_t)(br >> 64) & 1;
        }
        // p^-1 mod 2^256 as 64-bit limbs
        constexpr uint64_t PINV[4] = {0x0000000100000001ull, 0xffffffff00000000ull, 0xfffffffffffffffeull, 0x0000000100000000ull};
        uint64_t q[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            unsigned __int128 c = 0;
#pragma unroll
            for (int j = 0; i + j < 4; j++) {
                c += (unsigned __int128)s[i] * PINV[j] + q[i + j];
                q[i + j] = (uint64_t)c;
                c >>= 64;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) a[i] = q[i];
    }
}

// the Fr permutation (native.rs:45-62), values in Montgomery form and < 2r throughout.  The 8 full rounds follow the
// definition (constants, x^5 on every element, dense 5x5 MDS: 40 products each).  The 60 partial rounds use the derived
// sparse form (tools/gen_bn254_tables.py derive_fast, checked there against the definition): one pre-matrix (16 products),
// then per round x^5 on element 0 and 9 products instead of 25 -- 1 056 products per permutation instead of 2 000.
GL_DEV void bn254_full_round(fr8 (&s)[5], int rnd) {
#pragma unroll
    for (int i = 0; i < 5; i++) s[i] = fr_pow5(fr_add(s[i], fr_const(BN254F_RC[5 * rnd + i])));
    fr8 n[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        fr8 acc = fr_mul(s[0], fr_const(BN254F_MDS[5 * i]));
#pragma unroll
        for (int j = 1; j < 5; j++) acc = fr_add(acc, fr_mul(s[j], fr_const(BN254F_MDS[5 * i + j])));
        n[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) s[i] = n[i];
}
GL_DEV void bn254_permute_fr(fr8 (&s)[5]) {
#pragma unroll 1
    for (int rnd = 0; rnd < 4; rnd++) bn254_full_round(s, rnd);
    // ---- 60 partial rounds ----
#pragma unroll
    for (int i = 0; i < 5; i++) s[i] = fr_add(s[i], fr_const(BN254F_PART_FIRST[i]));
    {
        fr8 n[5];
        n[0] = s[0];
#pragma unroll
        for (int c = 1; c < 5; c++) {
            fr8 acc = fr_mul(s[1], fr_const(BN254F_PART_INIT[c - 1]));
#pragma unroll
            for (int r = 2; r < 5; r++) acc = fr_add(acc, fr_mul(s[r], fr_const(BN254F_PART_INIT[(r - 1) * 4 + (c - 1)])));
            n[c] = acc;
        }
#pragma unroll
        for (int i = 0; i < 5; i++) s[i] = n[i];
    }
#pragma unroll 1
    for (int r = 0; r < 60; r++) {
        fr8 s0 = fr_pow5(s[0]);
        if (r < 59) s0 = fr_add(s0, fr_const(BN254F_PART_POST[r]));
        fr8 d = fr_mul(s0, fr_const(BN254F_PART_M00[0]));
#pragma unroll
        for (int i = 1; i < 5; i++) {
            d = fr_add(d, fr_mul(s[i], fr_const(BN254F_PART_WHAT[4 * r + (i - 1)])));
            s[i] = fr_add(s[i], fr_mul(s0, fr_const(BN254F_PART_VS[4 * r + (i - 1)])));
        }
        s[0] = d;
    }
#pragma unroll 1
    for (int rnd = 64; rnd < 68; rnd++) bn254_full_round(s, rnd);
}

// Bn254PoseidonPermutation::permute on the 12-element sponge state (plonky2_config.rs:38-55)
GL_DEV void bn254_permute(uint64_t (&s)[12]) {
    fr8 st[5];
#pragma unroll
    for (int i = 0; i < 4; i++) st[i] = fr_encode3(s[3 * i], s[3 * i + 1], s[3 * i + 2]);
    st[4] = fr_zero();
    bn254_permute_fr(st);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint64_t d[3];
        fr_decode3(st[i], d);
        s[3 * i] = d[0]; s[3 * i + 1] = d[1]; s[3 * i + 2] = d[2];
    }
}

}  // namespace gl355
