// BN254 (halo2curves bn256) field arithmetic for the device: Fr and Fq elements as 8 x 32-bit limbs in Montgomery form (R = 2^256), CIOS on
// v_mad_u64_u32 (4 m < R for both primes, so products of operands < 2m stay < 2m without a final subtraction; sums and differences take one
// conditional subtraction of 2m).  Shared by the curve units (bn254_fr_fft.hip, bn254_msm.hip, bn254_kzg.hip) and the PLONK prover kernels (plonk_bn254.hip).
#pragma once
#include "gl355_internal.h"

#ifndef BN254C_QUAL
#define BN254C_QUAL __device__ __constant__ const
#endif
#include "bn254_curve_tables.h"
#include "bn254_addsub_asm.cuh"
#include "host_mont.h"

// gl355_bn254_g1_msm_prepare's handle (built in bn254_kzg.hip, read by bn254_msm.hip): the window multiples of a base set (device), see msm_table_build_kernel
struct gl355_msm_bases {
    gl355::Ctx* ctx;
    uint32_t* tab;              // [wps][n][16]
    uint64_t n;
    uint32_t c, wps;
};
namespace gl355 {

struct u256 { uint32_t l[8]; };
enum { F_R = 0, F_Q = 1 };

template <int F> GL_DEV const uint32_t* f_mod() { return F == F_Q ? BN254C_FQ_MOD : BN254C_FR_MOD; }
template <int F> GL_DEV const uint32_t* f_two_mod() { return F == F_Q ? BN254C_FQ_TWO_MOD : BN254C_FR_TWO_MOD; }
template <int F> GL_DEV const uint32_t* f_r2() { return F == F_Q ? BN254C_FQ_R2 : BN254C_FR_R2; }
template <int F> GL_DEV const uint32_t* f_one() { return F == F_Q ? BN254C_FQ_ONE : BN254C_FR_ONE; }

GL_DEV u256 u_const(const uint32_t* p) {
    u256 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = p[j];
    return r;
}
GL_DEV u256 u_zero() {
    u256 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = 0;
    return r;
}
GL_DEV bool u_is_zero(const u256& a) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) o |= a.l[j];
    return o == 0;
}
GL_DEV bool u_eq(const u256& a, const u256& b) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) o |= a.l[j] ^ b.l[j];
    return o == 0;
}
// a - m if a >= m else a
GL_DEV u256 u_cond_sub(const u256& a, const uint32_t* m) {
    uint32_t d[8];
    uint64_t br = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t v = (uint64_t)a.l[j] - m[j] - br;
        d[j] = (uint32_t)v;
        br = (v >> 32) & 1;
    }
    u256 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = br ? a.l[j] : d[j];
    return r;
}
// a * b * R^-1 (mod m), result < 2m for a, b < 2m
//
// One asm statement (bn254_mmul_asm.inc, written by tools/gen_mmul_asm.py, which explains the scheme): the CIOS product of a and b with the
// Montgomery reduction by M folded into each row, as independent multiply-adds against a bank of {t_j, 0} pairs + one carry chain per half-row:
// 128 v_mad_u64_u32 + 128 carry adds + 8 v_mul_lo, where the same loop compiled from C spends 128 + 118 64-bit adds + 268 moves.
#include "bn254_mmul_asm.inc"
template <int F>
__device__ __noinline__ u256 m_mul(u256 a, u256 b) {
    const uint32_t* M = f_mod<F>();
    const uint32_t n0 = F == F_Q ? BN254C_FQ_N0INV : BN254C_FR_N0INV;
    u256 r;
    uint32_t u8, mm;
    uint64_t sd;
    asm(GL355_MMUL_ASM_TEXT
        : [r0] "=v"(r.l[0]), [r1] "=v"(r.l[1]), [r2] "=v"(r.l[2]), [r3] "=v"(r.l[3]), [r4] "=v"(r.l[4]), [r5] "=v"(r.l[5]), [r6] "=v"(r.l[6]),
          [r7] "=v"(r.l[7]), [u8] "=&v"(u8), [mm] "=&v"(mm), [sd] "=&s"(sd)
        : [a0] "v"(a.l[0]), [a1] "v"(a.l[1]), [a2] "v"(a.l[2]), [a3] "v"(a.l[3]), [a4] "v"(a.l[4]), [a5] "v"(a.l[5]), [a6] "v"(a.l[6]),
          [a7] "v"(a.l[7]), [b0] "v"(b.l[0]), [b1] "v"(b.l[1]), [b2] "v"(b.l[2]), [b3] "v"(b.l[3]), [b4] "v"(b.l[4]), [b5] "v"(b.l[5]),
          [b6] "v"(b.l[6]), [b7] "v"(b.l[7]), [M0] "s"(M[0]), [M1] "s"(M[1]), [M2] "s"(M[2]), [M3] "s"(M[3]), [M4] "s"(M[4]), [M5] "s"(M[5]),
          [M6] "s"(M[6]), [M7] "s"(M[7]), [n0] "s"(n0)
        : GL355_MMUL_ASM_CLOBBERS);
    return r;
}
// Sums and differences (results < 2m for operands < 2m): the carry chains of bn254_addsub_asm.cuh
template <int F> GL_DEV u256 m_add(const u256& a, const u256& b) {
    const bn_limbs q = bn254_add_asm(a.l, b.l, f_two_mod<F>());
    u256 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = q.l[j];
    return r;
}
template <int F> GL_DEV u256 m_sub(const u256& a, const u256& b) {
    const uint32_t* tm = f_two_mod<F>();
    // a - b, plus 2m where that borrowed: a representative in [0, 2m) (every consumer either multiplies on or canonicalises)
    const bn_limbs q = bn254_sub_asm(a.l, b.l, tm);
    u256 d;
#pragma unroll
    for (int j = 0; j < 8; j++) d.l[j] = q.l[j];
    return d;
}
template <int F> GL_DEV u256 m_canon(const u256& a) { return u_cond_sub(a, f_mod<F>()); }       // < 2m -> < m
template <int F> GL_DEV bool m_is_zero(const u256& a) { return u_is_zero(m_canon<F>(a)); }
template <int F> GL_DEV bool m_eq(const u256& a, const u256& b) { return u_eq(m_canon<F>(a), m_canon<F>(b)); }
// any 256-bit integer -> Montgomery form (< 2m): 2^256 < 6m, so five conditional subtractions bring the input below m first
template <int F> GL_DEV u256 m_from_int(u256 a) {
#pragma unroll 1
    for (int k = 0; k < 5; k++) a = u_cond_sub(a, f_mod<F>());
    return m_mul<F>(a, u_const(f_r2<F>()));
}
template <int F> GL_DEV u256 m_to_int(const u256& a) {
    u256 one = u_zero();
    one.l[0] = 1;
    return m_canon<F>(m_mul<F>(a, one));
}
GL_DEV u256 load256(const uint64_t* p) {
    u256 r;
#pragma unroll
    for (int i = 0; i < 4; i++) { r.l[2 * i] = (uint32_t)p[i]; r.l[2 * i + 1] = (uint32_t)(p[i] >> 32); }
    return r;
}
GL_DEV void store256(uint64_t* p, const u256& a) {
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = (uint64_t)a.l[2 * i] | ((uint64_t)a.l[2 * i + 1] << 32);
}
template <int F> GL_DEV u256 m_pow_u64(u256 a, uint64_t e) {
    u256 r = u_const(f_one<F>());
    while (e) {
        if (e & 1) r = m_mul<F>(r, a);
        a = m_mul<F>(a, a);
        e >>= 1;
    }
    return r;
}
// a^(m-2): the inverse
template <int F> GL_DEV u256 m_inv(const u256& a) {
    const uint32_t* M = f_mod<F>();
    u256 r = u_const(f_one<F>());
#pragma unroll 1
    for (int i = 255; i >= 0; i--) {
        r = m_mul<F>(r, r);
        uint32_t w = M[i >> 5];
        if ((i >> 5) == 0) w -= 2;               // low limb of both primes is > 2: no borrow
        if ((w >> (i & 31)) & 1) r = m_mul<F>(r, a);
    }
    return r;
}


// A host scalar (host_mont.h's Fr) as a kernel argument: to_u256(x.l) hands over the Montgomery form, to_u256 of x.to_words the plain integer
inline u256 to_u256(const uint64_t w[4]) {
    u256 r;
    for (int i = 0; i < 4; i++) { r.l[2 * i] = (uint32_t)w[i]; r.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return r;
}

// ---- bn254_fr_fft.hip / bn254_msm.hip / bn254_kzg.hip: what the curve units call of each other, and the resident building blocks of the PLONK
// prover (plonk_bn254.hip)
int32_t bn254_fr_twiddles(Ctx* ctx, uint32_t log_n, bool inverse, uint64_t* tw /* n / 2 + 1 elements */);
int32_t bn254_fr_power_table(Ctx* ctx, const uint64_t base[4], const uint64_t f[4], uint64_t count, uint64_t* tab);
// the transforms on resident Montgomery data, n = 2^log_n values each (the index orders: bn254_fr_route.h)
int32_t bn254_fr_ntt_mont(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t scale_plain[4] /* or null */,
                          uint64_t* work /* n elements */);
int32_t bn254_fr_ntt_mont_coset_dif(Ctx* ctx, const uint64_t* in, uint64_t n_in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t shift_plain[4],
                                    uint64_t* btw /* n elements */, bool fill);
int32_t bn254_fr_ntt_mont_from_bitrev(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t* post /* or null */);
// `bases` (gl355_bn254_g1_msm_prepare over the same points, or null): the table of the points' window multiples -- every window's digits then fall into ONE
// set of buckets per scalar set (bn254_msm.hip, "shared buckets").
// max_bits: every scalar of the call is below 2^max_bits (256: no promise; a scalar on a non-identity base that breaks the promise further than the
// plan's digits can hold is GL355_E_INVALID_ARG, never a wrong sum).  Windows above that hold only zero digits: they are not built,
// sorted or reduced (range-check columns are 16-bit values, the arithmetic chip's operands 64-bit: 2 and 5 windows of 20 bits instead of 13)
int32_t bn254_msm_bits(gl355_ctx* h, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint32_t m, uint32_t max_bits, uint64_t* result,
                       const gl355_msm_bases* bases = nullptr, uint32_t* plan_out /* c, wps, one window, two-level sort */ = nullptr);
// in: 2^log_in values, out: n_out values of the 2^log_n-point transform, device arrays of plain integers; shift == nullptr: the plain transform
int32_t fr_ntt_run(Ctx* ctx, const uint64_t* in, uint32_t log_in, uint64_t* out, uint64_t n_out, uint32_t log_n, int32_t inverse, const uint64_t* shift);
// Q[i] = sum_{j > i} A[j] z^(j - i - 1), E = sum_j A[j] z^j on device arrays (see the division kernels of bn254_kzg.hip)
int32_t kzg_divide(Ctx* ctx, const uint64_t* A, uint64_t m, const Fr& z, int a_is_mont, uint64_t* Q, int q_plain, uint64_t* E_mont);
}  // namespace gl355
