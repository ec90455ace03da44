// Constraint / quotient batch evaluation for gfx950 (a10 of SURVEY.md 8).
//
// Replaces plonky2::plonk::prover::compute_quotient_polys ->
// vanishing_poly::eval_vanishing_poly_base_batch -> Gate::eval_unfiltered_base_batch (+ ZeroPolyOnCoset),
// reached from the reference through CircuitData::prove (src/plonky2_semaphore/access_set.rs:94,
// recursion.rs:168, wrapper.rs:55).  The formula is the one the reference's verifier re-evaluates at
// zeta: src/plonky2_verifier/chip/plonk/vanishing_poly.rs:18-153 (term order :110-123), gate filter
// chip/plonk/gates/mod.rs:87-132, quotient identity chip/plonk/plonk_verifier_chip.rs:174-210, and
// the gate evaluators chip/plonk/gates/*.rs (all 12 gate kinds of the dispatch table gates/mod.rs:141-196), and plonky2's
// CosetInterpolationGate as a thirteenth kind in kernel instances of its own (gate_coset_interpolation).
//
// One lane = one point x = 7*omega^i of the quotient coset (size n * 2^qdb).  The three committed
// oracles are column-major in bit-reversed row order, and lane t works on storage row t, so every
// one of the ~240 column reads per point is a perfectly coalesced 512-byte wave access; nothing is
// gathered except the 2 "next row" Z values.  All arithmetic is base field (the challenges alpha,
// beta, gamma are base-field elements, plonk_verifier_chip.rs:64-96).  The term list
//   [L0(x)(Z_c(x)-1)]_c || [prev*prod(num) - next*prod(den)]_{c,chunk} || [sum_g filter_g * constraint_{g,k}]_k
// is reduced with powers of each alpha on the fly, so no per-lane constraint array exists.
// Roofline: integer VALU (a PoseidonGate row costs about one permutation), not HBM.
#include "gl355_internal.h"
#include "poseidon_rounds.cuh"

namespace gl355 {

struct QuotArgs {
    gl355_circuit c;
    const uint64_t* cs;       // constants_sigmas LDE  [num_selectors + num_constants + routed][N]
    const uint64_t* wires;    // wires LDE             [num_wires (+salt)][N]
    const uint64_t* zs;       // Z + partial products  [num_challenges * (1 + num_pp) (+salt)][N]
    uint64_t lde_stride;      // N
    uint32_t qbits;           // log2 of the quotient domain
    const uint64_t* k_is;     // [routed]
    const uint64_t* xw_lo;    // omega_{Nq}^e two-level table
    const uint64_t* xw_hi;
    uint64_t zh_inv[16];      // 1 / (x^n - 1) for the 2^qdb classes of i mod 2^qdb
    uint64_t zh[16];          // x^n - 1
    uint64_t n_inv;           // 1/n
    uint64_t* out;            // [unit][num_challenges][Nq], storage (bit-reversed) order
    const uint64_t* alpha_pw; // alpha_{u,c}^k at [(u * num_challenges + c) * pw_stride + k], k < pw_stride (alpha_table_kernel)
    uint32_t pw_stride;
    // the lock-step units of one prover context (blockIdx.y): constants_sigmas is shared, wires / zs / out have unit strides,
    // every unit has its own challenges and public-input hash
    uint64_t wires_us, zs_us;
    uint64_t betas[GL355_MAX_UNITS * 4], gammas[GL355_MAX_UNITS * 4], pi_hash[GL355_MAX_UNITS * 4];
};

// alpha-power accumulation of the constraint stream: term k of the stream is weighted alpha_c^k.  The powers are the same for
// every lane, so they come from a table built once per launch (alpha_table_kernel) and read through the scalar cache
// (constant address space, wave-uniform index) instead of being multiplied along per lane -- one product per push and
// challenge instead of two.  NCH (the number of challenges) is a template parameter so that acc stays in registers (a
// run-time bound puts the array in scratch memory and every push() becomes scratch loads + stores).
typedef const __attribute__((address_space(4))) uint64_t* PwTable;
template <int NCH>
struct AlphaAcc {
    uint64_t acc[NCH];
    PwTable tab;
    uint32_t stride, idx;
    GL_DEV void init(const QuotArgs& a, uint32_t unit, uint32_t first = 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = 0;
        tab = (PwTable)(a.alpha_pw + (uint64_t)unit * NCH * a.pw_stride); stride = a.pw_stride; idx = first;
    }
    GL_DEV void push(uint64_t term) {
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = gl_add(acc[c], gl_mul(term, tab[c * stride + idx]));
        idx++;
    }
    GL_DEV void push_at(uint64_t term, uint32_t k) {       // term k of the stream, out of order
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = gl_add(acc[c], gl_mul(term, tab[c * stride + k]));
    }
};
// per-gate accumulation: sum_k alpha^(base+k) * c_k, later multiplied by the gate's filter.
//
// LAZILY REDUCED for two challenges (round 3): about 500 terms are pushed per point of the recursive circuit and a push was a modular
// product and a modular sum per challenge -- 40 of the kernel's ~76 VALU instructions per term.  Here a gate's sum is kept as three 64-bit
// columns (weights 1, 2^32, 2^64) with a 32-bit overflow count each; a push is four multiply-adds per challenge whose carry-outs
// are added into the counts -- 16 instructions for both challenges -- and the field value is formed once per gate (value()).
// The carry-outs live in scalar register pairs; gfx950 wants two wait states between a VALU write of a scalar register and the VALU read
// of it and the hazard recogniser does not look inside inline asm, so the two challenges' instructions are interleaved (every carry
// is consumed four instructions after it was produced).
template <int NCH>
struct LazyAcc : AlphaAcc<NCH> {
    GL_DEV uint64_t value(int c) const { return this->acc[c]; }
};
template <>
struct LazyAcc<2> {
    uint64_t A0[2], A1[2], A2[2];
    uint32_t k0[2], k1[2], k2[2];
    PwTable tab;
    uint32_t stride, idx;
    GL_DEV void init(const QuotArgs& a, uint32_t unit, uint32_t first = 0) {
#pragma unroll
        for (int c = 0; c < 2; c++) { A0[c] = A1[c] = A2[c] = 0; k0[c] = k1[c] = k2[c] = 0; }
        tab = (PwTable)(a.alpha_pw + (uint64_t)unit * 2 * a.pw_stride); stride = a.pw_stride; idx = first;
    }
    GL_DEV void push(uint64_t term) {
        const uint64_t ax = tab[idx], ay = tab[stride + idx];
        const uint32_t t0 = (uint32_t)term, t1 = (uint32_t)(term >> 32);
        uint64_t c0, c1, c2, c3;
        asm("v_mad_u64_u32 %0, %12, %16, %18, %0\n\t"
            "v_mad_u64_u32 %1, %13, %16, %20, %1\n\t"
            "v_mad_u64_u32 %2, %14, %16, %19, %2\n\t"
            "v_mad_u64_u32 %3, %15, %16, %21, %3\n\t"
            "v_addc_co_u32_e64 %6, vcc, 0, %6, %12\n\t"
            "v_addc_co_u32_e64 %7, vcc, 0, %7, %13\n\t"
            "v_addc_co_u32_e64 %8, vcc, 0, %8, %14\n\t"
            "v_addc_co_u32_e64 %9, vcc, 0, %9, %15\n\t"
            "v_mad_u64_u32 %2, %12, %17, %18, %2\n\t"
            "v_mad_u64_u32 %3, %13, %17, %20, %3\n\t"
            "v_mad_u64_u32 %4, %14, %17, %19, %4\n\t"
            "v_mad_u64_u32 %5, %15, %17, %21, %5\n\t"
            "v_addc_co_u32_e64 %8, vcc, 0, %8, %12\n\t"
            "v_addc_co_u32_e64 %9, vcc, 0, %9, %13\n\t"
            "v_addc_co_u32_e64 %10, vcc, 0, %10, %14\n\t"
            "v_addc_co_u32_e64 %11, vcc, 0, %11, %15"
            : "+v"(A0[0]), "+v"(A0[1]), "+v"(A1[0]), "+v"(A1[1]), "+v"(A2[0]), "+v"(A2[1]),          // 0..5
              "+v"(k0[0]), "+v"(k0[1]), "+v"(k1[0]), "+v"(k1[1]), "+v"(k2[0]), "+v"(k2[1]),          // 6..11
              "=&s"(c0), "=&s"(c1), "=&s"(c2), "=&s"(c3)                                                // 12..15
            : "v"(t0), "v"(t1),                                                                          // 16, 17
              "s"((uint32_t)ax), "s"((uint32_t)(ax >> 32)), "s"((uint32_t)ay), "s"((uint32_t)(ay >> 32)) // 18..21
            : "vcc");
        idx++;
    }
    // A0 + 2^32 A1 + 2^64 (A2 + k0) + 2^96 k1 + 2^128 k2  with  2^96 = -1, 2^128 = -2^32 (mod p)
    GL_DEV uint64_t value(int c) const {
        uint64_t r = gl_reduce128(A0[c], A2[c]);
        r = gl_add(r, gl_mul_2exp<32>(A1[c]));
        r = gl_add(r, gl_reduce128(0, k0[c]));
        r = gl_sub(r, k1[c]);
        return gl_sub(r, (uint64_t)k2[c] << 32);
    }
};
template <int NCH>
using GateAccT = LazyAcc<NCH>;

// alpha_c^k for k < stride, one thread per entry (square-and-multiply over the bits of k)
struct AlphaTabArgs { uint64_t alphas[GL355_MAX_UNITS * 4]; uint32_t nch, stride; uint64_t* out; };
__global__ void alpha_table_kernel(AlphaTabArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
    if (k >= a.stride) return;
    for (uint32_t c = 0; c < a.nch; c++) a.out[((uint64_t)u * a.nch + c) * a.stride + k] = gl_canon(gl_pow(a.alphas[u * 4 + c], k));
}

// a point's wire row: column j of the wires LDE at this lane's row (global memory), or of the LDS copy of the row (STAGE variant)
struct WireSrc { const uint64_t* p; uint64_t stride, idx, cs_stride; };    // cs_stride: of the constants_sigmas oracle (global memory)
#define WIRE(j) (w.p[(uint64_t)(j) * w.stride + w.idx])
#define CONST(j) (a.cs[(uint64_t)(j) * w.cs_stride + t])

// GROUPED COLUMN READS.  A column value is an Infinity-Cache hit (~545 clk idle) and with three waves per SIMD a read that is
// waited for on the spot is a bubble nobody fills, so the evaluators request their columns K at a time: the K loads are issued
// back to back into a register array (no wait, no branch between them) and the evaluator consumes from the registers -- one
// round trip per group.  A run-time loop runs over groups; the short last group CLAMPS its column indices to `last` (the last
// column the evaluator owns, so never past the oracle) and the surplus registers are ignored.
constexpr int QG = 8;
template <int K>
GL_DEV void wire_group(const WireSrc& w, uint32_t first, uint32_t last, uint64_t* v) {
#pragma unroll
    for (int i = 0; i < K; i++) { const uint32_t j = first + i; v[i] = WIRE(j < last ? j : last); }
}
template <int K>
GL_DEV void const_group(const QuotArgs& a, const WireSrc& w, uint64_t t, uint32_t first, uint32_t last, uint64_t* v) {
#pragma unroll
    for (int i = 0; i < K; i++) { const uint32_t j = first + i; v[i] = CONST(j < last ? j : last); }
}

// PoseidonGate: 123 constraints (gates/poseidon.rs:592-698); wire layout :329-380.  The first PSD_AHEAD S-box-input wires of a
// full round are requested one round ahead (in flight over the S-boxes and the MDS layer of the round before; all twelve do
// not fit next to the state at three waves), the rest in one group when the round starts; a partial round's wire four rounds ahead.
constexpr int PSD_AHEAD = 6;
template <class GateAcc>
GL_DEV void psd_round_wires(const WireSrc& w, GateAcc& g, uint64_t* s, uint64_t* sin, uint32_t first) {
    constexpr int PF = PSD_AHEAD;
    if constexpr (PF < 12) wire_group<12 - PF>(w, first + PF, first + 11, sin + PF);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        g.push(gl_sub(s[i], sin[i]));
        s[i] = sin[i];
    }
}
template <class GateAcc>
GL_DEV void gate_poseidon(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g) {
    constexpr int PF = PSD_AHEAD;
    uint64_t s[12], sin[12], pin[4];
    {
        uint64_t in[12], sd[5];                     // inputs 0..11, swap 24, delta 25..28: one group
        wire_group<12>(w, 0, 11, in);
        wire_group<5>(w, 24, 28, sd);
        const uint64_t swap = sd[0];
        g.push(gl_sub(gl_mul(swap, swap), swap));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t lhs = in[i], rhs = in[i + 4], delta = sd[1 + i];
            g.push(gl_sub(gl_mul(swap, gl_sub(rhs, lhs)), delta));
            s[i] = gl_add(lhs, delta);
            s[i + 4] = gl_sub(rhs, delta);
        }
#pragma unroll
        for (int i = 8; i < 12; i++) s[i] = in[i];
    }
    // every MDS layer also adds the NEXT round's constants (psd_mds; row 30 of the table is zero), so s is "state + constants",
    // the quantity the S-box-input wires are constrained to, whenever a round starts
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_canonical(s[i], PSD_ALL_RC[i]);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
        if (r != 0) psd_round_wires(w, g, s, sin, 29 + 12 * (r - 1));
        if (r < 3) wire_group<PF>(w, 29 + 12 * r, 64, sin);      // round r + 1's
        else wire_group<4>(w, 65, 86, pin);                      // the first four partial rounds'
#pragma unroll
        for (int i = 0; i < 12; i += 4) psd_sbox4(s[i], s[i + 1], s[i + 2], s[i + 3]);       // four S-boxes in lock-step (poseidon_rounds.cuh)
        psd_mds(s, &PSD_ALL_RC[12 * (r + 1)]);
    }
    // partial rounds in the dense form: the S-box input of round r is s[0] + RC[4+r][0] in either form, so the
    // 22 constraints (and the state handed to the closing full rounds) are the same polynomials in the wires
    // as in the reference's sparse formulation (gates/poseidon.rs:652-673), at fewer VALU cycles
#pragma unroll 1
    for (int r0 = 0; r0 < 24; r0 += 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (r0 + i < 22) {
                const uint64_t sin0 = pin[i];
                pin[i] = WIRE(r0 + i + 4 < 22 ? 65 + r0 + i + 4 : 86);       // round r + 4's (clamped: never used past round 21)
                g.push(gl_sub(s[0], sin0));
                s[0] = psd_sbox(sin0);
                if (r0 + i == 21) wire_group<PF>(w, 87, 98, sin);            // the first closing full round's
                psd_mds(s, &PSD_ALL_RC[12 * (5 + r0 + i)]);
            }
        }
    }
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
        psd_round_wires(w, g, s, sin, 87 + 12 * r);
        if (r < 3) wire_group<PF>(w, 87 + 12 * (r + 1), 134, sin);
        else wire_group<PF>(w, 12, 23, sin);                     // the first PF outputs; the other 12 - PF are read behind the loop
#pragma unroll
        for (int i = 0; i < 12; i += 4) psd_sbox4(s[i], s[i + 1], s[i + 2], s[i + 3]);
        psd_mds(s, &PSD_ALL_RC[12 * (27 + r)]);
    }
    if constexpr (PF < 12) wire_group<12 - PF>(w, 12 + PF, 23, sin + PF);
#pragma unroll
    for (int i = 0; i < 12; i++) g.push(gl_sub(s[i], sin[i]));
}

// BaseSumGate<2>{num_limbs}: sum_i limb_i 2^i - sum ; limb (limb - 1)   (gates/base_sum.rs:37-60)
template <class GateAcc>
GL_DEV void gate_base_sum(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t num_limbs) {
    const uint64_t sum = WIRE(0);
    const uint32_t groups = (num_limbs + QG - 1) / QG;
    uint64_t acc = 0;
    for (uint32_t gr = groups; gr-- > 0;) {
        uint64_t v[QG];
        wire_group<QG>(w, 1 + gr * QG, num_limbs, v);
#pragma unroll
        for (int i = QG - 1; i >= 0; i--)
            if (gr * QG + i < num_limbs) acc = gl_add(gl_add(acc, acc), v[i]);
    }
    g.push(gl_sub(acc, sum));
    for (uint32_t gr = 0; gr < groups; gr++) {
        uint64_t v[QG];
        wire_group<QG>(w, 1 + gr * QG, num_limbs, v);
#pragma unroll
        for (int i = 0; i < QG; i++)
            if (gr * QG + i < num_limbs) g.push(gl_sub(gl_mul(v[i], v[i]), v[i]));
    }
}
// ConstantGate{n}: const_i - wire_i   (gates/constant.rs:31-36); gate constants follow the selectors
template <class GateAcc>
GL_DEV void gate_constant(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t n) {
    for (uint32_t i0 = 0; i0 < n; i0 += 4) {
        uint64_t c[4], v[4];
        const_group<4>(a, w, t, a.c.num_selectors + i0, a.c.num_selectors + n - 1, c);
        wire_group<4>(w, i0, n - 1, v);
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i0 + i < n) g.push(gl_sub(c[i], v[i]));
    }
}
// PublicInputGate: wire_i - pi_hash_i   (gates/public_input.rs:32-39)
template <class GateAcc>
GL_DEV void gate_public_input(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t unit) {
    uint64_t v[4];
    wire_group<4>(w, 0, 3, v);
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) g.push(gl_sub(v[i], a.pi_hash[unit * 4 + i]));
}
// ArithmeticGate{num_ops}: out - (c0 m0 m1 + c1 addend)   (gates/arithmetic.rs:47-68)
template <class GateAcc>
GL_DEV void gate_arithmetic(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t num_ops) {
    const uint64_t c0 = CONST(a.c.num_selectors), c1 = CONST(a.c.num_selectors + 1);
    for (uint32_t i0 = 0; i0 < num_ops; i0 += 2) {           // two operations = one group
        uint64_t v[8];
        wire_group<8>(w, 4 * i0, 4 * num_ops - 1, v);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (i0 + i < num_ops) {
                const uint64_t m0 = v[4 * i], m1 = v[4 * i + 1], ad = v[4 * i + 2], out = v[4 * i + 3];
                g.push(gl_sub(out, gl_add(gl_mul(gl_mul(m0, m1), c0), gl_mul(ad, c1))));
            }
        }
    }
}

// ---- gates over the extension algebra: an F_p^2 element occupies two consecutive wires; on the coset
// every wire value is a base-field number, so the algebra product is the plain F_p^2 product
// (chip/goldilocks_extension_algebra_chip.rs:112-146).  Each algebra constraint yields 2 terms.
#define WIRE2(j) gl2_make(WIRE(j), WIRE((j) + 1))
template <class GateAcc>
GL_DEV void push2(GateAcc& g, gl2 v) { g.push(v.c0); g.push(v.c1); }

// ArithmeticExtensionGate{num_ops}: out - (c0 m0 m1 + c1 addend)   (gates/arithmetic_extension.rs:22-80)
template <class GateAcc>
GL_DEV void gate_arithmetic_ext(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t num_ops) {
    const uint64_t c0 = CONST(a.c.num_selectors), c1 = CONST(a.c.num_selectors + 1);
    if (num_ops == 0) return;
    const uint32_t last = 8 * num_ops - 1;
    uint64_t nx[8];
    wire_group<8>(w, 0, last, nx);
    for (uint32_t i = 0; i < num_ops; i++) {                 // one operation = one group, requested an operation ahead
        uint64_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = nx[k];
        wire_group<8>(w, 8 * (i + 1), last, nx);
        const gl2 m0 = gl2_make(v[0], v[1]), m1 = gl2_make(v[2], v[3]), ad = gl2_make(v[4], v[5]), out = gl2_make(v[6], v[7]);
        const gl2 comp = gl2_add(gl2_mul_base(gl2_mul(m0, m1), c0), gl2_mul_base(ad, c1));
        push2(g, gl2_sub(out, comp));
    }
}
// MulExtensionGate{num_ops}: out - c0 m0 m1   (gates/multiplication_extension.rs:22-68)
template <class GateAcc>
GL_DEV void gate_mul_ext(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t num_ops) {
    const uint64_t c0 = CONST(a.c.num_selectors);
    if (num_ops == 0) return;
    const uint32_t last = 6 * num_ops - 1;
    uint64_t nx[6];
    wire_group<6>(w, 0, last, nx);
    for (uint32_t i = 0; i < num_ops; i++) {
        uint64_t v[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = nx[k];
        wire_group<6>(w, 6 * (i + 1), last, nx);
        const gl2 m0 = gl2_make(v[0], v[1]), m1 = gl2_make(v[2], v[3]), out = gl2_make(v[4], v[5]);
        push2(g, gl2_sub(out, gl2_mul_base(gl2_mul(m0, m1), c0)));
    }
}
// PoseidonMdsGate: out_r - sum_i CIRC[i] in[(i+r)%12] - DIAG[r] in[r]   (gates/poseidon_mds.rs:26-126).  The 24 input wires are
// read once into registers; four output rows per pass of the loop, after which the inputs are rotated by four elements, so
// that every register index is a compile-time one.  A row's two output wires are read when the row is pushed (a group of them does not fit next to the inputs at three waves).
template <class GateAcc>
GL_DEV void gate_poseidon_mds(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g) {
    uint64_t in[24];
    wire_group<24>(w, 0, 23, in);
#pragma unroll 1
    for (uint32_t r0 = 0; r0 < 12; r0 += 4) {
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            gl2 acc = gl2_make(0, 0);
#pragma unroll
            for (uint32_t i = 0; i < 12; i++) {
                const gl2 x = gl2_make(in[2 * ((i + r) % 12)], in[2 * ((i + r) % 12) + 1]);
                acc = gl2_add(acc, gl2_make(gl_mul_small(x.c0, GL_PSD_MDS_CIRC[i]), gl_mul_small(x.c1, GL_PSD_MDS_CIRC[i])));
            }
            if (r0 + r == 0) {
                const gl2 x = gl2_make(in[0], in[1]);
                acc = gl2_add(acc, gl2_make(gl_mul_small(x.c0, 8), gl_mul_small(x.c1, 8)));
            }
            push2(g, gl2_sub(WIRE2(2 * (12 + r0 + r)), acc));
        }
        uint64_t rot[8];
#pragma unroll
        for (int k = 0; k < 8; k++) rot[k] = in[k];
#pragma unroll
        for (int k = 0; k < 16; k++) in[k] = in[k + 8];
#pragma unroll
        for (int k = 0; k < 8; k++) in[16 + k] = rot[k];
    }
}
// RandomAccessGate{bits, copies, extra}   (gates/random_access.rs:27-147)
template <class GateAcc>
GL_DEV void gate_random_access(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t param) {
    const uint32_t bits = param & 0xFF, copies = (param >> 8) & 0xFF, extra = (param >> 16) & 0xFF;
    const uint32_t vec = 1u << bits, routed = (2 + vec) * copies + extra;
    for (uint32_t c = 0; c < copies; c++) {
        const uint32_t base = (2 + vec) * c;
        // a copy's wires in one go: its bit wires (<= 4) once, the claimed index and element, the list (<= 16 items)
        uint64_t b[4], hd[2], items[16];
        wire_group<4>(w, routed + c * bits, routed + c * bits + bits - 1, b);      // 1 <= bits <= 4 (checked at launch)
        wire_group<2>(w, base, base + 1, hd);
        wire_group<8>(w, base + 2, base + 1 + vec, &items[0]);
        if (vec > 8) wire_group<8>(w, base + 10, base + 1 + vec, &items[8]);
        uint64_t recon = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if ((uint32_t)i < bits) g.push(gl_sub(gl_mul(b[i], b[i]), b[i]));
#pragma unroll
        for (int i = 3; i >= 0; i--)
            if ((uint32_t)i < bits) recon = gl_add(gl_add(recon, recon), b[i]);
        g.push(gl_sub(recon, hd[0]));
        // fold the list: item = x + b (y - x) per pair, one bit per level (bits <= 4 => <= 16 items; entries past the list
        // hold clamped re-reads and are never folded in)
        uint32_t len = vec;
        for (uint32_t lvl = 0; lvl < bits; lvl++) {
            const uint64_t bl = b[0];                // the level's bit; the rest move down one place
            b[0] = b[1]; b[1] = b[2]; b[2] = b[3];
            for (uint32_t k = 0; k < 8; k++) {
                if (k < len / 2) items[k] = gl_add(gl_mul(bl, gl_sub(items[2 * k + 1], items[2 * k])), items[2 * k]);
            }
            len >>= 1;
        }
        g.push(gl_sub(items[0], hd[1]));
    }
    if (extra != 0) {
        for (uint32_t i0 = 0; i0 < extra; i0 += 4) {
            uint64_t cv[4], v[4];
            const_group<4>(a, w, t, a.c.num_selectors + i0, a.c.num_selectors + extra - 1, cv);
            wire_group<4>(w, (2 + vec) * copies + i0, (2 + vec) * copies + extra - 1, v);
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i0 + i < extra) g.push(gl_sub(cv[i], v[i]));
        }
    }
}
// ReducingGate{n} / ReducingExtensionGate{n}: acc*alpha + coeff - acc_i   (gates/reducing.rs:20-85,
// gates/reducing_extension.rs:20-87); the last accumulator is the output (wires 0..1)
template <bool EXT, class GateAcc>
GL_DEV void gate_reducing(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t n) {
    constexpr int CW = EXT ? 8 : 4;                          // coefficient wires of four steps
    if (n == 0) return;
    uint64_t hd[6];                                          // output, alpha, initial accumulator
    wire_group<6>(w, 0, 5, hd);
    const gl2 alpha = gl2_make(hd[2], hd[3]);
    gl2 acc = gl2_make(hd[4], hd[5]);
    const uint32_t start_accs = 6 + (EXT ? 2 * n : n);
    // four steps = one group of coefficients + one group of old accumulators; the last step's accumulator is the output, so the
    // accumulator columns end at start_accs + 2 (n - 1) - 1 (for n = 1 that clamps onto the coefficient wire in front of them)
    const uint32_t last_coeff = start_accs - 1, last_acc = start_accs + 2 * (n - 1) - 1;
    for (uint32_t i0 = 0; i0 < n; i0 += 4) {
        uint64_t cf[CW], ac[8];
        wire_group<CW>(w, 6 + (EXT ? 2 : 1) * i0, last_coeff, cf);
        wire_group<8>(w, start_accs + 2 * i0, last_acc, ac);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (i0 + i < n) {
                gl2 coeff;
                if constexpr (EXT) coeff = gl2_make(cf[2 * i], cf[2 * i + 1]);
                else coeff = gl2_make(cf[i], 0);
                const gl2 acc_i = (i0 + i == n - 1) ? gl2_make(hd[0], hd[1]) : gl2_make(ac[2 * i], ac[2 * i + 1]);
                push2(g, gl2_sub(gl2_add(gl2_mul(acc, alpha), coeff), acc_i));
                acc = acc_i;
            }
        }
    }
}

// CosetInterpolationGate{subgroup_bits b, degree d} (plonky2 gates/coset_interpolation.rs; layout and formula in coset_interp.h):
// 2 (2 + 2 n_int) constraints.  The domain x_i = g^i of the three subgroup sizes is one table (the 16th roots of unity, strided) and
// the barycentric weights w_i = x_i / N one table per size; the gate type and its parameter are wave-uniform, so the entries come
// through the scalar cache.  The value wires arrive in groups of eight (four extension values), requested one group ahead; x, eval and
// prod stay gl2 values in the lazy form (any u64) until they are pushed.  Every register index is a compile-time one.
__device__ __constant__ const uint64_t CI_X16[16] = {
    0x0000000000000001ull, 0xefffffff00000001ull, 0xfffffffeff000001ull, 0x000ffffffff00000ull, 0x0001000000000000ull, 0x0000000000001000ull,
    0xfffffeff00000101ull, 0xffffffef00000001ull, 0xffffffff00000000ull, 0x1000000000000000ull, 0x0000000001000000ull, 0xffefffff00100001ull,
    0xfffeffff00000001ull, 0xfffffffefffff001ull, 0x000000ffffffff00ull, 0x0000001000000000ull};      // (7^((p-1)/16))^i
__device__ __constant__ const uint64_t CI_W[3][16] = {                                                // x_i / N for N = 4, 8, 16
    {0xbfffffff40000001ull, 0x0000400000000000ull, 0x3fffffffc0000000ull, 0xffffbfff00000001ull},
    {0xdfffffff20000001ull, 0xfffffffeffe00001ull, 0x0000200000000000ull, 0xffffffdf00000021ull, 0x1fffffffe0000000ull, 0x0000000000200000ull,
     0xffffdfff00000001ull, 0x0000001fffffffe0ull},
    {0xefffffff10000001ull, 0xfeffffff00000001ull, 0xfffffffefff00001ull, 0x0000ffffffff0000ull, 0x0000100000000000ull, 0x0000000000000100ull,
     0xffffffef00000011ull, 0xfffffffe00000001ull, 0x0ffffffff0000000ull, 0x0100000000000000ull, 0x0000000000100000ull, 0xfffeffff00010001ull,
     0xffffefff00000001ull, 0xfffffffeffffff01ull, 0x0000000ffffffff0ull, 0x0000000100000000ull}};
template <class GateAcc>
GL_DEV void gate_coset_interpolation(const QuotArgs& a, const WireSrc& w, uint64_t t, GateAcc& g, uint32_t param) {
    CosetInterpShape s;
    coset_interp_shape(param, s);                            // checked at launch
    typedef const __attribute__((address_space(4))) uint64_t* Tab;
    const Tab xs = (Tab)CI_X16, ws = (Tab)CI_W[s.bits - 2];
    const uint32_t stride = 16u >> s.bits, last = 2 * s.n;   // the last value wire
    const uint64_t shift = WIRE(0);
    uint64_t pv[4], sh[2], nx[8];
    wire_group<4>(w, s.point, s.point + 3, pv);              // evaluation point, evaluation value
    wire_group<2>(w, s.shifted, s.shifted + 1, sh);
    wire_group<8>(w, 1, last, nx);
    const gl2 x = gl2_make(sh[0], sh[1]);
    push2(g, gl2_sub(gl2_make(pv[0], pv[1]), gl2_mul_base(x, shift)));
    gl2 eval = gl2_make(0, 0), prod = gl2_make(1, 0);
    uint32_t brk = s.degree, ni = 0;
    for (uint32_t i0 = 0; i0 < s.n; i0 += 4) {
        uint64_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = nx[k];
        wire_group<8>(w, 1 + 2 * (i0 + 4), last, nx);        // clamped behind the last group
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t i = i0 + k;
            if (i == brk) {                                  // wave-uniform: the fold continues from intermediate pair ni
                uint64_t ie[2], ip[2];
                wire_group<2>(w, s.start_int + 2 * ni, s.start_int + 2 * ni + 1, ie);
                wire_group<2>(w, s.start_int + 2 * (s.n_int + ni), s.start_int + 2 * (s.n_int + ni) + 1, ip);
                push2(g, gl2_sub(gl2_make(ie[0], ie[1]), eval));
                push2(g, gl2_sub(gl2_make(ip[0], ip[1]), prod));
                eval = gl2_make(ie[0], ie[1]); prod = gl2_make(ip[0], ip[1]);
                ni++; brk += s.degree - 1;
            }
            const gl2 xm = gl2_make(gl_sub(x.c0, xs[i * stride]), x.c1);
            const gl2 vw = gl2_mul_base(gl2_make(v[2 * k], v[2 * k + 1]), ws[i]);
            eval = gl2_add(gl2_mul(eval, xm), gl2_mul(vw, prod));
            prod = gl2_mul(prod, xm);
        }
    }
    push2(g, gl2_sub(gl2_make(pv[2], pv[3]), eval));
}

// STAGE (experiment of round 2, not instantiated any more: profiles/r02_quotient_ab.txt): the wave first copies its 64 points' wire rows (num_wires x 64 x 8 B = 69 KB) into LDS and
// every evaluator reads them from there -- each wire column crosses the fabric once instead of ~4 times, at 2 waves per CU.
// INTERP: the instances that also know CosetInterpolationGate.  The kernel is tuned to three waves per SIMD and its register
// allocation follows every evaluator in the gate loop, so the thirteenth evaluator lives in instances of its own, launched when (and
// only when) the circuit has that gate; the INTERP = false instances are the code every circuit without it has always run.
template <int NCH, bool STAGE = false, bool INTERP = false>
__global__ void __launch_bounds__(STAGE ? 64 : 128) __attribute__((amdgpu_waves_per_eu(STAGE ? 1 : 3, 3))) quotient_kernel(QuotArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t wire_lds[];
    const uint64_t nq = 1ull << a.qbits;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const uint32_t unit = blockIdx.y;
    const uint64_t* __restrict__ wglob = a.wires + (uint64_t)unit * a.wires_us;
    WireSrc w{wglob, a.lde_stride, t, a.lde_stride};
    if constexpr (STAGE) {
        for (uint32_t j = 0; j < a.c.num_wires; j++) wire_lds[j * 64 + threadIdx.x] = wglob[(uint64_t)j * a.lde_stride + t];
        w = WireSrc{wire_lds, 64, threadIdx.x, a.lde_stride};        // one wave per block: no barrier needed, each lane reads only its own column entries
    }
    const uint64_t* __restrict__ zs = a.zs + (uint64_t)unit * a.zs_us;
    const uint32_t qdb = a.qbits - a.c.degree_bits;
    const uint64_t iq = __brevll(t) >> (64 - a.qbits);   // natural index of storage row t
    const uint64_t x = gl_mul_small(gl_mul(a.xw_lo[iq & 4095], a.xw_hi[iq >> 12]), 7);
    // next row: natural index iq + 2^qdb (g*x), its storage row is bitrev of that
    const uint64_t iq_next = (iq + (1ull << qdb)) & (nq - 1);
    const uint64_t t_next = __brevll(iq_next) >> (64 - a.qbits);
    constexpr uint32_t nch = NCH;
    const uint32_t npp = a.c.num_partial_products;
    const uint32_t routed = a.c.num_routed_wires, chunk = a.c.max_degree;
    const uint32_t n_sel = a.c.num_selectors, n_cst = a.c.num_constants;

    AlphaAcc<NCH> total;
    total.init(a, unit);
    // ---- L0(x) (Z_c(x) - 1);  L0(x) = (x^n - 1) / (n (x - 1))  (vanishing_poly.rs:155-178) ---------
    const uint64_t zh = a.zh[iq & ((1u << qdb) - 1)];  // x^n - 1 (never zero on the coset)
    const uint64_t l0 = gl_mul(gl_mul(zh, a.n_inv), gl_inv(gl_sub(x, 1)));
    for (uint32_t c = 0; c < nch; c++) {
        const uint64_t z = zs[(uint64_t)c * a.lde_stride + t];
        total.push(gl_sub(gl_mul(l0, z), l0));
    }
    // ---- partial products (vanishing_poly.rs:54-108, 183-218) -------------------------------------
    // every routed wire and its sigma value are loaded ONCE and serve all challenges (the term of (challenge c, chunk ch) keeps
    // its place c * n_chunks + ch in the stream: push_at)
    {
        const uint32_t n_chunks = (routed + chunk - 1) / chunk;
        uint64_t prev[NCH], bx[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            prev[c] = zs[(uint64_t)c * a.lde_stride + t];
            bx[c] = gl_mul(a.betas[unit * 4 + c], x);
        }
        const uint32_t first = total.idx;
        // wire j + 1, its sigma and its k are requested before the eight products of wire j (the index is clamped to the last
        // routed wire: sigma_{routed-1} is the last column of its batch)
        const uint32_t sig0 = n_sel + n_cst;
        uint64_t wn = WIRE(0), sn = CONST(sig0), kn = a.k_is[0];
        for (uint32_t ch = 0; ch < n_chunks; ch++) {
            uint64_t num[NCH], den[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) { num[c] = 1; den[c] = 1; }
            for (uint32_t j = ch * chunk; j < (ch + 1) * chunk && j < routed; j++) {
                const uint64_t wj = wn, sj = sn, kj = kn;
                const uint32_t jn = j + 1 < routed ? j + 1 : routed - 1;
                wn = WIRE(jn); sn = CONST(sig0 + jn); kn = a.k_is[jn];
                if constexpr (NCH == 2) {
                    // the eight products of a wire in two lock-step groups of four (gl_mul_multi: partners fill the carry wait states)
                    const uint64_t a1[4] = {bx[0], bx[1], a.betas[unit * 4], a.betas[unit * 4 + 1]}, b1[4] = {kj, kj, sj, sj};
                    uint64_t p1[4], p2[4];
                    gl_mul_multi<4>(a1, b1, p1);
                    const uint64_t wg0 = gl_add(wj, a.gammas[unit * 4]), wg1 = gl_add(wj, a.gammas[unit * 4 + 1]);
                    const uint64_t a2[4] = {num[0], num[1], den[0], den[1]};
                    const uint64_t b2[4] = {gl_add(wg0, p1[0]), gl_add(wg1, p1[1]), gl_add(wg0, p1[2]), gl_add(wg1, p1[3])};
                    gl_mul_multi<4>(a2, b2, p2);
                    num[0] = p2[0]; num[1] = p2[1]; den[0] = p2[2]; den[1] = p2[3];
                } else {
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        const uint64_t wg = gl_add(wj, a.gammas[unit * 4 + c]);
                        num[c] = gl_mul(num[c], gl_add(wg, gl_mul(bx[c], kj)));
                        den[c] = gl_mul(den[c], gl_add(wg, gl_mul(a.betas[unit * 4 + c], sj)));
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const uint64_t next = (ch + 1 < n_chunks) ? zs[(uint64_t)(nch + c * npp + ch) * a.lde_stride + t]
                                                          : zs[(uint64_t)c * a.lde_stride + t_next];
                total.push_at(gl_sub(gl_mul(prev[c], num[c]), gl_mul(next, den[c])), first + c * n_chunks + ch);
                prev[c] = next;
            }
        }
        total.idx = first + nch * n_chunks;
    }
    // ---- gate constraints, each gate's stream multiplied by its filter (gates/mod.rs:87-132) ---------
    uint64_t gate_sum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) gate_sum[c] = 0;
    for (uint32_t gi = 0; gi < a.c.num_gates; gi++) {
        const gl355_gate gt = a.c.gates[gi];
        if (gt.type == GL355_GATE_NOOP) continue;
        GateAccT<NCH> g;
        // every column address of an evaluator is invariant in this loop; left visible, the compiler forms them all in front of
        // the loop and spills them, so each gate starts from strides and a row index it cannot see through
        WireSrc wg = w;
        uint64_t tg = t;
        asm volatile("" : "+s"(wg.stride), "+s"(wg.cs_stride), "+v"(tg));
        wg.idx = STAGE ? w.idx : tg;
        g.init(a, unit, total.idx);
        bool interp = false;
        if constexpr (INTERP) {
            if (gt.type == GL355_GATE_COSET_INTERPOLATION) { gate_coset_interpolation(a, wg, tg, g, gt.param); interp = true; }
        }
        if (!interp) switch (gt.type) {
            case GL355_GATE_POSEIDON: gate_poseidon(a, wg, tg, g); break;
            case GL355_GATE_BASE_SUM: gate_base_sum(a, wg, tg, g, gt.param); break;
            case GL355_GATE_CONSTANT: gate_constant(a, wg, tg, g, gt.param); break;
            case GL355_GATE_PUBLIC_INPUT: gate_public_input(a, wg, tg, g, unit); break;
            case GL355_GATE_ARITHMETIC: gate_arithmetic(a, wg, tg, g, gt.param); break;
            case GL355_GATE_ARITHMETIC_EXT: gate_arithmetic_ext(a, wg, tg, g, gt.param); break;
            case GL355_GATE_MUL_EXT: gate_mul_ext(a, wg, tg, g, gt.param); break;
            case GL355_GATE_POSEIDON_MDS: gate_poseidon_mds(a, wg, tg, g); break;
            case GL355_GATE_RANDOM_ACCESS: gate_random_access(a, wg, tg, g, gt.param); break;
            case GL355_GATE_REDUCING: gate_reducing<false>(a, wg, tg, g, gt.param); break;
            case GL355_GATE_REDUCING_EXT: gate_reducing<true>(a, wg, tg, g, gt.param); break;
            default: break;
        }
        const uint64_t sel = CONST(gt.selector_index);
        uint64_t filter = 1;
        for (uint32_t k = gt.group_start; k < gt.group_end; k++)
            if (k != gi) filter = gl_mul(filter, gl_sub(k, sel));
        if (n_sel > 1) filter = gl_mul(filter, gl_sub(0xFFFFFFFFull, sel));  // UNUSED_SELECTOR = u32::MAX
#pragma unroll
        for (uint32_t c = 0; c < nch; c++) gate_sum[c] = gl_add(gate_sum[c], gl_mul(filter, g.value(c)));
    }
    const uint64_t zh_inv = a.zh_inv[iq & ((1u << qdb) - 1)];
    for (uint32_t c = 0; c < nch; c++) {
        const uint64_t v = gl_mul(gl_add(total.acc[c], gate_sum[c]), zh_inv);
        a.out[((uint64_t)unit * nch + c) * nq + t] = gl_canon(v);
    }
}

int32_t quotient_dev(Ctx* ctx, const gl355_circuit* c, const uint64_t* cs_lde, const uint64_t* wires_lde,
                     const uint64_t* zs_lde, uint64_t lde_stride, const uint64_t* k_is_dev, const uint64_t* betas,
                     const uint64_t* gammas, const uint64_t* alphas, const uint64_t pi_hash[4], uint64_t* out_values) {
    uint64_t b[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0}, al[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < c->num_challenges && i < 4; i++) { b[i] = betas[i]; g[i] = gammas[i]; al[i] = alphas[i]; }
    return quotient_units_dev(ctx, c, 1, cs_lde, wires_lde, 0, zs_lde, 0, lde_stride, k_is_dev, b, g, al, pi_hash, out_values);
}

// B lock-step units (blockIdx.y): betas / gammas / alphas / pi_hashes are [B][4]
int32_t quotient_units_dev(Ctx* ctx, const gl355_circuit* c, uint32_t B, const uint64_t* cs_lde, const uint64_t* wires_lde, uint64_t wires_us,
                           const uint64_t* zs_lde, uint64_t zs_us, uint64_t lde_stride, const uint64_t* k_is_dev, const uint64_t* betas,
                           const uint64_t* gammas, const uint64_t* alphas, const uint64_t* pi_hashes, uint64_t* out_values) {
    uint32_t qdb = 0;
    while ((1u << qdb) < c->max_degree) qdb++;
    if ((1u << qdb) != c->max_degree || qdb > c->rate_bits || qdb > 4) return ctx->fail(GL355_E_UNSUPPORTED, "quotient: degree factor must be a power of two <= 2^rate_bits");
    if (c->num_challenges == 0 || c->num_challenges > 4) return ctx->fail(GL355_E_UNSUPPORTED, "quotient: 1..4 challenges");
    if (B == 0 || B > GL355_MAX_UNITS) return ctx->fail(GL355_E_INVALID_ARG, "quotient: 1..GL355_MAX_UNITS units");
    // the evaluators index the wire and constant columns unchecked: every gate's wires and constants exist (gate_shape.h) before
    // anything is allocated or launched.  The evaluators' own limits follow.
    char msg[GATE_MSG_LEN];
    if (gate_table_check(*c, "quotient", msg) != GL355_OK) return ctx->fail(GL355_E_INVALID_ARG, msg);
    // length of the constraint stream = the permutation-argument prefix + the longest gate (the evaluators push exactly
    // GateShape::constraints terms)
    uint32_t longest = 0;
    bool has_interp = false;
    for (uint32_t g = 0; g < c->num_gates; g++) {
        const uint32_t type = c->gates[g].type, bits = c->gates[g].param & 0xFF;
        // the evaluator keeps a copy's bit wires in four registers and its list in sixteen
        if (type == GL355_GATE_RANDOM_ACCESS && (bits < 1 || bits > 4)) return ctx->fail(GL355_E_UNSUPPORTED, "quotient: RandomAccessGate with 1..4 bits");
        // the evaluator's domain and weight tables are those of 4, 8 and 16 points (coset_interp_shape knows no other today)
        if (type == GL355_GATE_COSET_INTERPOLATION && (bits < 2 || bits > 4))
            return ctx->fail(GL355_E_UNSUPPORTED, "quotient: CosetInterpolationGate with 2..4 subgroup bits");
        has_interp |= type == GL355_GATE_COSET_INTERPOLATION;
        GateShape s;
        gate_shape(type, c->gates[g].param, s);
        longest = s.constraints > longest ? s.constraints : longest;
    }
    QuotArgs a;
    memset(&a, 0, sizeof a);
    a.c = *c;
    a.cs = cs_lde; a.wires = wires_lde; a.zs = zs_lde; a.lde_stride = lde_stride; a.wires_us = wires_us; a.zs_us = zs_us;
    a.qbits = c->degree_bits + qdb;
    a.k_is = k_is_dev;
    GL355_TRY(ctx->pow_tables(gl_root_of_unity(a.qbits), &a.xw_lo, &a.xw_hi));
    // x^n = 7^n * omega_{2^qdb}^(i mod 2^qdb)
    const uint64_t sn = gl_pow(7, 1ull << c->degree_bits);
    const uint64_t wq = gl_root_of_unity(qdb);
    uint64_t w = 1;
    for (uint32_t k = 0; k < (1u << qdb); k++) {
        a.zh[k] = gl_canon(gl_sub(gl_mul(sn, w), 1));
        a.zh_inv[k] = gl_canon(gl_inv(a.zh[k]));
        w = gl_mul(w, wq);
    }
    AlphaTabArgs ta;
    memset(&ta, 0, sizeof ta);
    for (uint32_t u = 0; u < B; u++) {
        for (uint32_t i = 0; i < c->num_challenges; i++) {
            a.betas[u * 4 + i] = gl_canon(betas[u * 4 + i]); a.gammas[u * 4 + i] = gl_canon(gammas[u * 4 + i]);
            ta.alphas[u * 4 + i] = gl_canon(alphas[u * 4 + i]);
        }
        for (int i = 0; i < 4; i++) a.pi_hash[u * 4 + i] = gl_canon(pi_hashes[u * 4 + i]);
    }
    a.n_inv = gl_canon(gl_inv((1ull << c->degree_bits) % GL_P));
    a.out = out_values;
    const uint32_t n_chunks = (c->num_routed_wires + c->max_degree - 1) / c->max_degree;
    a.pw_stride = ((c->num_challenges * (1 + n_chunks) + longest + 1) + 63) & ~63u;
    Scratch pw(ctx);
    GL355_TRY(pw.get((size_t)B * c->num_challenges * a.pw_stride * 8));
    a.alpha_pw = pw.as<uint64_t>();
    ta.nch = c->num_challenges; ta.stride = a.pw_stride; ta.out = pw.as<uint64_t>();
    hipLaunchKernelGGL(alpha_table_kernel, dim3((a.pw_stride + 255) / 256, B), dim3(256), 0, ctx->stream, ta);
    GL355_HIP(ctx, hipGetLastError());
    const uint64_t nq = 1ull << a.qbits;
    // every column of the three oracles once per point of the quotient coset + the result
    ProfScope ps(ctx, "quotient_kernel", (uint64_t)B * nq * 8 * ((uint64_t)c->num_selectors + c->num_constants + c->num_routed_wires + c->num_wires +
                                                   (uint64_t)c->num_challenges * (2 + c->num_partial_products)));
    // (the LDS-staged variant quotient_kernel<NCH, true> measured slower -- profiles/r02_quotient_ab.txt -- and is no longer instantiated)
    // three and four challenges: no circuit of the project has them; those instantiations do not fit 168 registers with the grouped
    // reads and spill (156 / 372 bytes of scratch per lane) -- correct, slower than they could be
    const dim3 grid((uint32_t)((nq + 127) / 128), B);
    if (has_interp) {        // a circuit with CosetInterpolationGate: the instances that know it (see quotient_kernel)
        switch (c->num_challenges) {
            case 1: hipLaunchKernelGGL((quotient_kernel<1, false, true>), grid, dim3(128), 0, ctx->stream, a); break;
            case 2: hipLaunchKernelGGL((quotient_kernel<2, false, true>), grid, dim3(128), 0, ctx->stream, a); break;
            case 3: hipLaunchKernelGGL((quotient_kernel<3, false, true>), grid, dim3(128), 0, ctx->stream, a); break;
            default: hipLaunchKernelGGL((quotient_kernel<4, false, true>), grid, dim3(128), 0, ctx->stream, a); break;
        }
    } else switch (c->num_challenges) {
        case 1: hipLaunchKernelGGL(quotient_kernel<1>, grid, dim3(128), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(quotient_kernel<2>, grid, dim3(128), 0, ctx->stream, a); break;
        case 3: hipLaunchKernelGGL(quotient_kernel<3>, grid, dim3(128), 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL(quotient_kernel<4>, grid, dim3(128), 0, ctx->stream, a); break;
    }
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

}  // namespace gl355
