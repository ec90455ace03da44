// CosetInterpolationGate { subgroup_bits, degree } (plonky2 gates/coset_interpolation.rs, D = 2): layout and witness generation, shared
// by the host (gl355_coset_interpolation_witness, the tape replay, the verifier's and the launcher's shape checks) and the device
// tape interpreter.  The gate is restated from upstream's definition (include/gl355.h states it in full); the reference's verifier
// does not have it (chip/plonk/gates/mod.rs:141-196 lists 12 gates).
//
// N = 2^bits values v_i (extension) on the coset shift * <g>, g = primitive_root_of_unity(bits), are interpolated at an extension
// point in barycentric form on the SUBGROUP: x = point / shift, x_i = g^i, w_i = 1 / prod_{j != i}(x_i - x_j) = x_i / N,
//   (eval, prod) <- (eval (x - x_i) + v_i w_i prod, prod (x - x_i))  from (0, 1);  the value is eval after point N - 1.
// A gate of degree d folds d points from (0, 1) and d - 1 points from every (eval, prod) pair it has on intermediate wires.
#pragma once
#include "gl_field.cuh"

namespace gl355 {

struct CosetInterpShape {
    uint32_t bits, degree, n, n_int;
    uint32_t point, value, start_int, shifted;      // wire positions (value i at 1 + 2 i; start_int = the routed wires)
    uint32_t num_wires, num_constraints;
};
// false: bits outside 2..4 or degree outside 2..N (a degree above N would fold points the gate does not have)
GL_HD bool coset_interp_shape(uint32_t param, CosetInterpShape& s) {
    s.bits = param & 0xFF; s.degree = (param >> 8) & 0xFF;
    if ((param >> 16) != 0 || s.bits < 2 || s.bits > 4) return false;
    s.n = 1u << s.bits;
    if (s.degree < 2 || s.degree > s.n) return false;
    s.n_int = (s.n - 2) / (s.degree - 1);
    s.point = 1 + 2 * s.n; s.value = s.point + 2; s.start_int = s.point + 4;
    s.shifted = s.start_int + 4 * s.n_int;
    s.num_wires = s.shifted + 2;
    s.num_constraints = 2 * (2 + 2 * s.n_int);
    return true;
}
// first point of the chunk that continues from intermediate pair i (the first chunk is [0, degree))
GL_HD uint32_t coset_interp_chunk_start(const CosetInterpShape& s, uint32_t i) { return 1 + (s.degree - 1) * (i + 1); }

// fills shifted_evaluation_point, the intermediates and evaluation_value of the row at W.  0 ok, 1 = shift is zero
GL_HD int coset_interp_fill(const CosetInterpShape& s, uint64_t* W) {
    const uint64_t shift = gl_canon(W[0]);
    if (shift == 0) return 1;
    const uint64_t g = gl_root_of_unity(s.bits), n_inv = gl_inv(s.n);
    const gl2 x = gl2_canon(gl2_mul_base(gl2_make(W[s.point], W[s.point + 1]), gl_inv(shift)));
    W[s.shifted] = x.c0; W[s.shifted + 1] = x.c1;
    gl2 eval = gl2_make(0, 0), prod = gl2_make(1, 0);
    uint64_t xi = 1;
    uint32_t next_int = 0, brk = s.degree;
    for (uint32_t i = 0; i < s.n; i++) {
        if (i == brk && next_int < s.n_int) {
            eval = gl2_canon(eval); prod = gl2_canon(prod);
            W[s.start_int + 2 * next_int] = eval.c0; W[s.start_int + 2 * next_int + 1] = eval.c1;
            W[s.start_int + 2 * (s.n_int + next_int)] = prod.c0; W[s.start_int + 2 * (s.n_int + next_int) + 1] = prod.c1;
            next_int++; brk += s.degree - 1;
        }
        const gl2 xm = gl2_make(gl_sub(x.c0, xi), x.c1);
        const gl2 vw = gl2_mul_base(gl2_make(W[1 + 2 * i], W[2 + 2 * i]), gl_mul(xi, n_inv));
        eval = gl2_add(gl2_mul(eval, xm), gl2_mul(vw, prod));
        prod = gl2_mul(prod, xm);
        xi = gl_mul(xi, g);
    }
    eval = gl2_canon(eval);
    W[s.value] = eval.c0; W[s.value + 1] = eval.c1;
    return 0;
}

}  // namespace gl355
