// The register file of the PLONK expression interpreters and the helpers they share: plonk_kernels.cuh (the prover's evaluator) and
// plonk_check.hip (the witness checker's row-domain evaluator with poison bits) run the same programs over the same file.
#pragma once
#include "bn254_field.cuh"
#include "plonk_program.h"

namespace gl355 {

GL_DEV u256 fr_one() { return u_const(BN254C_FR_ONE); }
GL_DEV u256 fr_neg(const u256& a) { return m_sub<F_R>(u_zero(), a); }

// position of the point `rot` steps after the point at position i
GL_DEV uint64_t plk_rotated(uint64_t i, int32_t rot, uint64_t n, uint32_t log_n, uint32_t bitrev) {
    if (rot == 0) return i;
    if (!bitrev) return (uint64_t)((int64_t)i + (int64_t)n + rot) & (n - 1);
    const uint64_t j = __brevll(i) >> (64 - log_n);
    return __brevll((uint64_t)((int64_t)j + (int64_t)n + rot) & (n - 1)) >> (64 - log_n);
}
// (Measured alternative: the file in LDS, [register][limb][lane] with one wave per workgroup -- no scratch, but 24 KB per wave leave six waves
// per CU, and evaluate_h at k = 23 took 627 ms against 598 ms with the scratch-backed file below; the scratch lines of a wave stay in L2.)
#define PLK_REG_CASES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11)
// the register file as twelve named values: the compiler still places it in scratch memory (400 bytes per lane), as it does an indexed array
struct PlkRegs {
#define PLK_DECL(K) u256 r##K;
    PLK_REG_CASES(PLK_DECL)
#undef PLK_DECL
};
GL_DEV u256 plk_reg_read(const PlkRegs& f, uint32_t i) {
    switch (i) {
#define PLK_RD(K) case K: return f.r##K;
        PLK_REG_CASES(PLK_RD)
#undef PLK_RD
    default: return f.r0;
    }
}
GL_DEV void plk_reg_write(PlkRegs& f, uint32_t i, const u256& v) {
    switch (i) {
#define PLK_WR(K) case K: f.r##K = v; break;
        PLK_REG_CASES(PLK_WR)
#undef PLK_WR
    default: break;
    }
}
}  // namespace gl355
