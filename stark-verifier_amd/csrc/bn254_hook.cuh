// Record layouts and limb helpers of the BN254 test hooks (include/gl355.h "test hooks"): gl355_bn254_arith_batch / gl355_bn254_g1_chain in
// bn254_curve_hook.hip, their j_* chains in bn254_g1_hook.hip, the hasher's fr_enter / fr_leave in merkle_bn254.hip.  Test entry points only.
#pragma once
#include "bn254_f29.cuh"
#include "bn254_g1.cuh"

namespace gl355 {
#define HK_OPND 28u                                                  // operand record: x[9] y[9] z[9] identity
#define HK_REC 40u                                                   // trace record: four 9-word slots, identity, accumulator, 0, 0
GL_DEV u256 hk_u(const uint32_t* p) {
    u256 r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.l[j] = p[j];
    return r;
}
GL_DEV f29 hk_f(const uint32_t* p) {
    f29 r;
#pragma unroll
    for (int j = 0; j < 9; j++) r.l[j] = p[j];
    return r;
}
GL_DEV void hk_put_u(uint32_t* o, const u256& v) {
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = v.l[j];
    o[8] = 0;
}
GL_DEV void hk_put_f(uint32_t* o, const f29& v) {
#pragma unroll
    for (int j = 0; j < 9; j++) o[j] = v.l[j];
}
GL_DEV void hk_put_b(uint32_t* o, bool v) {
    o[0] = v ? 1u : 0u;
#pragma unroll
    for (int j = 1; j < 9; j++) o[j] = 0;
}
GL_DEV void hk_rec(uint32_t* r, const uint32_t* c0, const uint32_t* c1, const uint32_t* c2, const uint32_t* c3, int w, bool ident, uint32_t which) {
    for (int j = 0; j < 9; j++) {
        r[j] = j < w ? c0[j] : 0u;
        r[9 + j] = j < w ? c1[j] : 0u;
        r[18 + j] = j < w ? c2[j] : 0u;
        r[27 + j] = c3 && j < w ? c3[j] : 0u;
    }
    r[36] = ident ? 1u : 0u;
    r[37] = which;
    r[38] = r[39] = 0;
}
GL_DEV void hk_rec_bad(uint32_t* r) {
    for (uint32_t j = 0; j < HK_REC; j++) r[j] = 0;
    r[37] = 0xffffffffu;
}
GL_DEV void hk_rec_jac(uint32_t* r, const jac& p, uint32_t which) { hk_rec(r, p.x.l, p.y.l, p.z.l, nullptr, 8, j_is_identity(p), which); }
GL_DEV jac hk_jac(const uint32_t* o) {
    jac p;
    p.x = hk_u(o); p.y = hk_u(o + 9); p.z = hk_u(o + 18);
    return p;
}
}  // namespace gl355
