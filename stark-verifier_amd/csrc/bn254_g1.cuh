// BN254 G1 point arithmetic for the device: Jacobian coordinates over Fq in Montgomery form (bn254_field.cuh).  Shared by the MSM /
// fixed-base kernels (bn254_msm.hip, bn254_kzg.hip) and the group FFT (bn254_g1_fft.hip).
#pragma once
#include "bn254_field.cuh"

namespace gl355 {

struct jac { u256 x, y, z; };                 // z == 0 (mod q): the identity
GL_DEV jac j_identity() { jac p; p.x = u_const(BN254C_FQ_ONE); p.y = p.x; p.z = u_zero(); return p; }
GL_DEV bool j_is_identity(const jac& p) { return m_is_zero<F_Q>(p.z); }
__device__ __noinline__ jac j_double(jac p) {
    if (j_is_identity(p)) return p;
    const u256 a = m_mul<F_Q>(p.x, p.x), b = m_mul<F_Q>(p.y, p.y), c = m_mul<F_Q>(b, b);
    const u256 xb = m_add<F_Q>(p.x, b);
    u256 d = m_sub<F_Q>(m_sub<F_Q>(m_mul<F_Q>(xb, xb), a), c);
    d = m_add<F_Q>(d, d);
    const u256 e = m_add<F_Q>(m_add<F_Q>(a, a), a), f = m_mul<F_Q>(e, e);
    jac r;
    r.x = m_sub<F_Q>(f, m_add<F_Q>(d, d));
    u256 c8 = m_add<F_Q>(c, c);
    c8 = m_add<F_Q>(c8, c8);
    c8 = m_add<F_Q>(c8, c8);
    r.y = m_sub<F_Q>(m_mul<F_Q>(e, m_sub<F_Q>(d, r.x)), c8);
    const u256 yz = m_mul<F_Q>(p.y, p.z);
    r.z = m_add<F_Q>(yz, yz);
    return r;
}
// p + (x2, y2) with an affine second operand (Montgomery form; the caller skips the identity)
__device__ __noinline__ jac j_madd(jac p, u256 x2, u256 y2) {
    if (j_is_identity(p)) { jac r; r.x = x2; r.y = y2; r.z = u_const(BN254C_FQ_ONE); return r; }
    const u256 z1z1 = m_mul<F_Q>(p.z, p.z);
    const u256 u2 = m_mul<F_Q>(x2, z1z1), s2 = m_mul<F_Q>(m_mul<F_Q>(y2, p.z), z1z1);
    const u256 h = m_sub<F_Q>(u2, p.x), r = m_sub<F_Q>(s2, p.y);
    if (m_is_zero<F_Q>(h)) return m_is_zero<F_Q>(r) ? j_double(p) : j_identity();
    const u256 h2 = m_mul<F_Q>(h, h), h3 = m_mul<F_Q>(h2, h), v = m_mul<F_Q>(p.x, h2);
    jac o;
    o.x = m_sub<F_Q>(m_sub<F_Q>(m_mul<F_Q>(r, r), h3), m_add<F_Q>(v, v));
    o.y = m_sub<F_Q>(m_mul<F_Q>(r, m_sub<F_Q>(v, o.x)), m_mul<F_Q>(p.y, h3));
    o.z = m_mul<F_Q>(p.z, h);
    return o;
}
// the same, inlined into its caller: as a call the mixed addition makes every kernel that uses it a 210-VGPR kernel (two waves per SIMD: the
// convention keeps the callee's whole frame apart from the caller's); inlined, the bucket loops take 142 (three waves) -- the bucket
// accumulation is bound by the latency of its random 64-byte point reads, which more resident waves cover
GL_DEV jac j_madd_inl(const jac& p, const u256& x2, const u256& y2) {
    if (j_is_identity(p)) { jac r; r.x = x2; r.y = y2; r.z = u_const(BN254C_FQ_ONE); return r; }
    const u256 z1z1 = m_mul<F_Q>(p.z, p.z);
    const u256 u2 = m_mul<F_Q>(x2, z1z1), s2 = m_mul<F_Q>(m_mul<F_Q>(y2, p.z), z1z1);
    const u256 h = m_sub<F_Q>(u2, p.x), r = m_sub<F_Q>(s2, p.y);
    if (m_is_zero<F_Q>(h)) return m_is_zero<F_Q>(r) ? j_double(p) : j_identity();
    const u256 h2 = m_mul<F_Q>(h, h), h3 = m_mul<F_Q>(h2, h), v = m_mul<F_Q>(p.x, h2);
    jac o;
    o.x = m_sub<F_Q>(m_sub<F_Q>(m_mul<F_Q>(r, r), h3), m_add<F_Q>(v, v));
    o.y = m_sub<F_Q>(m_mul<F_Q>(r, m_sub<F_Q>(v, o.x)), m_mul<F_Q>(p.y, h3));
    o.z = m_mul<F_Q>(p.z, h);
    return o;
}
__device__ __noinline__ jac j_add(jac p, jac q) {
    if (j_is_identity(p)) return q;
    if (j_is_identity(q)) return p;
    const u256 z1z1 = m_mul<F_Q>(p.z, p.z), z2z2 = m_mul<F_Q>(q.z, q.z);
    const u256 u1 = m_mul<F_Q>(p.x, z2z2), u2 = m_mul<F_Q>(q.x, z1z1);
    const u256 s1 = m_mul<F_Q>(m_mul<F_Q>(p.y, q.z), z2z2), s2 = m_mul<F_Q>(m_mul<F_Q>(q.y, p.z), z1z1);
    const u256 h = m_sub<F_Q>(u2, u1), r = m_sub<F_Q>(s2, s1);
    if (m_is_zero<F_Q>(h)) return m_is_zero<F_Q>(r) ? j_double(p) : j_identity();
    const u256 h2 = m_mul<F_Q>(h, h), h3 = m_mul<F_Q>(h2, h), v = m_mul<F_Q>(u1, h2);
    jac o;
    o.x = m_sub<F_Q>(m_sub<F_Q>(m_mul<F_Q>(r, r), h3), m_add<F_Q>(v, v));
    o.y = m_sub<F_Q>(m_mul<F_Q>(r, m_sub<F_Q>(v, o.x)), m_mul<F_Q>(s1, h3));
    o.z = m_mul<F_Q>(m_mul<F_Q>(p.z, q.z), h);
    return o;
}
// inlined form for the reduction levels (same reason as j_madd_inl)
GL_DEV jac j_add_inl(const jac& p, const jac& q) {
    if (j_is_identity(p)) return q;
    if (j_is_identity(q)) return p;
    const u256 z1z1 = m_mul<F_Q>(p.z, p.z), z2z2 = m_mul<F_Q>(q.z, q.z);
    const u256 u1 = m_mul<F_Q>(p.x, z2z2), u2 = m_mul<F_Q>(q.x, z1z1);
    const u256 s1 = m_mul<F_Q>(m_mul<F_Q>(p.y, q.z), z2z2), s2 = m_mul<F_Q>(m_mul<F_Q>(q.y, p.z), z1z1);
    const u256 h = m_sub<F_Q>(u2, u1), r = m_sub<F_Q>(s2, s1);
    if (m_is_zero<F_Q>(h)) return m_is_zero<F_Q>(r) ? j_double(p) : j_identity();
    const u256 h2 = m_mul<F_Q>(h, h), h3 = m_mul<F_Q>(h2, h), v = m_mul<F_Q>(u1, h2);
    jac o;
    o.x = m_sub<F_Q>(m_sub<F_Q>(m_mul<F_Q>(r, r), h3), m_add<F_Q>(v, v));
    o.y = m_sub<F_Q>(m_mul<F_Q>(r, m_sub<F_Q>(v, o.x)), m_mul<F_Q>(s1, h3));
    o.z = m_mul<F_Q>(m_mul<F_Q>(p.z, q.z), h);
    return o;
}
GL_DEV void j_store(uint32_t* dst, const jac& p) {
#pragma unroll
    for (int j = 0; j < 8; j++) { dst[j] = p.x.l[j]; dst[8 + j] = p.y.l[j]; dst[16 + j] = p.z.l[j]; }
}
GL_DEV jac j_load(const uint32_t* src) {
    jac p;
#pragma unroll
    for (int j = 0; j < 8; j++) { p.x.l[j] = src[j]; p.y.l[j] = src[8 + j]; p.z.l[j] = src[16 + j]; }
    return p;
}

GL_DEV void j_to_affine_mont(const jac& p, u256& x, u256& y) {           // p not the identity
    const u256 zi = m_inv<F_Q>(p.z), zi2 = m_mul<F_Q>(zi, zi);
    x = m_mul<F_Q>(p.x, zi2);
    y = m_mul<F_Q>(p.y, m_mul<F_Q>(zi2, zi));
}

}  // namespace gl355
