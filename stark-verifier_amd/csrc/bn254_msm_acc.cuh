// Point forms of the MSM's accumulators, shared by the MSM kernels (bn254_msm.hip) and the chain test hook (bn254_curve_hook.hip).
// The product kernels add bucket points in XYZZ coordinates on nine 29-bit limbs (xyzz29, msm_add_point_xyzz) and run the reduction levels on
// Jacobian points in the same limb form (jac29_add / jac29_double); the point table they read holds x 2^261, y 2^261 (msm_table_form).
#pragma once
#include "bn254_field.cuh"
#include "bn254_f29.cuh"
#include "bn254_g1.cuh"

namespace gl355 {
// the point table's form: the bucket loops add in the 29-bit-limb form of bn254_f29.cuh, whose Montgomery radix is 2^261, so the table holds
// x 2^261, y 2^261 (one product by the Montgomery form of 2^32 per coordinate and MSM)
GL_DEV u256 msm_table_form(const u256& v_mont) {
    return m_canon<F_Q>(m_mul<F_Q>(v_mont, u_const(FQ_C32)));
}
// msm_add_point (8 x 32-bit Jacobian, table in the R = 2^256 form) and msm_add_point29 (29-bit Jacobian) are the cross-check forms of the bucket
// addition: no product kernel calls them, they are reachable only through the chain hook (GL355_BN_CHAIN_JAC / _JAC29).
GL_DEV jac msm_add_point(const uint32_t* pm, jac acc, uint32_t e) {      // e: point index, bit 31 = subtract
    const uint32_t* p = pm + 16ull * (e & 0x7fffffffu);
    u256 x, y;
#pragma unroll
    for (int j = 0; j < 8; j++) { x.l[j] = p[j]; y.l[j] = p[8 + j]; }
    if (e >> 31) y = m_sub<F_Q>(u_zero(), y);
    return j_madd_inl(acc, x, y);
}
// The accumulator of a bucket loop in the 29-bit-limb form.  Bounds (in units of q; "n" = limbs normalised): x < 5.2 n, y < 3.3 n, z < 1.3 n.
struct jac29 { f29 x, y, z; bool ident; };
GL_DEV jac jac29_lower(const jac29& p) {                            // -> the R = 2^256 Jacobian form of the reduction kernels
    if (p.ident) return j_identity();
    jac r;
    r.x = f29_lower(p.x); r.y = f29_lower(p.y); r.z = f29_lower(p.z);
    return r;
}
// the rare branch: the bucket's sum and the point share their x.  Equal points: the sum is twice the AFFINE point (a = 0 curve:
// XX = x^2, YY = y^2, S = 2 ((x + YY)^2 - XX - YY^2), M = 3 XX, X3 = M^2 - 2 S, Y3 = M (S - X3) - 8 YY^2, Z3 = 2 y), in the same lazy form with
// a product by one wherever a bound would pass what the lent constants cover; opposite points: the identity.
GL_DEV void jac29_same_x(jac29& acc, const f29& x2, const f29& y2, bool equal) {
    if (!equal) { acc.ident = true; return; }
    const f29 one = f29_const(FQ29_ONE);
    const f29 xx = f29_mul(x2, x2), yy = f29_mul(y2, y2), yyyy = f29_mul(yy, yy);
    const f29 t = f29_norm(f29_add(x2, yy));
    const f29 s0 = f29_norm(f29_sub(f29_mul(t, t), f29_norm(f29_add(xx, yyyy)), FQ29_C4));          // < 5.1
    const f29 sv = f29_mul(f29_norm(f29_add(s0, s0)), one);                                             // S < 1.1
    const f29 mv = f29_norm(f29_add(xx, f29_add(xx, xx)));                                              // M < 3.1
    const f29 x3 = f29_norm(f29_sub(f29_mul(mv, mv), f29_norm(f29_add(sv, sv)), FQ29_C4));            // < 5.1
    const f29 y4 = f29_norm(f29_add(f29_norm(f29_add(yyyy, yyyy)), f29_norm(f29_add(yyyy, yyyy))));    // 4 YY^2 < 4.2
    f29 y3 = f29_mul(f29_sub(sv, x3, FQ29_C8), mv);
    y3 = f29_norm(f29_sub(y3, y4, FQ29_C8));
    y3 = f29_norm(f29_sub(y3, y4, FQ29_C8));                                                            // < 17.3
    acc.x = x3; acc.y = f29_mul(y3, one); acc.z = f29_mul(f29_norm(f29_add(y2, y2)), one);
}
// acc += (x2, +-y2): 11 products, sums and differences without carries, five re-normalisations
GL_DEV void msm_add_point29(const uint32_t* pm, jac29& acc, uint32_t e) {
    const uint32_t* p = pm + 16ull * (e & 0x7fffffffu);
    u256 x8, y8;
#pragma unroll
    for (int j = 0; j < 8; j++) { x8.l[j] = p[j]; y8.l[j] = p[8 + j]; }
    const f29 x2 = f29_from_u256(x8);
    f29 y2 = f29_from_u256(y8);                                      // < q, n
    if (e >> 31) y2 = f29_norm(f29_neg(y2, FQ29_C2));                 // 2 q - y < 2 q, n
    if (acc.ident) { acc.x = x2; acc.y = y2; acc.z = f29_const(FQ29_ONE); acc.ident = false; return; }
    const f29 z1z1 = f29_mul(acc.z, acc.z);
    const f29 u2 = f29_mul(x2, z1z1), s2 = f29_mul(f29_mul(y2, acc.z), z1z1);
    const f29 h = f29_norm(f29_sub(u2, acc.x, FQ29_C8));            // < 9.3, n
    const f29 h2 = f29_mul(h, h);
    const f29 r = f29_norm(f29_sub(s2, acc.y, FQ29_C4));            // < 5.3, n
    if (f29_is_zero_mod(h2)) { jac29_same_x(acc, x2, y2, f29_is_zero_mod(f29_mul(r, r))); return; }
    const f29 h3 = f29_mul(h2, h), v = f29_mul(acc.x, h2);
    const f29 w = f29_norm(f29_add(h3, f29_add(v, v)));              // h^3 + 2 v < 3.9, n
    const f29 x3 = f29_norm(f29_sub(f29_mul(r, r), w, FQ29_C4));     // < 5.3, n
    const f29 m1 = f29_mul(f29_sub(v, x3, FQ29_C8), r);              // (v + 8 q - x3 < 9.3) r
    const f29 y3 = f29_norm(f29_sub(m1, f29_mul(acc.y, h3), FQ29_C2));   // < 3.3, n
    acc.z = f29_mul(acc.z, h);
    acc.x = x3; acc.y = y3;
}
// ---- Jacobian + Jacobian and doubling in the same form, for the reduction levels (chains of dependent additions on few lanes: the regime
// where the inlined 29-bit product is twice the called asm one).  Coordinates stay below 12 q with normalised limbs: inputs (X, Y, Z) < 12 q
// give X3 < 5.2, Y3 < 3.3, Z3 < 1.1 (addition) and X3 < 9.3, Y3 < 1.2, Z3 < 3.8 (doubling: Z3 = 2 (Y Z / 2^261 + q), < 2.1 for the Y < 3.3,
// Z < 2.2 these formulas and the lifted items give the levels).
GL_DEV void jac29_double(jac29& p) {
    if (p.ident) return;
    const f29 one = f29_const(FQ29_ONE);
    const f29 A = f29_mul(p.x, p.x), B = f29_mul(p.y, p.y), C = f29_mul(B, B);
    const f29 t = f29_norm(f29_add(p.x, B));
    const f29 d0 = f29_norm(f29_sub(f29_mul(t, t), f29_norm(f29_add(A, C)), FQ29_C4));        // (X + B)^2 - A - C < 6.2
    const f29 dr = f29_mul(d0, one);
    const f29 D = f29_norm(f29_add(dr, dr));                                                     // < 2.1
    const f29 E = f29_norm(f29_add(A, f29_add(A, A)));                                           // < 5.6
    const f29 x3 = f29_norm(f29_sub(f29_mul(E, E), f29_norm(f29_add(D, D)), FQ29_C8));          // < 9.3
    const f29 c4 = f29_norm(f29_add(f29_norm(f29_add(C, C)), f29_norm(f29_add(C, C))));          // 4 C < 4.1
    f29 y3 = f29_mul(f29_sub(D, x3, FQ29_C16), E);                                               // (D + 16 q - X3 < 18.2) E
    y3 = f29_norm(f29_sub(y3, c4, FQ29_C8));
    y3 = f29_norm(f29_sub(y3, c4, FQ29_C8));                                                     // < 17.7
    const f29 yz = f29_mul(p.y, p.z);
    p.x = x3; p.y = f29_mul(y3, one); p.z = f29_norm(f29_add(yz, yz));
}
GL_DEV void jac29_add(jac29& p, const jac29& q) {
    if (q.ident) return;
    if (p.ident) { p = q; return; }
    const f29 z1z1 = f29_mul(p.z, p.z), z2z2 = f29_mul(q.z, q.z);
    const f29 u1 = f29_mul(p.x, z2z2), u2 = f29_mul(q.x, z1z1);
    const f29 s1 = f29_mul(p.y, f29_mul(q.z, z2z2)), s2 = f29_mul(q.y, f29_mul(p.z, z1z1));
    const f29 h = f29_norm(f29_sub(u2, u1, FQ29_C2)), r = f29_norm(f29_sub(s2, s1, FQ29_C2));
    const f29 h2 = f29_mul(h, h);
    if (f29_is_zero_mod(h2)) {                                       // the same x: twice the point, or the identity
        if (f29_is_zero_mod(f29_mul(r, r))) jac29_double(p); else p.ident = true;
        return;
    }
    const f29 h3 = f29_mul(h2, h), v = f29_mul(u1, h2);
    const f29 w = f29_norm(f29_add(h3, f29_add(v, v)));
    const f29 x3 = f29_norm(f29_sub(f29_mul(r, r), w, FQ29_C4));
    const f29 m1 = f29_mul(f29_sub(v, x3, FQ29_C8), r);
    p.y = f29_norm(f29_sub(m1, f29_mul(s1, h3), FQ29_C2));
    p.z = f29_mul(f29_mul(p.z, q.z), h);
    p.x = x3;
}
GL_DEV jac29 jac29_lift(const jac& p) {                              // the 8 x 32-bit R-domain point in this form (three products)
    jac29 r;
    r.ident = j_is_identity(p);
    if (!r.ident) { r.x = f29_lift_inl(p.x); r.y = f29_lift_inl(p.y); r.z = f29_lift_inl(p.z); }
    return r;
}
// ---- the bucket loops' accumulator in XYZZ coordinates (x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2): the mixed addition is 10 products where the Jacobian one is
// 11 -- ZZ and ZZZ are kept instead of being rebuilt from Z (z^2, y2 z) at every step.  madd-2008-s: U2 = x2 ZZ, S2 = y2 ZZZ, P = U2 - X, R = S2 - Y,
// PP = P^2, PPP = P PP, Q = X PP, X3 = R^2 - PPP - 2 Q, Y3 = R (Q - X3) - Y PPP, ZZ3 = ZZ PP, ZZZ3 = ZZZ PPP; the sums and differences carry the bounds of the
// Jacobian form above (P < 9.3, R < 5.3, X3 < 5.3, Y3 < 3.3; ZZ, ZZZ are products: < 1.3).  A finished sum leaves as the Jacobian point (X ZZ, Y ZZZ, ZZ).
struct xyzz29 { f29 x, y, zz, zzz; bool ident; };
GL_DEV jac msm_xyzz_lower(const xyzz29& p) {
    if (p.ident) return j_identity();
    jac r;
    r.x = f29_lower(f29_mul(p.x, p.zz)); r.y = f29_lower(f29_mul(p.y, p.zzz)); r.z = f29_lower(p.zz);
    return r;
}
GL_DEV void msm_add_point_xyzz(const uint32_t* pm, xyzz29& acc, uint32_t e) {
    const uint32_t* p = pm + 16ull * (e & 0x7fffffffu);
    u256 x8, y8;
#pragma unroll
    for (int j = 0; j < 8; j++) { x8.l[j] = p[j]; y8.l[j] = p[8 + j]; }
    const f29 x2 = f29_from_u256(x8);
    f29 y2 = f29_from_u256(y8);                                      // < q, n
    if (e >> 31) y2 = f29_norm(f29_neg(y2, FQ29_C2));                 // 2 q - y < 2 q, n
    if (acc.ident) { acc.x = x2; acc.y = y2; acc.zz = f29_const(FQ29_ONE); acc.zzz = acc.zz; acc.ident = false; return; }
    const f29 u2 = f29_mul(x2, acc.zz), s2 = f29_mul(y2, acc.zzz);
    const f29 h = f29_norm(f29_sub(u2, acc.x, FQ29_C8));            // P < 9.3, n
    const f29 h2 = f29_mul(h, h);
    const f29 r = f29_norm(f29_sub(s2, acc.y, FQ29_C4));            // R < 5.3, n
    if (f29_is_zero_mod(h2)) {                                       // the same x: twice the affine point, or the identity (rare)
        jac29 t;
        t.ident = false;
        jac29_same_x(t, x2, y2, f29_is_zero_mod(f29_mul(r, r)));
        if (t.ident) { acc.ident = true; return; }
        acc.x = t.x; acc.y = t.y; acc.zz = f29_mul(t.z, t.z); acc.zzz = f29_mul(acc.zz, t.z);
        return;
    }
    const f29 h3 = f29_mul(h2, h), v = f29_mul(acc.x, h2);
    const f29 w = f29_norm(f29_add(h3, f29_add(v, v)));              // PPP + 2 Q < 3.9, n
    const f29 x3 = f29_norm(f29_sub(f29_mul(r, r), w, FQ29_C4));     // < 5.3, n
    const f29 m1 = f29_mul(f29_sub(v, x3, FQ29_C8), r);              // (Q + 8 q - X3 < 9.3) R
    const f29 y3 = f29_norm(f29_sub(m1, f29_mul(acc.y, h3), FQ29_C2));   // < 3.3, n
    acc.zz = f29_mul(acc.zz, h2);
    acc.zzz = f29_mul(acc.zzz, h3);
    acc.x = x3; acc.y = y3;
}
}  // namespace gl355
