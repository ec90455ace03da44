// Jacobian G1 arithmetic over the host's bn256::Fq (host_mont.h), and affine points as canonical integers in and out of it: shared by the
// host end of the MSM (host_bn254_curve.cpp), the pairing (host_bn254_pairing.cpp) and the Halo2 verifier (plonk_verifier.cpp).
// Everything is `inline`: each translation unit keeps its own copy.
#pragma once
#include "host_mont.h"

namespace gl355 {
namespace hostfq {
struct Jac { Fq x, y, z; };
inline Jac j_identity() { return {Fq::one(), Fq::one(), Fq::zero()}; }
inline bool j_is_identity(const Jac& p) { return p.z.is_zero(); }
inline Jac j_double(const Jac& p) {                // y^2 = x^3 + 3 (a = 0)
    if (j_is_identity(p)) return p;
    const Fq a = p.x * p.x, b = p.y * p.y, c = b * b;
    const Fq xb = p.x + b;
    Fq d = xb * xb - a - c;
    d = d + d;
    const Fq e = a + a + a, f = e * e;
    Jac r;
    r.x = f - (d + d);
    Fq c8 = c + c; c8 = c8 + c8; c8 = c8 + c8;
    r.y = e * (d - r.x) - c8;
    const Fq yz = p.y * p.z;
    r.z = yz + yz;
    return r;
}
inline Jac j_add(const Jac& p, const Jac& q) {
    if (j_is_identity(p)) return q;
    if (j_is_identity(q)) return p;
    const Fq z1z1 = p.z * p.z, z2z2 = q.z * q.z;
    const Fq u1 = p.x * z2z2, u2 = q.x * z1z1;
    const Fq s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
    const Fq h = u2 - u1, r = s2 - s1;
    if (h.is_zero()) return r.is_zero() ? j_double(p) : j_identity();
    const Fq h2 = h * h, h3 = h2 * h, v = u1 * h2;
    Jac o;
    o.x = r * r - h3 - (v + v);
    o.y = r * (v - o.x) - s1 * h3;
    o.z = p.z * q.z * h;
    return o;
}

inline bool words_lt_q(const uint64_t w[4]) { return !Fq::geq_m(w); }
inline bool g1_words_are_identity(const uint64_t p[8]) {
    uint64_t o = 0;
    for (int i = 0; i < 8; i++) o |= p[i];
    return o == 0;
}
// affine x | y as integers (zeros = the identity; a coordinate at or above q is reduced) <-> Jacobian; g1_load checks nothing
inline Jac g1_load(const uint64_t p[8]) {
    if (g1_words_are_identity(p)) return j_identity();
    return {Fq::from_words(p), Fq::from_words(p + 4), Fq::one()};
}
inline void g1_store(const Jac& r, uint64_t out[8]) {
    if (j_is_identity(r)) { memset(out, 0, 64); return; }
    const Fq zi = r.z.inv(), zi2 = zi * zi;
    (r.x * zi2).to_words(out);
    (r.y * (zi2 * zi)).to_words(out + 4);
}
// canonical coordinates and y^2 = x^3 + 3 (the identity passes)
inline bool g1_valid(const uint64_t p[8]) {
    if (g1_words_are_identity(p)) return true;
    if (!words_lt_q(p) || !words_lt_q(p + 4)) return false;
    const Fq x = Fq::from_words(p), y = Fq::from_words(p + 4);
    return y * y == x * x * x + Fq::from_u64(3);
}
}  // namespace hostfq
}  // namespace gl355
