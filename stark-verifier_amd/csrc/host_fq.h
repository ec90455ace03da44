// Host-side bn256::Fq (4 x 64-bit limbs, Montgomery form with R = 2^256 -- the representation the MSM kernels store -- CIOS on unsigned
// __int128) and Jacobian G1 arithmetic over it: shared by the host end of the MSM (host_bn254_curve.cpp), the pairing
// (host_bn254_pairing.cpp) and the Halo2 verifier (plonk_verifier.cpp).  Everything is `inline`: each translation unit keeps its own copy.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bn254_curve_tables.h"

namespace gl355 {
namespace hostfq {
typedef unsigned __int128 u128;
struct Fq { uint64_t l[4]; };
static const uint64_t* const Q = BN254C_FQ_MOD_64;

inline bool geq_q(const Fq& a) {
    for (int i = 3; i >= 0; i--) { if (a.l[i] > Q[i]) return true; if (a.l[i] < Q[i]) return false; }
    return true;
}
inline void sub_q(Fq& a) {
    u128 br = 0;
    for (int i = 0; i < 4; i++) { const u128 d = (u128)a.l[i] - Q[i] - (uint64_t)br; a.l[i] = (uint64_t)d; br = (d >> 64) & 1; }
}
inline Fq fq_canon(Fq a) { while (geq_q(a)) sub_q(a); return a; }      // the kernels keep values lazily below 2q
inline Fq fq_add(const Fq& a, const Fq& b) {
    Fq r; u128 c = 0;
    for (int i = 0; i < 4; i++) { c += (u128)a.l[i] + b.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
    if (c || geq_q(r)) sub_q(r);          // q < 2^254: the sum of two canonical values never carries out of 256 bits
    return r;
}
inline Fq fq_sub(const Fq& a, const Fq& b) {
    Fq r; u128 br = 0;
    for (int i = 0; i < 4; i++) { const u128 d = (u128)a.l[i] - b.l[i] - (uint64_t)br; r.l[i] = (uint64_t)d; br = (d >> 64) & 1; }
    if (br) { u128 c = 0; for (int i = 0; i < 4; i++) { c += (u128)r.l[i] + Q[i]; r.l[i] = (uint64_t)c; c >>= 64; } }
    return r;
}
inline Fq fq_mul(const Fq& a, const Fq& b) {       // a b R^-1 mod q, canonical operands and result
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) { c += (u128)a.l[j] * b.l[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * BN254C_FQ_N0INV_64;
        c = ((u128)m * Q[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) { c += (u128)m * Q[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fq r = {{t[0], t[1], t[2], t[3]}};
    if (t[4] || geq_q(r)) sub_q(r);
    return r;
}
inline bool fq_is_zero(const Fq& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
inline Fq fq_one() { Fq r; memcpy(r.l, BN254C_FQ_ONE_64, 32); return r; }
inline Fq fq_inv(const Fq& a) {                    // a^(q-2)
    uint64_t e[4] = {Q[0] - 2, Q[1], Q[2], Q[3]};
    Fq r = fq_one();
    for (int i = 255; i >= 0; i--) {
        r = fq_mul(r, r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = fq_mul(r, a);
    }
    return r;
}
struct Jac { Fq x, y, z; };
inline bool j_is_identity(const Jac& p) { return fq_is_zero(p.z); }
inline Jac j_double(const Jac& p) {                // y^2 = x^3 + 3 (a = 0)
    if (j_is_identity(p)) return p;
    const Fq a = fq_mul(p.x, p.x), b = fq_mul(p.y, p.y), c = fq_mul(b, b);
    const Fq xb = fq_add(p.x, b);
    Fq d = fq_sub(fq_sub(fq_mul(xb, xb), a), c);
    d = fq_add(d, d);
    const Fq e = fq_add(fq_add(a, a), a), f = fq_mul(e, e);
    Jac r;
    r.x = fq_sub(f, fq_add(d, d));
    Fq c8 = fq_add(c, c); c8 = fq_add(c8, c8); c8 = fq_add(c8, c8);
    r.y = fq_sub(fq_mul(e, fq_sub(d, r.x)), c8);
    const Fq yz = fq_mul(p.y, p.z);
    r.z = fq_add(yz, yz);
    return r;
}
inline Jac j_add(const Jac& p, const Jac& q) {
    if (j_is_identity(p)) return q;
    if (j_is_identity(q)) return p;
    const Fq z1z1 = fq_mul(p.z, p.z), z2z2 = fq_mul(q.z, q.z);
    const Fq u1 = fq_mul(p.x, z2z2), u2 = fq_mul(q.x, z1z1);
    const Fq s1 = fq_mul(fq_mul(p.y, q.z), z2z2), s2 = fq_mul(fq_mul(q.y, p.z), z1z1);
    const Fq h = fq_sub(u2, u1), r = fq_sub(s2, s1);
    if (fq_is_zero(h)) {
        if (fq_is_zero(r)) return j_double(p);
        Jac id; id.x = fq_one(); id.y = id.x; memset(id.z.l, 0, 32);
        return id;
    }
    const Fq h2 = fq_mul(h, h), h3 = fq_mul(h2, h), v = fq_mul(u1, h2);
    Jac o;
    o.x = fq_sub(fq_sub(fq_mul(r, r), h3), fq_add(v, v));
    o.y = fq_sub(fq_mul(r, fq_sub(v, o.x)), fq_mul(s1, h3));
    o.z = fq_mul(fq_mul(p.z, q.z), h);
    return o;
}

inline Jac j_identity() { Jac id; id.x = fq_one(); id.y = id.x; memset(id.z.l, 0, 32); return id; }
// canonical integer (4 words, < q) <-> Montgomery form
inline Fq fq_from_int(const uint64_t w[4]) { Fq x, r2; memcpy(x.l, w, 32); memcpy(r2.l, BN254C_FQ_R2_64, 32); return fq_mul(x, r2); }
inline void fq_to_int(const Fq& a, uint64_t w[4]) { Fq o; memset(o.l, 0, 32); o.l[0] = 1; const Fq r = fq_mul(a, o); memcpy(w, r.l, 32); }
inline Fq fq_neg(const Fq& a) { Fq z; memset(z.l, 0, 32); return fq_sub(z, a); }
inline bool fq_eq(const Fq& a, const Fq& b) { return memcmp(a.l, b.l, 32) == 0; }
inline bool words_lt_q(const uint64_t w[4]) { Fq a; memcpy(a.l, w, 32); return !geq_q(a); }
// affine x | y as canonical integers (zeros = the identity) <-> Jacobian; g1_load checks nothing
inline Jac g1_load(const uint64_t p[8]) {
    bool ident = true;
    for (int i = 0; i < 8; i++) ident = ident && p[i] == 0;
    if (ident) return j_identity();
    Jac r; r.x = fq_from_int(p); r.y = fq_from_int(p + 4); r.z = fq_one();
    return r;
}
inline void g1_store(const Jac& r, uint64_t out[8]) {
    if (j_is_identity(r)) { memset(out, 0, 64); return; }
    const Fq zi = fq_inv(r.z), zi2 = fq_mul(zi, zi);
    fq_to_int(fq_mul(r.x, zi2), out);
    fq_to_int(fq_mul(r.y, fq_mul(zi2, zi)), out + 4);
}
// canonical coordinates and y^2 = x^3 + 3 (the identity passes)
inline bool g1_valid(const uint64_t p[8]) {
    bool ident = true;
    for (int i = 0; i < 8; i++) ident = ident && p[i] == 0;
    if (ident) return true;
    if (!words_lt_q(p) || !words_lt_q(p + 4)) return false;
    const Fq x = fq_from_int(p), y = fq_from_int(p + 4);
    const uint64_t three[4] = {3, 0, 0, 0};
    return fq_eq(fq_mul(y, y), fq_add(fq_mul(fq_mul(x, x), x), fq_from_int(three)));
}
}  // namespace hostfq
}  // namespace gl355
