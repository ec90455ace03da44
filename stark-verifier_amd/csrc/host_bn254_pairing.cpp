// The BN254 optimal ate pairing on the host: what halo2_proofs' verify_proof ends in (VerifierSHPLONK + SingleStrategy,
// the check the reference runs on every finalisation proof, chip/native_chip/test_utils.rs:82-93) and what Ethereum's EIP-197 precompile
// computes.  One proof, or one batch of any size, needs two Miller loops and one final exponentiation -- milliseconds on one core, with
// nothing to run in parallel -- so there is no device code here.
//
// Tower over host_mont.h's Montgomery Fq:  Fq2 = Fq[u] / (u^2 + 1),  Fq6 = Fq2[v] / (v^3 - xi),  Fq12 = Fq6[w] / (w^2 - v),  xi = 9 + u, so w^6 = xi.
// G2 is the order-r subgroup of the twist E': y^2 = x^3 + 3 / xi over Fq2; (x', y') -> (x' w^2, y' w^3) maps it into E(Fq12).
// Miller loop: f_{6x+2,Q}(P), x = 4965661367192848881, with T kept affine (one Fq2 inversion per step), then the two lines through
// pi(Q) and -pi^2(Q); a line through twist points T, T2 with twist slope l, evaluated at P = (xP, yP) in E(Fq):
//     yP  -  l xP w  +  (l xT - yT) w^3          (vertical lines lie in a proper subfield and die in the final exponentiation)
// Final exponentiation: f^((q^6 - 1)(q^2 + 1)) by one inversion, a conjugation and a q^2-Frobenius, then the hard part
// (q^4 - q^2 + 1) / r by square-and-multiply over its 761 bits.  The Frobenius constants are powers of xi^((q - 1) / 6), computed once.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/gl355.h"
#include "host_fq.h"
#include "host_pairing.h"

namespace gl355 {
using namespace hostfq;

// Ethereum's / halo2curves' generator of G2 (include/gl355.h), x.c0 | x.c1 | y.c0 | y.c1
const uint64_t BN254_G2_GENERATOR[16] = {
    0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull,
    0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull,
    0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull,
    0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull};

namespace {

// ---- Fq2 ---------------------------------------------------------------------------------------------------------------------------
struct Fq2 { Fq c0, c1; };
Fq2 operator+(const Fq2& a, const Fq2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
Fq2 operator-(const Fq2& a, const Fq2& b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
Fq2 operator-(const Fq2& a) { return {a.c0.neg(), a.c1.neg()}; }
Fq2 operator*(const Fq2& a, const Fq2& b) {            // Karatsuba over u^2 = -1
    const Fq t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    return {t0 - t1, (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
}
Fq2 sqr(const Fq2& a) {
    const Fq t = a.c0 * a.c1;
    return {(a.c0 + a.c1) * (a.c0 - a.c1), t + t};
}
Fq2 scale(const Fq2& a, const Fq& s) { return {a.c0 * s, a.c1 * s}; }
Fq2 conj(const Fq2& a) { return {a.c0, a.c1.neg()}; }
Fq2 dbl(const Fq2& a) { return a + a; }
bool is_zero(const Fq2& a) { return a.c0.is_zero() && a.c1.is_zero(); }
bool operator==(const Fq2& a, const Fq2& b) { return a.c0 == b.c0 && a.c1 == b.c1; }
Fq2 fq2_zero() { return {Fq::zero(), Fq::zero()}; }
Fq2 fq2_one() { return {Fq::one(), Fq::zero()}; }
Fq2 inv(const Fq2& a) {                                 // conj(a) / (c0^2 + c1^2); inv(0) = 0
    const Fq n = (a.c0 * a.c0 + a.c1 * a.c1).inv();
    return {a.c0 * n, (a.c1 * n).neg()};
}
Fq2 mul_xi(const Fq2& a) {                              // (c0 + c1 u)(9 + u) = (9 c0 - c1) + (9 c1 + c0) u
    auto x9 = [](const Fq& v) { Fq t = v + v; t = t + t; t = t + t; return t + v; };
    return {x9(a.c0) - a.c1, x9(a.c1) + a.c0};
}
Fq2 pow(const Fq2& a, const uint64_t e[4]) {
    Fq2 r = fq2_one();
    for (int i = 255; i >= 0; i--) {
        r = sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = r * a;
    }
    return r;
}

// ---- Fq6, Fq12 ---------------------------------------------------------------------------------------------------------------------
struct Fq6 { Fq2 a0, a1, a2; };
Fq6 operator+(const Fq6& a, const Fq6& b) { return {a.a0 + b.a0, a.a1 + b.a1, a.a2 + b.a2}; }
Fq6 operator-(const Fq6& a, const Fq6& b) { return {a.a0 - b.a0, a.a1 - b.a1, a.a2 - b.a2}; }
Fq6 operator-(const Fq6& a) { return {-a.a0, -a.a1, -a.a2}; }
Fq6 operator*(const Fq6& a, const Fq6& b) {            // Karatsuba (6 Fq2 products), v^3 = xi
    const Fq2 t0 = a.a0 * b.a0, t1 = a.a1 * b.a1, t2 = a.a2 * b.a2;
    return {t0 + mul_xi((a.a1 + a.a2) * (b.a1 + b.a2) - t1 - t2),
            (a.a0 + a.a1) * (b.a0 + b.a1) - t0 - t1 + mul_xi(t2),
            (a.a0 + a.a2) * (b.a0 + b.a2) - t0 - t2 + t1};
}
Fq6 mul_v(const Fq6& a) { return {mul_xi(a.a2), a.a0, a.a1}; }
Fq6 inv(const Fq6& a) {
    const Fq2 t0 = sqr(a.a0) - mul_xi(a.a1 * a.a2), t1 = mul_xi(sqr(a.a2)) - a.a0 * a.a1, t2 = sqr(a.a1) - a.a0 * a.a2;
    const Fq2 d = inv(a.a0 * t0 + mul_xi(a.a2 * t1 + a.a1 * t2));
    return {t0 * d, t1 * d, t2 * d};
}
bool operator==(const Fq6& a, const Fq6& b) { return a.a0 == b.a0 && a.a1 == b.a1 && a.a2 == b.a2; }
Fq6 fq6_zero() { return {fq2_zero(), fq2_zero(), fq2_zero()}; }

struct Fq12 { Fq6 c0, c1; };
Fq12 operator*(const Fq12& a, const Fq12& b) {          // w^2 = v
    const Fq6 t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    return {t0 + mul_v(t1), (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
}
Fq12 sqr(const Fq12& a) { return a * a; }
Fq12 conj(const Fq12& a) { return {a.c0, -a.c1}; }      // a^(q^6)
Fq12 inv(const Fq12& a) {
    const Fq6 d = inv(a.c0 * a.c0 - mul_v(a.c1 * a.c1));
    return {a.c0 * d, -(a.c1 * d)};
}
Fq12 fq12_one() { return {{fq2_one(), fq2_zero(), fq2_zero()}, fq6_zero()}; }
bool operator==(const Fq12& a, const Fq12& b) { return a.c0 == b.c0 && a.c1 == b.c1; }

// ---- constants derived once from q ---------------------------------------------------------------------------------------------------
struct Consts {
    Fq2 b_twist;            // 3 / xi
    Fq2 g12, g13;           // xi^((q-1)/3), xi^((q-1)/2): the q-Frobenius on twist coordinates
    Fq g22;                 // xi^((q^2-1)/3): the q^2-Frobenius on the twist's x (its y changes sign)
    Fq z[6];                // zeta^i, zeta = xi^((q^2-1)/6): the q^2-Frobenius multiplies the coefficient of w^i by zeta^i
    Consts() {
        const uint64_t* Q = Fq::M();
        const Fq2 xi = {Fq::from_u64(9), Fq::one()};
        b_twist = scale(inv(xi), Fq::from_u64(3));
        uint64_t e[4];                                  // (q - 1) / 6
        unsigned __int128 rem = 0;
        for (int i = 3; i >= 0; i--) {
            const unsigned __int128 cur = (rem << 64) | (i == 0 ? Q[0] - 1 : Q[i]);
            e[i] = (uint64_t)(cur / 6);
            rem = cur % 6;
        }
        const Fq2 g11 = pow(xi, e);
        g12 = sqr(g11);
        g13 = g12 * g11;
        g22 = (g12 * conj(g12)).c0;                     // the norm: x^(q+1)
        z[0] = Fq::one();
        z[1] = (g11 * conj(g11)).c0;
        for (int i = 2; i < 6; i++) z[i] = z[i - 1] * z[1];
    }
};
const Consts& K() { static const Consts k; return k; }

Fq12 frobenius2(const Fq12& a) {
    const Consts& k = K();
    return {{a.c0.a0, scale(a.c0.a1, k.z[2]), scale(a.c0.a2, k.z[4])}, {scale(a.c1.a0, k.z[1]), scale(a.c1.a1, k.z[3]), scale(a.c1.a2, k.z[5])}};
}

// (q^4 - q^2 + 1) / r, little-endian words (761 bits)
const uint64_t HARD_EXP[12] = {0xe81bb482ccdf42b1ull, 0x5abf5cc4f49c36d4ull, 0xf1154e7e1da014fdull, 0xdcc7b44c87cdbacfull,
                               0xaaa441e3954bcf8aull, 0x6b887d56d5095f23ull, 0x79581e16f3fd90c6ull, 0x3b1b1355d189227dull,
                               0x4e529a5861876f6bull, 0x6c0eb522d5b12278ull, 0x331ec15183177fafull, 0x01baaa710b0759adull};

Fq12 final_exponentiation(const Fq12& f) {
    Fq12 t = conj(f) * inv(f);                          // f^(q^6 - 1)
    t = frobenius2(t) * t;                              // ^(q^2 + 1)
    Fq12 r = fq12_one();
    bool started = false;
    for (int i = 767; i >= 0; i--) {
        if (started) r = sqr(r);
        if ((HARD_EXP[i >> 6] >> (i & 63)) & 1) { r = started ? r * t : t; started = true; }
    }
    return r;
}

// ---- G2 on the twist ----------------------------------------------------------------------------------------------------------------
struct G2Aff { Fq2 x, y; };
struct G2Jac { Fq2 x, y, z; };
G2Jac g2_identity() { return {fq2_one(), fq2_one(), fq2_zero()}; }
G2Jac g2_double(const G2Jac& p) {                       // a = 0: the formulas of host_fq.h's j_double over Fq2
    if (is_zero(p.z)) return p;
    const Fq2 a = sqr(p.x), b = sqr(p.y), c = sqr(b);
    const Fq2 d = dbl(sqr(p.x + b) - a - c), e = a + a + a, f = sqr(e);
    G2Jac r;
    r.x = f - dbl(d);
    r.y = e * (d - r.x) - dbl(dbl(dbl(c)));
    r.z = dbl(p.y * p.z);
    return r;
}
G2Jac g2_add(const G2Jac& p, const G2Jac& q) {
    if (is_zero(p.z)) return q;
    if (is_zero(q.z)) return p;
    const Fq2 z1z1 = sqr(p.z), z2z2 = sqr(q.z);
    const Fq2 u1 = p.x * z2z2, u2 = q.x * z1z1, s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
    const Fq2 h = u2 - u1, r = s2 - s1;
    if (is_zero(h)) return is_zero(r) ? g2_double(p) : g2_identity();
    const Fq2 h2 = sqr(h), h3 = h2 * h, v = u1 * h2;
    G2Jac o;
    o.x = sqr(r) - h3 - dbl(v);
    o.y = r * (v - o.x) - s1 * h3;
    o.z = p.z * q.z * h;
    return o;
}
G2Jac g2_mul(const G2Jac& p, const uint64_t e[4]) {
    G2Jac r = g2_identity();
    for (int i = 255; i >= 0; i--) {
        r = g2_double(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = g2_add(r, p);
    }
    return r;
}
bool g2_is_identity_words(const uint64_t p[16]) {
    uint64_t o = 0;
    for (int i = 0; i < 16; i++) o |= p[i];
    return o == 0;
}
G2Aff g2_load(const uint64_t p[16]) { return {{Fq::from_words(p), Fq::from_words(p + 4)}, {Fq::from_words(p + 8), Fq::from_words(p + 12)}}; }
void g2_store(const G2Jac& r, uint64_t out[16]) {
    if (is_zero(r.z)) { memset(out, 0, 128); return; }
    const Fq2 zi = inv(r.z), zi2 = sqr(zi), x = r.x * zi2, y = r.y * zi2 * zi;
    x.c0.to_words(out); x.c1.to_words(out + 4); y.c0.to_words(out + 8); y.c1.to_words(out + 12);
}
bool g2_on_twist(const G2Aff& p) { return sqr(p.y) == sqr(p.x) * p.x + K().b_twist; }

// ---- Miller loop ----------------------------------------------------------------------------------------------------------------------
struct Pair { Fq xp, yp; G2Aff q, t; };
Fq12 line(const Pair& pr, const Fq2& slope) {
    Fq12 l;
    l.c0 = {{pr.yp, Fq::zero()}, fq2_zero(), fq2_zero()};
    l.c1 = {-scale(slope, pr.xp), slope * pr.t.x - pr.t.y, fq2_zero()};
    return l;
}
// f <- f * line through T and T (q == nullptr) or T and *q, at P;  T <- the sum
void step(Fq12& f, Pair& pr, const G2Aff* q) {
    const Fq2 slope = q ? (q->y - pr.t.y) * inv(q->x - pr.t.x) : (sqr(pr.t.x) + dbl(sqr(pr.t.x))) * inv(dbl(pr.t.y));
    f = f * line(pr, slope);
    const Fq2 x3 = sqr(slope) - pr.t.x - (q ? q->x : pr.t.x);
    pr.t.y = slope * (pr.t.x - x3) - pr.t.y;
    pr.t.x = x3;
}
Fq12 multi_miller_loop(std::vector<Pair>& pairs) {
    const unsigned __int128 e = (unsigned __int128)6 * 4965661367192848881ull + 2;      // 65 bits
    Fq12 f = fq12_one();
    for (int i = 63; i >= 0; i--) {
        f = sqr(f);
        for (auto& pr : pairs) step(f, pr, nullptr);
        if ((e >> i) & 1) for (auto& pr : pairs) step(f, pr, &pr.q);
    }
    const Consts& k = K();
    for (auto& pr : pairs) {
        const G2Aff q1 = {conj(pr.q.x) * k.g12, conj(pr.q.y) * k.g13};                  // pi(Q)
        const G2Aff q2 = {scale(pr.q.x, k.g22), pr.q.y};                                // -pi^2(Q)
        step(f, pr, &q1);
        step(f, pr, &q2);
    }
    return f;
}

}  // namespace

const char* bn254_g2_invalid(const uint64_t p[16], bool subgroup) {
    if (g2_is_identity_words(p)) return nullptr;
    for (int c = 0; c < 4; c++) if (!words_lt_q(p + 4 * c)) return "a G2 coordinate is not below q";
    const G2Aff a = g2_load(p);
    if (!g2_on_twist(a)) return "a G2 point is not on the twist";
    if (subgroup && !is_zero(g2_mul({a.x, a.y, fq2_one()}, BN254C_FR_MOD_64).z)) return "a G2 point is outside the order-r subgroup";
    return nullptr;
}

bool bn254_pairing_product_is_one(const uint64_t* g1, const uint64_t* g2, uint32_t n) {
    std::vector<Pair> pairs;
    for (uint32_t i = 0; i < n; i++) {
        bool ident1 = true;
        for (int j = 0; j < 8; j++) ident1 = ident1 && g1[8 * i + j] == 0;
        if (ident1 || g2_is_identity_words(g2 + 16 * i)) continue;
        Pair pr;
        pr.xp = Fq::from_words(g1 + 8 * i); pr.yp = Fq::from_words(g1 + 8 * i + 4);
        pr.q = g2_load(g2 + 16 * i); pr.t = pr.q;
        pairs.push_back(pr);
    }
    if (pairs.empty()) return true;
    return final_exponentiation(multi_miller_loop(pairs)) == fq12_one();
}

}  // namespace gl355

using namespace gl355;

extern "C" {

int32_t gl355_bn254_g2_mul(const uint64_t scalar[4], const uint64_t* point, uint64_t out[16]) {
    if (!scalar || !out) return GL355_E_INVALID_ARG;
    if (!point) point = BN254_G2_GENERATOR;
    if (const char* why = bn254_g2_invalid(point, false)) { plonk_verify_set_error(std::string("bn254_g2_mul: ") + why); return GL355_E_INVALID_ARG; }
    if (g2_is_identity_words(point)) { memset(out, 0, 128); return GL355_OK; }
    const G2Aff a = g2_load(point);
    g2_store(g2_mul({a.x, a.y, fq2_one()}, scalar), out);
    return GL355_OK;
}

int32_t gl355_bn254_pairing_check(const uint64_t* g1, const uint64_t* g2, uint32_t n, int32_t* ok) {
    if (!ok || (n && (!g1 || !g2))) return GL355_E_INVALID_ARG;
    *ok = 0;
    for (uint32_t i = 0; i < n; i++) {
        const char* why = bn254_g1_valid_host(g1 + 8 * i) ? nullptr : "the G1 point is non-canonical or off the curve";
        if (!why) why = bn254_g2_invalid(g2 + 16 * i, true);
        if (why) { plonk_verify_set_error("bn254_pairing_check: pair " + std::to_string(i) + ": " + why); return GL355_E_INVALID_ARG; }
    }
    *ok = bn254_pairing_product_is_one(g1, g2, n) ? 1 : 0;
    return GL355_OK;
}

}  // extern "C"
