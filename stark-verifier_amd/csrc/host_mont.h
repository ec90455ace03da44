// The host's BN254 prime fields: bn256::Fr and bn256::Fq as the two instantiations of one class.  4 x 64-bit limbs, Montgomery form with
// R = 2^256 -- the representation the kernels keep in HBM, so a value crosses the boundary as 32 bytes without conversion -- CIOS on
// unsigned __int128.  Fr: challenges, the Keccak transcript (host_fr.h), the verifier, the witness tape, the BN254-Poseidon sponge and the
// handful of scalars around every FFT / KZG launch.  Fq: the host end of the MSM, the pairing and G1 validation (host_fq.h).
// Plain C++17 with no HIP in it: the .hip units include it in both passes, a test program includes it alone.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bn254_curve_tables.h"

namespace gl355 {

// P: MOD (the prime m), N0INV (-m^-1 mod 2^64), R2 (R^2 mod m), ONE (R mod m); ROOT and S where root_of_unity is called
template <class P>
struct Mont {
    uint64_t l[4];          // Montgomery form, canonical (< m)
    typedef unsigned __int128 u128;
    static const uint64_t* M() { return P::MOD; }
    static bool geq_m(const uint64_t a[4]) {
        for (int i = 3; i >= 0; i--) { if (a[i] > M()[i]) return true; if (a[i] < M()[i]) return false; }
        return true;
    }
    static void sub_m(uint64_t a[4]) {
        u128 br = 0;
        for (int i = 0; i < 4; i++) { const u128 d = (u128)a[i] - M()[i] - (uint64_t)br; a[i] = (uint64_t)d; br = (d >> 64) & 1; }
    }
    static Mont zero() { Mont r; memset(r.l, 0, 32); return r; }
    static Mont one() { Mont r; memcpy(r.l, P::ONE, 32); return r; }
    static Mont mont_mul(const Mont& a, const Mont& b) {       // a b R^-1 mod m: canonical for a b < R m (one operand may be any 256-bit word string)
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; i++) {
            u128 c = 0;
            for (int j = 0; j < 4; j++) { c += (u128)a.l[j] * b.l[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
            c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
            const uint64_t m = t[0] * P::N0INV;
            c = ((u128)m * M()[0] + t[0]) >> 64;
            for (int j = 1; j < 4; j++) { c += (u128)m * M()[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
            c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
        }
        Mont r = {{t[0], t[1], t[2], t[3]}};
        if (t[4] || geq_m(r.l)) sub_m(r.l);
        return r;
    }
    // any 256-bit integer (little-endian limbs) -> the field element
    static Mont from_words(const uint64_t w[4]) {
        Mont r2; memcpy(r2.l, P::R2, 32);
        return mont_mul(from_mont_words(w), r2);
    }
    static Mont from_u64(uint64_t v) { const uint64_t w[4] = {v, 0, 0, 0}; return from_words(w); }
    // Montgomery words as the kernels store them (possibly lazily reduced, < 2m; any 256-bit word string is accepted) -> canonical
    static Mont from_mont_words(const uint64_t w[4]) { Mont a; memcpy(a.l, w, 32); while (geq_m(a.l)) sub_m(a.l); return a; }
    void to_words(uint64_t w[4]) const { Mont o = {{1, 0, 0, 0}}; const Mont r = mont_mul(*this, o); memcpy(w, r.l, 32); }
    Mont operator*(const Mont& b) const { return mont_mul(*this, b); }
    Mont operator+(const Mont& b) const {
        Mont r; u128 c = 0;
        for (int i = 0; i < 4; i++) { c += (u128)l[i] + b.l[i]; r.l[i] = (uint64_t)c; c >>= 64; }
        if (c || geq_m(r.l)) sub_m(r.l);          // m < 2^254: the sum of two canonical values never carries out of 256 bits
        return r;
    }
    Mont operator-(const Mont& b) const {
        Mont r; u128 br = 0;
        for (int i = 0; i < 4; i++) { const u128 d = (u128)l[i] - b.l[i] - (uint64_t)br; r.l[i] = (uint64_t)d; br = (d >> 64) & 1; }
        if (br) { u128 c = 0; for (int i = 0; i < 4; i++) { c += (u128)r.l[i] + M()[i]; r.l[i] = (uint64_t)c; c >>= 64; } }
        return r;
    }
    Mont neg() const { return zero() - *this; }
    bool is_zero() const { return (l[0] | l[1] | l[2] | l[3]) == 0; }
    bool operator==(const Mont& b) const { return memcmp(l, b.l, 32) == 0; }
    bool operator!=(const Mont& b) const { return !(*this == b); }
    Mont pow(const uint64_t e[4]) const {
        Mont r = one();
        for (int i = 255; i >= 0; i--) {
            r = r * r;
            if ((e[i >> 6] >> (i & 63)) & 1) r = r * *this;
        }
        return r;
    }
    Mont pow_u64(uint64_t e) const { const uint64_t w[4] = {e, 0, 0, 0}; return pow(w); }
    Mont inv() const { const uint64_t e[4] = {M()[0] - 2, M()[1], M()[2], M()[3]}; return pow(e); }       // a^(m-2); inv(0) = 0
    // canonical integer comparison (the order halo2curves' Ord gives Fr and BTreeSet iterates in)
    bool less_than(const Mont& b) const {
        uint64_t x[4], y[4];
        to_words(x); b.to_words(y);
        for (int i = 3; i >= 0; i--) { if (x[i] != y[i]) return x[i] < y[i]; }
        return false;
    }
    // a primitive 2^log_n-th root of unity, log_n <= P::S (the scalar field only)
    static Mont root_of_unity(uint32_t log_n) {
        Mont w = from_words(P::ROOT);
        for (uint32_t k = log_n; k < P::S; k++) w = w * w;
        return w;
    }
};

struct FrParams {
    static constexpr const uint64_t* MOD = BN254C_FR_MOD_64;
    static constexpr const uint64_t* R2 = BN254C_FR_R2_64;
    static constexpr const uint64_t* ONE = BN254C_FR_ONE_64;
    static constexpr uint64_t N0INV = BN254C_FR_N0INV_64;
    static constexpr const uint64_t* ROOT = BN254C_FR_ROOT_64;
    static constexpr uint32_t S = BN254C_FR_S;
};
struct FqParams {
    static constexpr const uint64_t* MOD = BN254C_FQ_MOD_64;
    static constexpr const uint64_t* R2 = BN254C_FQ_R2_64;
    static constexpr const uint64_t* ONE = BN254C_FQ_ONE_64;
    static constexpr uint64_t N0INV = BN254C_FQ_N0INV_64;
};
typedef Mont<FrParams> Fr;
typedef Mont<FqParams> Fq;

}  // namespace gl355
