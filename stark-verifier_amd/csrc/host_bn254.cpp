// Host-side (CPU, sequential) BN254-Poseidon: the one round function both host users run (constants, x^5, dense 5 x 5 MDS --
// src/plonky2_verifier/bn245_poseidon/native.rs:45-62), and the permutation of the 12-element sponge state that the Fiat-Shamir
// Challenger and the circuit digest need when the proof's hasher is the reference's Bn254PoseidonHash
// (bn245_poseidon/plonky2_config.rs:38-75, native.rs:16-77).  About 50 permutations per proof, so it runs on the calling thread like
// the Poseidon-Goldilocks one in host_transcript.cpp; the data-parallel work is in merkle_bn254.hip.  Field: host_mont.h; tables:
// bn254_tables.h, already in its form.
#include "gl355_internal.h"
#include "host_mont.h"

#include "bn254_tables.h"

namespace gl355 {
namespace {

typedef unsigned __int128 u128;

Fr encode3(const uint64_t* x) {          // x0 + x1 p + x2 p^2 (< 2^192)
    uint64_t a[4] = {gl_canon(x[2]), 0, 0, 0};
    for (int step = 1; step >= 0; step--) {
        u128 c = gl_canon(x[step]);
        for (int i = 0; i < 4; i++) { c += (u128)a[i] * GL_P; a[i] = (uint64_t)c; c >>= 64; }
    }
    return Fr::from_words(a);
}
void decode3(const Fr& x, uint64_t* out) {      // the three low base-p digits of the canonical value
    uint64_t a[4];
    x.to_words(a);
    for (int d = 0; d < 3; d++) {
        u128 rem = 0;
        for (int i = 3; i >= 0; i--) {
            const u128 cur = (rem << 64) | a[i];
            a[i] = (uint64_t)(cur / GL_P);
            rem = cur % GL_P;
        }
        out[d] = (uint64_t)rem;
    }
}

}  // namespace

// round rnd of 68 on the state s: the first and last four are full (x^5 on every element), the 60 between them partial (on s[0] only)
void host_bn254_poseidon_round(Fr s[5], int rnd) {
    static const struct Tables {
        Fr rc[340], mds[25];
        Tables() {
            for (int i = 0; i < 340; i++) memcpy(rc[i].l, BN254_RC[i], 32);
            for (int i = 0; i < 25; i++) memcpy(mds[i].l, BN254_MDS[i], 32);
        }
    } T;   // C++11 magic static: initialised once, thread-safe
    const bool full = rnd < 4 || rnd >= 64;
    for (int i = 0; i < 5; i++) {
        s[i] = s[i] + T.rc[5 * rnd + i];
        if (full || i == 0) { const Fr x2 = s[i] * s[i]; s[i] = x2 * x2 * s[i]; }
    }
    Fr n[5];
    for (int i = 0; i < 5; i++) {
        Fr acc = s[0] * T.mds[5 * i];
        for (int j = 1; j < 5; j++) acc = acc + s[j] * T.mds[5 * i + j];
        n[i] = acc;
    }
    memcpy(s, n, sizeof n);
}

void host_bn254_permute(uint64_t s[12]) {
    Fr st[5];
    for (int i = 0; i < 4; i++) st[i] = encode3(s + 3 * i);
    st[4] = Fr::zero();
    for (int rnd = 0; rnd < 68; rnd++) host_bn254_poseidon_round(st, rnd);
    for (int i = 0; i < 4; i++) decode3(st[i], s + 3 * i);
}

}  // namespace gl355
