// Host end of the bn256::G1 multi-scalar multiplication (halo2 `best_multiexp`, reached from the reference at
// src/plonky2_verifier/verifier_api.rs:77-92): the combination of the per-window sums
//     result = sum_w 2^(c w) W_w          (Horner from the top window: 254 dependent doublings)
// and the conversion to an affine point.  It is strictly sequential -- 270 group operations of ~10 k VALU instructions each are
// ~4 ms on one GPU lane (what the first version did) and ~0.1 ms here on one host core with 64-bit limbs.
// Fq arithmetic: host_mont.h (the representation the kernels store); the point formulas: host_fq.h.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "host_fq.h"
#include "host_pairing.h"

namespace gl355 {
using namespace hostfq;
namespace {
Fq load_fq(const uint32_t* p) {
    uint64_t w[4];
    for (int i = 0; i < 4; i++) w[i] = (uint64_t)p[2 * i] | ((uint64_t)p[2 * i + 1] << 32);
    return Fq::from_mont_words(w);
}
Jac load_jac(const uint32_t* p) { return {load_fq(p), load_fq(p + 8), load_fq(p + 16)}; }
}  // namespace

// s, wt: n_windows Jacobian points each as the kernels store them (x | y | z, 8 x 32-bit limbs each, Montgomery form, < 2q); the sum
// of window w is s[w] + wt[w] (bucket j weighs j + 1); wt may be null (a window of one bucket)
void bn254_g1_horner_host(const uint32_t* s, const uint32_t* wt, uint32_t n_windows, uint32_t c, uint64_t result[8]) {
    Jac r = j_identity();
    for (uint32_t w = n_windows; w-- > 0;) {
        for (uint32_t k = 0; k < c; k++) r = j_double(r);
        r = j_add(r, load_jac(s + 24 * w));
        if (wt) r = j_add(r, load_jac(wt + 24 * w));
    }
    g1_store(r, result);
}

// out = a + b for affine points as integers (x | y, zeros = the identity; g1_load reduces a coordinate at or above q): the host end of a
// commitment made in two parts
void bn254_g1_add_host(const uint64_t a[8], const uint64_t b[8], uint64_t out[8]) { g1_store(j_add(g1_load(a), g1_load(b)), out); }

// sum_i scalars[i] points[i] on one core: the verifier's MSM over a proof's ~150 commitments, and the batch verifier's below the size
// where a device launch pays.  Pippenger buckets over unsigned c-bit digits; windows above the longest scalar are never built (the batch
// verifier's 128-bit weights).
void bn254_g1_msm_host(const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t out[8]) {
    uint32_t bits = 0;
    for (uint64_t i = 0; i < n; i++)
        for (int l = 3; l >= 0; l--) if (scalars[4 * i + l]) { bits = std::max<uint32_t>(bits, 64 * l + 64 - (uint32_t)__builtin_clzll(scalars[4 * i + l])); break; }
    uint32_t lg = 0;
    while ((2ull << lg) <= n) lg++;
    const uint32_t c = std::min(14u, std::max(2u, lg > 1 ? lg - 1 : 2u));
    const uint32_t n_windows = (bits + c - 1) / c;
    std::vector<Jac> pts(n);
    for (uint64_t i = 0; i < n; i++) pts[i] = g1_load(points + 8 * i);
    std::vector<Jac> buckets((size_t)1 << c);
    Jac acc = j_identity();
    for (uint32_t w = n_windows; w-- > 0;) {
        for (uint32_t k = 0; k < c; k++) acc = j_double(acc);
        for (auto& b : buckets) b = j_identity();
        const uint32_t lo = w * c;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t* sc = scalars + 4 * i;
            uint64_t d = sc[lo >> 6] >> (lo & 63);
            if ((lo & 63) + c > 64 && (lo >> 6) + 1 < 4) d |= sc[(lo >> 6) + 1] << (64 - (lo & 63));
            d &= (1ull << c) - 1;
            if (d) buckets[d] = j_add(buckets[d], pts[i]);
        }
        Jac run = j_identity(), sum = j_identity();
        for (size_t j = buckets.size(); j-- > 1;) { run = j_add(run, buckets[j]); sum = j_add(sum, run); }
        acc = j_add(acc, sum);
    }
    g1_store(acc, out);
}

void bn254_g1_neg_host(const uint64_t p[8], uint64_t out[8]) {
    if (g1_words_are_identity(p)) { memset(out, 0, 64); return; }
    memcpy(out, p, 32);
    Fq::from_words(p + 4).neg().to_words(out + 4);
}

bool bn254_g1_valid_host(const uint64_t p[8]) { return g1_valid(p); }

}  // namespace gl355
