// Internal interface of the host BN254 pairing (host_bn254_pairing.cpp) and the host G1 multi-scalar multiplication
// (host_bn254_curve.cpp) towards the Halo2 verifier (plonk_verifier.cpp).  Points and scalars cross it as the C ABI's canonical integers.
#pragma once
#include <stdint.h>

#include <string>

namespace gl355 {

extern const uint64_t BN254_G2_GENERATOR[16];

// nullptr if p is the identity or a canonical point of the twist (and, with `subgroup`, of order r); else what is wrong with it
const char* bn254_g2_invalid(const uint64_t p[16], bool subgroup);
// prod_i e(g1[i], g2[i]) == 1 for points the caller has validated (an identity on either side contributes 1)
bool bn254_pairing_product_is_one(const uint64_t* g1 /* n x 8 */, const uint64_t* g2 /* n x 16 */, uint32_t n);
// sum_i scalars[i] points[i] on one core (Pippenger buckets); scalars are any 256-bit integers, points valid affine G1 points
void bn254_g1_msm_host(const uint64_t* points /* n x 8 */, const uint64_t* scalars /* n x 4 */, uint64_t n, uint64_t out[8]);
void bn254_g1_neg_host(const uint64_t p[8], uint64_t out[8]);
bool bn254_g1_valid_host(const uint64_t p[8]);
// the thread's gl355_plonk_verify_last_error text (plonk_verifier.cpp)
void plonk_verify_set_error(const std::string& why);

}  // namespace gl355
