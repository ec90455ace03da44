// The Keccak-256 transcript that halo2-solidity-verifier's Keccak256Transcript defines (chip/native_chip/test_utils.rs:73), over the host's
// bn256::Fr (host_mont.h) -- the sequential side of the Halo2 / KZG prover and verifier.
#pragma once
#include <vector>

#include "host_mont.h"

namespace gl355 {

void keccak256_host(const uint8_t* data, size_t len, uint8_t out[32]);

// halo2-solidity-verifier's Keccak256Transcript (writer side): 32-byte big-endian words into a running buffer and into the proof; a
// challenge = keccak256(buffer) as a big-endian integer mod r, the digest becomes the buffer (plus 0x01 when squeezed twice in a row)
struct KeccakTranscript {
    std::vector<uint8_t> buf, proof;
    static void be32(const uint64_t w[4], uint8_t out[32]) {
        for (int i = 0; i < 4; i++) for (int b = 0; b < 8; b++) out[31 - (8 * i + b)] = (uint8_t)(w[i] >> (8 * b));
    }
    static void from_be32(const uint8_t b[32], uint64_t w[4]) {      // be32's inverse: the one place a 256-bit big-endian integer is read
        for (int i = 0; i < 4; i++) { w[i] = 0; for (int j = 0; j < 8; j++) w[i] |= (uint64_t)b[31 - (8 * i + j)] << (8 * j); }
    }
    void common_scalar(const Fr& s) { uint64_t w[4]; s.to_words(w); uint8_t b[32]; be32(w, b); buf.insert(buf.end(), b, b + 32); }
    void write_scalar(const Fr& s) { uint64_t w[4]; s.to_words(w); uint8_t b[32]; be32(w, b); buf.insert(buf.end(), b, b + 32); proof.insert(proof.end(), b, b + 32); }
    void write_point(const uint64_t xy[8]) {            // affine, canonical integers; all zero = the identity
        uint8_t b[64];
        be32(xy, b); be32(xy + 4, b + 32);
        buf.insert(buf.end(), b, b + 64);
        proof.insert(proof.end(), b, b + 64);
    }
    Fr squeeze_challenge() {
        std::vector<uint8_t> data(buf);
        if (buf.size() == 32) data.push_back(1);
        uint8_t h[32];
        keccak256_host(data.data(), data.size(), h);
        buf.assign(h, h + 32);
        uint64_t w[4];
        from_be32(h, w);
        return Fr::from_words(w);                           // 256-bit big-endian integer mod r
    }
};

}  // namespace gl355
