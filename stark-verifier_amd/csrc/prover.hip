// FRI prover loop in one call (a12 + a13 + a14 of SURVEY.md 8): commit phase, proof of work and the
// layer openings of every query, with the polynomial resident on the device throughout: one unit
// through fri_tail_units (fri.hip), the routine the lock-step prover runs.
//
// Replaces plonky2::fri::prover::{fri_proof, fri_committed_trees, fri_proof_of_work,
// fri_prover_query_rounds} (reached through CircuitData::prove, src/plonky2_semaphore/access_set.rs:94).
// Per layer, with A = 2^arity_bits[l]: bit-reverse the evaluations into leaves of A extension elements (hash_or_noop: the two
// elements of arity 2 are their own digest, longer leaves are hashed), Merkle tree with cap, observe cap, squeeze beta, fold the
// coefficients by A, coset-NTT on shift^A (src/plonky2_verifier/chip/fri_chip.rs:168-226,275-316 states the arity-2 case; transcript
// order chip/plonk/plonk_verifier_chip.rs:120-140).  Only the cap (<= 16 digests) crosses PCIe per layer.
#include "gl355_internal.h"
#include "blinding.cuh"

#include <errno.h>
#include <new>
#include <sys/random.h>

using namespace gl355;

extern "C" int32_t gl355_fri_prove(gl355_ctx* h, const uint64_t* final_coeffs, uint32_t log_n, uint32_t rate_bits,
                                   uint32_t cap_height, const uint32_t* arity_bits, uint32_t n_layers, uint32_t pow_bits,
                                   uint32_t num_queries, gl355_challenger* ch, uint64_t* caps_out, uint64_t* final_poly_out,
                                   uint64_t* pow_witness, uint64_t* query_indices, uint64_t* step_evals,
                                   uint64_t* step_siblings) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!final_coeffs || !ch || !caps_out || !final_poly_out || !pow_witness || !query_indices || !step_evals || !step_siblings)
        return ctx->fail(GL355_E_INVALID_ARG, "fri_prove: null argument");
    const uint32_t lde_bits = log_n + rate_bits;
    if (log_n == 0 || lde_bits > 27 || n_layers > 32) return ctx->fail(GL355_E_UNSUPPORTED, "fri_prove: unsupported size");
    if (n_layers && !arity_bits) return ctx->fail(GL355_E_INVALID_ARG, "fri_prove: null argument");
    for (uint32_t l = 0; l < n_layers; l++) {
        if (arity_bits[l] == 0) return ctx->fail(GL355_E_INVALID_ARG, "fri_prove: an arity of 0 bits");
        if (arity_bits[l] > GL355_MAX_FRI_ARITY_BITS) return ctx->fail(GL355_E_UNSUPPORTED, "fri_prove: a layer folds by 2, 4, 8 or 16");
    }
    // the interleaved coefficients as the two base columns the shared FRI tail folds, then that tail for one unit
    FriShape shape{log_n, rate_bits, cap_height, pow_bits, num_queries, ch->hasher, FriLayers()};
    const FriLayers& fl = shape.layers;
    if (shape.layers.init(lde_bits, cap_height, n_layers, arity_bits) != GL355_OK)
        return ctx->fail(GL355_E_INVALID_ARG, "fri_prove: too many layers for the cap height");
    if (fl.total_bits > log_n) return ctx->fail(GL355_E_INVALID_ARG, "fri_prove: the layers fold more than the polynomial has coefficients");
    const uint64_t n = 1ull << log_n, N = 1ull << lde_bits;
    const uint64_t sib_total = fl.sib_total;
    Staged sc(ctx);
    GL355_TRY(sc.open(final_coeffs, n * 16, 1));
    Scratch work(ctx), outb(ctx);
    GL355_TRY(work.get((2 * n + n + 8 + 2 * N) * 8));
    GL355_TRY(outb.get(((uint64_t)num_queries * (1 + fl.ev_total + sib_total) + 16) * 8));
    uint64_t* cols = work.as<uint64_t>();
    uint64_t* cols2 = cols + 2 * n;
    uint64_t* vals = cols2 + n + 8;
    uint64_t* d_idx = outb.as<uint64_t>();
    uint64_t* d_ev = d_idx + num_queries;
    uint64_t* d_sib = d_ev + (uint64_t)num_queries * fl.ev_total;
    uint64_t* stage = nullptr;
    GL355_TRY(ctx->pinned(fri_tail_stage_words(shape, 1) * 8, reinterpret_cast<void**>(&stage)));
    GL355_TRY(ext_split_dev(ctx, sc.as<uint64_t>(), n, cols, cols + n));
    const FriUnitOut out{caps_out, final_poly_out, pow_witness};
    GL355_TRY(fri_tail_units(ctx, shape, 1, cols, cols2, vals, stage, ch, &out, query_indices, d_idx, d_ev, d_sib));
    if (n_layers) GL355_HIP(ctx, ctx->d2h(step_evals, d_ev, (uint64_t)num_queries * fl.ev_total * 8));
    if (sib_total) GL355_HIP(ctx, ctx->d2h(step_siblings, d_sib, (uint64_t)num_queries * sib_total * 8));
    GL355_HIP(ctx, ctx->wait());
    return GL355_OK;
}

// ================================================================================================
// gl355_prove: CircuitData::prove in one call (src/plonky2_semaphore/access_set.rs:94, recursion.rs:168,
// wrapper.rs:55).  Stage order and transcript: chip/plonk/plonk_verifier_chip.rs:55-154; oracle and
// opening order: types/common_data.rs:100-222, types/assigned.rs:26-44.  Everything between the
// witness upload and the final proof download stays resident in HBM; the host only runs the
// Challenger (about 50 permutations).  The proof is returned as one flat u64 buffer (layout in
// include/gl355.h), which doubles as the wire format between aggregation levels.
// ================================================================================================
namespace gl355 {

// salt columns of a blinded oracle: thread b writes the four elements of ChaCha20 block b of `stream` (blinding.cuh)
__global__ void salt_kernel(uint64_t* out, uint64_t n, BlindKey key, uint32_t stream) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (4 * b >= n) return;
    uint64_t e[4];
    blind_block_elements(key, stream, (uint32_t)b, e);
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (4 * b + j < n) out[4 * b + j] = e[j];
}

// key == NULL: a fresh 256-bit key from the OS CSPRNG for this proof (what plonky2's OsRng does); else the caller's key
int32_t resolve_blinding_key(Ctx* ctx, const uint8_t* key, BlindKey* out) {
    uint8_t buf[32];
    if (!key) {
        size_t got = 0;
        while (got < sizeof buf) {
            const ssize_t r = getrandom(buf + got, sizeof buf - got, 0);
            if (r < 0) { if (errno == EINTR) continue; return ctx->fail(GL355_E_UNSUPPORTED, "getrandom failed: no blinding key"); }
            got += (size_t)r;
        }
        key = buf;
    }
    *out = blind_key_from_bytes(key);
    return GL355_OK;
}

int32_t resolve_blinding_key_words(Ctx* ctx, const uint8_t* key, uint32_t out[8]) {
    BlindKey k;
    GL355_TRY(resolve_blinding_key(ctx, key, &k));
    memcpy(out, k.w, 32);
    return GL355_OK;
}

}  // namespace gl355

extern "C" uint64_t gl355_proof_words(const gl355_prover_data* pd) {
    if (!pd || !pd->circuit) return 0;
    return ProofLayout(*pd).words;
}

// ---- single-proof entries: one unit through the lock-step prover (prover_batch.hip) ---------------------------------------
extern "C" int32_t gl355_prove(gl355_ctx* h, const gl355_prover_data* pd, const uint64_t* wires, const uint64_t* public_inputs,
                               uint32_t n_public_inputs, const uint8_t* blinding_key, uint64_t* proof, uint64_t proof_capacity_words) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!pd || !pd->circuit || !wires) return ctx->fail(GL355_E_INVALID_ARG, "prove: null argument");
    Staged s_wires(ctx);
    GL355_TRY(s_wires.open(wires, ((uint64_t)pd->circuit->num_wires << pd->circuit->degree_bits) * 8, 1));
    ProveUnit io{public_inputs, n_public_inputs, {0}, proof, proof_capacity_words};
    GL355_TRY(resolve_blinding_key_words(ctx, blinding_key, io.key));
    try {
        return prove_units(ctx, pd, 1, s_wires.as<uint64_t>(), nullptr, nullptr, 0, 0, 0, 0, 0, &io);
    } catch (const std::bad_alloc&) {
        return ctx->fail(GL355_E_OOM, "prove: out of host memory");
    } catch (...) {
        return ctx->fail(GL355_E_HIP, "prove: unexpected host failure");
    }
}

// Witness given as its non-zero rows only (the rest of the 2^degree_bits rows are Noop rows): rows[r] lists
// all num_wires values of circuit row row_idx[r].  The zero-knowledge blinding rows are filled on the device:
// rows [blind_start, blind_start+n_blind) get random values on every wire, and n_z_pairs consecutive row
// pairs starting at z_start carry, on every routed wire, one random value shared by the two rows of the pair (the builder
// copy-constrains each column between them: plonky2 `blind`).
extern "C" int32_t gl355_prove_sparse(gl355_ctx* h, const gl355_prover_data* pd, const uint32_t* row_idx, const uint64_t* rows,
                                      uint32_t n_rows, uint32_t blind_start, uint32_t n_blind, uint32_t z_start, uint32_t n_z_pairs,
                                      const uint64_t* public_inputs, uint32_t n_public_inputs, const uint8_t* blinding_key, uint64_t* proof,
                                      uint64_t proof_capacity_words) {
    return gl355_prove_sparse_units(h, pd, 1, row_idx, rows, n_rows, blind_start, n_blind, z_start, n_z_pairs, public_inputs, n_public_inputs,
                                    blinding_key, proof, proof_capacity_words);
}

// the same for n_units independent witnesses of ONE circuit, proven in lock-step on this context (every stage's kernels carry
// a unit dimension; per-unit transcripts, keys and proofs): rows = [n_units][n_rows][num_wires], public_inputs = [n_units][n_public_inputs],
// proofs = [n_units][proof_capacity_words], blinding_keys = [n_units][32] or NULL (a fresh OS-random key for every unit)
extern "C" int32_t gl355_prove_sparse_units(gl355_ctx* h, const gl355_prover_data* pd, uint32_t n_units, const uint32_t* row_idx, const uint64_t* rows,
                                            uint32_t n_rows, uint32_t blind_start, uint32_t n_blind, uint32_t z_start, uint32_t n_z_pairs,
                                            const uint64_t* public_inputs, uint32_t n_public_inputs, const uint8_t* blinding_keys,
                                            uint64_t* proofs, uint64_t proof_capacity_words) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!pd || !pd->circuit || (!row_idx && n_rows) || (!rows && n_rows) || !proofs || (!public_inputs && n_public_inputs))
        return ctx->fail(GL355_E_INVALID_ARG, "prove_sparse: null argument");
    if (n_units == 0 || n_units > GL355_MAX_UNITS) return ctx->fail(GL355_E_INVALID_ARG, "prove_sparse: 1..GL355_MAX_UNITS units per call");
    const uint64_t n = 1ull << pd->circuit->degree_bits;
    if ((uint64_t)blind_start + n_blind > n || (uint64_t)z_start + 2ull * n_z_pairs > n) return ctx->fail(GL355_E_INVALID_ARG, "prove_sparse: blinding rows out of range");
    for (uint32_t r = 0; r < n_rows; r++)
        if (row_idx[r] >= n) return ctx->fail(GL355_E_INVALID_ARG, "prove_sparse: row index out of range");
    ProveUnit io[GL355_MAX_UNITS];
    for (uint32_t u = 0; u < n_units; u++) {
        io[u] = ProveUnit{public_inputs ? public_inputs + (uint64_t)u * n_public_inputs : nullptr, n_public_inputs, {0},
                          proofs + (uint64_t)u * proof_capacity_words, proof_capacity_words};
        GL355_TRY(resolve_blinding_key_words(ctx, blinding_keys ? blinding_keys + 32ull * u : nullptr, io[u].key));
    }
    try {
        return prove_units(ctx, pd, n_units, nullptr, row_idx, rows, n_rows, blind_start, n_blind, z_start, n_z_pairs, io);
    } catch (const std::bad_alloc&) {
        return ctx->fail(GL355_E_OOM, "prove: out of host memory");
    } catch (...) {
        return ctx->fail(GL355_E_HIP, "prove: unexpected host failure");      // nothing is thrown across the C boundary
    }
}

// ---- blinding-stream surface (blinding.cuh) ----------------------------------------------------------------------------
// per-unit key of a batch: first 32 bytes of ChaCha20 block 0 under the batch key with nonce ("key", index_lo, index_hi)
extern "C" int32_t gl355_derive_key(const uint8_t base_key[32], uint64_t index, uint8_t out[32]) {
    if (!base_key || !out) return GL355_E_INVALID_ARG;
    uint32_t o[16];
    chacha20_block(blind_key_from_bytes(base_key), 0, GL355_BLIND_NONCE_KEY, (uint32_t)index, (uint32_t)(index >> 32), o);
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(o[i] >> (8 * b));
    return GL355_OK;
}
// the first `count` field elements of blinding stream `stream` under `key`, produced by the device kernel the prover uses
extern "C" int32_t gl355_blinding_elements(gl355_ctx* h, const uint8_t key[32], uint32_t stream, uint64_t count, uint64_t* out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!key || (!out && count)) return ctx->fail(GL355_E_INVALID_ARG, "blinding_elements: null argument");
    if (count == 0) return GL355_OK;
    if (count > (1ull << 34)) return ctx->fail(GL355_E_UNSUPPORTED, "blinding_elements: a stream holds 2^34 elements");
    Staged so(ctx);
    GL355_TRY(so.open(out, count * 8, 2));
    hipLaunchKernelGGL(salt_kernel, dim3((uint32_t)((count / 4 + 256) / 256)), dim3(256), 0, ctx->stream, so.as<uint64_t>(), count,
                       blind_key_from_bytes(key), stream);
    GL355_HIP(ctx, hipGetLastError());
    return so.finish();
}
