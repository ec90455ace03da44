// Circuit artifacts: a built circuit (shape, selector / constant / sigma tables, FRI parameters, blinding rows, the sparse
// witness-row map and, for the recursive verifier, the witness tape) serialised once by the host-side builder and loaded
// here, so that the per-proof path is native end to end:
//   gl355_semaphore_prove      = fill_semaphore_targets + data.prove      (src/plonky2_semaphore/access_set.rs:61-104)
//   gl355_circuit_prove_tape   = set_proof_with_pis_target + data.prove   (recursion.rs:72-86,167-168; wrapper.rs:49-55)
// Building a circuit (plonky2's CircuitBuilder::build, access_set.rs:91, recursion.rs:167, wrapper.rs:41) happens once per
// circuit shape and stays on the host-side builder; proving happens per signal and needs nothing but this file's calls.
// A loaded circuit is read-only and may be used concurrently by every context of its device.
#include "gl355_internal.h"
#include "circuit_artifact.h"

#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

using namespace gl355;

// owns its device memory and its oracle; deleted with its device selected (gl355_circuit_destroy, or a load that fails)
struct gl355_circuit_handle {
    Ctx* owner = nullptr;
    gl355_circuit c;
    gl355_prover_data pd;
    gl355_verifier_data vd;            // gl355_circuit_verify: the cap and the k_is below, everything else as in pd
    gl355_oracle* cs = nullptr;
    uint64_t* d_sigmas = nullptr;
    uint64_t* d_kis = nullptr;
    uint64_t* d_tape = nullptr;        // device copy of the tape | segment starts | public-input positions (witness_tape_dev.hip)
    uint64_t* d_seg_start = nullptr;
    uint64_t* d_pi_pos = nullptr;
    std::vector<uint32_t> row_idx;
    std::vector<uint64_t> pi_pos, tape, seg_lens;
    std::vector<uint64_t> cs_cap, k_is_host;     // verifier data
    std::vector<uint32_t> fri_arity_bits;        // [n_fri_layers]: the artifact's table (versions 4 / 5), all ones for versions 2 / 3; pd.fri_arity_bits points here
    uint64_t n_seq = 0;
    uint32_t blind_start = 0, n_blind = 0, z_start = 0, n_z_pairs = 0, n_pi = 0;
    uint64_t n_inputs = 0;
    ~gl355_circuit_handle() {
        if (cs) gl355_oracle_destroy(cs);
        if (d_sigmas) (void)hipFree(d_sigmas);
        if (d_kis) (void)hipFree(d_kis);
        if (d_tape) (void)hipFree(d_tape);
    }
};

namespace {
// witness generation of n_units units: tape replays spread over the context's replay threads (one unit per thread at a time;
// a single unit still uses its segments in parallel)
int32_t replay_units(uint32_t threads, const gl355_circuit_handle* ch, uint32_t n_units, const uint64_t* inputs, uint64_t* rows, uint64_t n_words,
                     uint64_t* failed_unit, uint64_t* failed_op) {
    const uint32_t nt = std::max<uint32_t>(1, std::min<uint32_t>(threads, n_units));
    auto replay = [&](uint32_t u, uint32_t segment_threads, uint64_t* failed) {
        return gl355_witness_replay_segmented(ch->tape.data(), ch->tape.size() / 5, ch->n_seq, ch->seg_lens.data(), (uint32_t)ch->seg_lens.size(), segment_threads,
                                              inputs + (uint64_t)u * ch->n_inputs, ch->n_inputs, rows + (uint64_t)u * n_words, n_words, ch->c.num_wires, failed);
    };
    if (n_units == 1 || nt == 1) {
        for (uint32_t u = 0; u < n_units; u++) {
            uint64_t f = 0;
            const int32_t rc = replay(u, n_units == 1 ? threads : 1, &f);
            if (rc != GL355_OK) { *failed_unit = u; *failed_op = f; return rc; }
        }
        return GL355_OK;
    }
    std::atomic<uint32_t> next{0};
    std::vector<int32_t> rcs(n_units, GL355_OK);
    std::vector<uint64_t> fails(n_units, 0);
    auto worker = [&]() {
        for (uint32_t u; (u = next.fetch_add(1)) < n_units;) rcs[u] = replay(u, 1, &fails[u]);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    for (uint32_t u = 0; u < n_units; u++)
        if (rcs[u] != GL355_OK) { *failed_unit = u; *failed_op = fails[u]; return rcs[u]; }
    return GL355_OK;
}
}  // namespace

// for the batch runtime (batch.cpp), which overlaps the witness generation of one batch with the proving of the previous one
namespace gl355 {
uint64_t circuit_rows_words(const gl355_circuit_handle* ch) { return (uint64_t)ch->row_idx.size() * ch->c.num_wires; }
// device scratch of one device replay: inputs | status | public inputs
uint64_t circuit_replay_aux_bytes(const gl355_circuit_handle* ch, uint32_t n_units) { return (uint64_t)n_units * (ch->n_inputs + 1 + ch->n_pi) * 8 + 64; }
int32_t circuit_replay_units_dev(const gl355_circuit_handle* ch, int device, hipStream_t stream, uint32_t n_units, const uint64_t* inputs, uint64_t* d_rows,
                                 void* d_aux, uint64_t* pis_out, uint64_t* failed_unit, uint64_t* failed_op, void* h_aux) {
    if (!ch->d_tape) return GL355_E_INVALID_ARG;
    if (hipSetDevice(device) != hipSuccess) return GL355_E_HIP;
    uint64_t* d_inputs = reinterpret_cast<uint64_t*>(d_aux);
    uint64_t* d_status = d_inputs + (uint64_t)n_units * ch->n_inputs;
    uint64_t* d_pis = d_status + n_units;
    // h_aux: a pinned host mirror of d_aux (circuit_replay_aux_bytes) -- the batch runtime's side stream; nullptr: the caller's pageable memory
    const uint64_t* src = inputs;
    std::vector<uint64_t> back_pageable;
    uint64_t* back;
    if (h_aux) {
        uint64_t* h_inputs = reinterpret_cast<uint64_t*>(h_aux);
        memcpy(h_inputs, inputs, (size_t)n_units * ch->n_inputs * 8);
        src = h_inputs;
        back = h_inputs + (uint64_t)n_units * ch->n_inputs;
    } else {
        back_pageable.resize((size_t)n_units * (1 + ch->n_pi));
        back = back_pageable.data();
    }
    if (hipMemcpyAsync(d_inputs, src, (size_t)n_units * ch->n_inputs * 8, hipMemcpyHostToDevice, stream) != hipSuccess) return GL355_E_HIP;
    GL355_TRY(tape_replay_dev(stream, ch->d_tape, ch->d_seg_start, ch->n_seq, (uint32_t)ch->seg_lens.size(), n_units, d_inputs, ch->n_inputs, d_rows,
                              circuit_rows_words(ch), ch->d_pi_pos, ch->n_pi, d_status, d_pis));
    if (hipMemcpyAsync(back, d_status, (size_t)n_units * (1 + ch->n_pi) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return GL355_E_HIP;
    for (;;) {                        // wait for the side stream without holding a core
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return GL355_E_HIP;
        (void)hipGetLastError();
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    for (uint32_t u = 0; u < n_units; u++)
        if (back[u] != ~0ull) { *failed_unit = u; *failed_op = back[u]; return GL355_E_WITNESS; }
    memcpy(pis_out, back + n_units, (size_t)n_units * ch->n_pi * 8);
    return GL355_OK;
}
int32_t circuit_replay_units(const gl355_circuit_handle* ch, uint32_t threads, uint32_t n_units, const uint64_t* inputs, uint64_t* rows, uint64_t* pis_out,
                             uint64_t* failed_unit, uint64_t* failed_op) {
    const uint64_t n_words = circuit_rows_words(ch);
    GL355_TRY(replay_units(threads, ch, n_units, inputs, rows, n_words, failed_unit, failed_op));
    for (uint32_t u = 0; u < n_units; u++)
        for (uint32_t i = 0; i < ch->n_pi; i++) pis_out[(size_t)u * ch->n_pi + i] = rows[(uint64_t)u * n_words + ch->pi_pos[i]];
    return GL355_OK;
}
}  // namespace gl355

extern "C" {

// argument checks, the host's whole check of the artifact (circuit_artifact.h), then the device work: uploads, the commitment of
// constants_sigmas and the digest or cap comparison.  Everything below the parse reads the view.
int32_t gl355_circuit_load(gl355_ctx* h, const uint64_t* blob, uint64_t words, gl355_circuit_handle** out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    char msg[ART_MSG_LEN];
    if (!out) return ctx->fail(art_refuse(ART_R_TRUNCATED, msg), msg);
    *out = nullptr;
    ArtifactView v;
    if (const int32_t rc = artifact_parse(blob, words, v, msg)) return ctx->fail(rc, msg);
    const gl355_circuit& c = v.c;
    const uint64_t n = 1ull << c.degree_bits, routed = c.num_routed_wires, n_cap = 1ull << v.cap_height;

    std::unique_ptr<gl355_circuit_handle> ch(new (std::nothrow) gl355_circuit_handle());
    if (!ch) return GL355_E_OOM;
    ch->owner = ctx;
    ch->c = c;
    ch->blind_start = v.blind_start; ch->n_blind = v.n_blind; ch->z_start = v.z_start; ch->n_z_pairs = v.n_z_pairs;
    ch->n_inputs = v.n_inputs; ch->n_pi = (uint32_t)v.n_pi; ch->n_seq = v.n_seq;
    ch->fri_arity_bits.assign(v.fri_arity_bits, v.fri_arity_bits + v.n_fri_layers);
    ch->row_idx.assign(v.row_idx.p, v.row_idx.p + v.n_rows);      // each below n <= 2^24 (artifact_parse)
    ch->pi_pos.assign(v.pi_pos.p, v.pi_pos.p + v.n_pi);
    ch->tape.assign(v.tape.p, v.tape.p + v.tape.words);
    ch->seg_lens.assign(v.seg_lens.p, v.seg_lens.p + v.n_segs);
    ch->k_is_host.assign(v.k_is.p, v.k_is.p + routed);
    // device copies of the tape, the sigma values and the k_is (plain allocations: shared by every context of the device)
    if (v.n_ops) {
        std::vector<uint64_t> seg_start(v.n_segs + 1, v.n_seq);
        for (uint64_t k = 0; k < v.n_segs; k++) seg_start[k + 1] = seg_start[k] + ch->seg_lens[k];
        const uint64_t tape_words = v.tape.words + (v.n_segs + 1) + v.n_pi;
        if (hipMalloc((void**)&ch->d_tape, tape_words * 8 + 8) != hipSuccess) return ctx->fail(GL355_E_OOM, "circuit_load: hipMalloc");
        ch->d_seg_start = ch->d_tape + v.tape.words;
        ch->d_pi_pos = ch->d_seg_start + (v.n_segs + 1);
        if (hipMemcpy(ch->d_tape, v.tape.p, v.tape.words * 8, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(ch->d_seg_start, seg_start.data(), (v.n_segs + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
            (v.n_pi && hipMemcpy(ch->d_pi_pos, v.pi_pos.p, v.n_pi * 8, hipMemcpyHostToDevice) != hipSuccess))
            return ctx->fail(GL355_E_HIP, "circuit_load: upload");
    }
    if (hipMalloc(&ch->d_sigmas, routed * n * 8) != hipSuccess || hipMalloc(&ch->d_kis, routed * 8 + 8) != hipSuccess) return ctx->fail(GL355_E_OOM, "circuit_load: hipMalloc");
    if (hipMemcpyAsync(ch->d_sigmas, v.sigmas.p, routed * n * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(ch->d_kis, v.k_is.p, routed * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return ctx->fail(GL355_E_HIP, "circuit_load: upload");
    // constants and sigmas are adjacent in the artifact: one batch
    GL355_TRY(gl355_commit_h(h, v.hasher, v.constants.p, c.degree_bits, c.num_selectors + c.num_constants + c.num_routed_wires, c.rate_bits, 0, nullptr,
                             v.cap_height, &ch->cs));
    // the digest covers the preprocessed commitment and the shape: recompute it, a stale or foreign artifact is refused
    std::vector<uint64_t> pre(n_cap * 4 + 3 + c.num_gates);
    GL355_TRY(gl355_oracle_cap(ch->cs, pre.data()));
    ch->cs_cap.assign(pre.begin(), pre.begin() + n_cap * 4);
    uint64_t* s = pre.data() + n_cap * 4;
    s[0] = c.degree_bits; s[1] = c.num_gates; s[2] = c.num_selectors;
    for (uint32_t g = 0; g < c.num_gates; g++) s[3 + g] = ((uint64_t)c.gates[g].type << 32) | c.gates[g].param;   // no aliasing between (type, param) pairs
    if (v.external_digest) {
        // versions 3 / 5: the transcript uses the digest as given (e.g. plonky2's own); what ties the tables to it is the commitment
        if (memcmp(pre.data(), v.cap.p, n_cap * 32) != 0) return ctx->fail(GL355_E_INVALID_ARG, "circuit_load: the artifact's constants_sigmas cap does not match its tables");
    } else {
        uint64_t dg[4];
        gl355_host_hash_no_pad_h(v.hasher, pre.data(), pre.size(), dg);
        if (memcmp(dg, v.digest, 32) != 0) return ctx->fail(GL355_E_INVALID_ARG, "circuit_load: circuit digest of the artifact does not match its tables");
    }
    gl355_prover_data& pd = ch->pd;
    memset(&pd, 0, sizeof pd);
    pd.circuit = &ch->c;
    pd.constants_sigmas = ch->cs;
    pd.sigmas = ch->d_sigmas;
    pd.k_is = ch->d_kis;
    memcpy(pd.circuit_digest, v.digest, 32);
    pd.cap_height = v.cap_height; pd.pow_bits = v.pow_bits; pd.num_queries = v.num_queries;
    pd.n_fri_layers = v.n_fri_layers; pd.zero_knowledge = v.zero_knowledge; pd.hasher = v.hasher;
    pd.fri_arity_bits = v.arity_table ? ch->fri_arity_bits.data() : nullptr;      // versions 2 / 3 carry a layer count only: the reference's flow, every layer folds by 2
    gl355_verifier_data& vd = ch->vd;
    memset(&vd, 0, sizeof vd);
    vd.circuit = &ch->c; vd.constants_sigmas_cap = ch->cs_cap.data(); vd.k_is = ch->k_is_host.data();
    memcpy(vd.circuit_digest, pd.circuit_digest, 32);
    vd.cap_height = pd.cap_height; vd.pow_bits = pd.pow_bits; vd.num_queries = pd.num_queries; vd.n_fri_layers = pd.n_fri_layers;
    vd.zero_knowledge = pd.zero_knowledge; vd.hasher = pd.hasher;
    vd.fri_arity_bits = pd.fri_arity_bits;
    *out = ch.release();
    return GL355_OK;
}

int32_t gl355_circuit_destroy(gl355_circuit_handle* ch) {
    if (!ch) return GL355_OK;
    (void)hipSetDevice(ch->owner->device);
    delete ch;
    return GL355_OK;
}

int32_t gl355_circuit_info(const gl355_circuit_handle* ch, uint64_t* proof_words, uint32_t* n_public_inputs, uint32_t* n_rows,
                           uint64_t* n_inputs, uint32_t* degree_bits) {
    if (!ch) return GL355_E_INVALID_ARG;
    if (proof_words) *proof_words = gl355_proof_words(&ch->pd);
    if (n_public_inputs) *n_public_inputs = ch->n_pi;
    if (n_rows) *n_rows = (uint32_t)ch->row_idx.size();
    if (n_inputs) *n_inputs = ch->n_inputs;
    if (degree_bits) *degree_bits = ch->c.degree_bits;
    return GL355_OK;
}
const uint64_t* gl355_circuit_digest(const gl355_circuit_handle* ch) { return ch ? ch->pd.circuit_digest : nullptr; }
int32_t gl355_circuit_fri_arity_bits(const gl355_circuit_handle* ch, uint32_t* out, uint32_t* n_layers) {
    if (!ch) return GL355_E_INVALID_ARG;
    if (n_layers) *n_layers = ch->pd.n_fri_layers;
    if (out) memcpy(out, ch->fri_arity_bits.data(), ch->fri_arity_bits.size() * sizeof(uint32_t));
    return GL355_OK;
}

int32_t gl355_circuit_verify(const gl355_circuit_handle* ch, const uint64_t* proof, uint64_t proof_words, const uint64_t* public_inputs,
                             uint32_t n_public_inputs) {
    if (!ch) return GL355_E_INVALID_ARG;
    return gl355_verify(&ch->vd, proof, proof_words, public_inputs, n_public_inputs);
}

int32_t gl355_circuit_prove_rows(gl355_ctx* h, const gl355_circuit_handle* ch, const uint64_t* rows, const uint64_t* public_inputs,
                                 uint32_t n_public_inputs, const uint8_t* blinding_key, uint64_t* proof, uint64_t proof_capacity_words) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !rows) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_rows: null argument");
    if (ctx->device != ch->owner->device) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_rows: circuit was loaded on another device");
    return gl355_prove_sparse(h, &ch->pd, ch->row_idx.data(), rows, (uint32_t)ch->row_idx.size(), ch->blind_start, ch->n_blind, ch->z_start,
                              ch->n_z_pairs, public_inputs, n_public_inputs, blinding_key, proof, proof_capacity_words);
}
int32_t gl355_circuit_prove_rows_units(gl355_ctx* h, const gl355_circuit_handle* ch, uint32_t n_units, const uint64_t* rows, const uint64_t* public_inputs,
                                       uint32_t n_public_inputs, const uint8_t* blinding_keys, uint64_t* proofs) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !rows || !proofs) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_rows_units: null argument");
    if (ctx->device != ch->owner->device) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_rows_units: circuit was loaded on another device");
    return gl355_prove_sparse_units(h, &ch->pd, n_units, ch->row_idx.data(), rows, (uint32_t)ch->row_idx.size(), ch->blind_start, ch->n_blind, ch->z_start,
                                    ch->n_z_pairs, public_inputs, n_public_inputs, blinding_keys, proofs, gl355_proof_words(&ch->pd));
}

int32_t gl355_circuit_witness_rows(gl355_ctx* h, const gl355_circuit_handle* ch, uint32_t n_units, const uint64_t* inputs, uint64_t n_inputs,
                                   int32_t on_device, uint64_t* rows, uint64_t* public_inputs_out, uint64_t* failed_entry) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !inputs || !rows) return ctx->fail(GL355_E_INVALID_ARG, "circuit_witness_rows: null argument");
    if (ch->tape.empty()) return ctx->fail(GL355_E_INVALID_ARG, "circuit_witness_rows: this artifact carries no witness tape");
    if (n_inputs != ch->n_inputs || n_units == 0 || n_units > GL355_MAX_UNITS) return ctx->fail(GL355_E_INVALID_ARG, "circuit_witness_rows: bad input shape");
    const uint64_t n_words = circuit_rows_words(ch);
    std::vector<uint64_t> pis((size_t)n_units * ch->n_pi + 1);
    uint64_t fu = 0, fo = ~0ull;
    int32_t rc;
    if (!on_device) {
        rc = circuit_replay_units(ch, ctx->replay_threads, n_units, inputs, rows, pis.data(), &fu, &fo);
    } else {
        if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
        Scratch d_rows(ctx), aux(ctx);
        GL355_TRY(d_rows.get(n_units * n_words * 8));
        GL355_TRY(aux.get(circuit_replay_aux_bytes(ch, n_units)));
        rc = circuit_replay_units_dev(ch, ctx->device, ctx->stream, n_units, inputs, d_rows.as<uint64_t>(), aux.p, pis.data(), &fu, &fo);
        if (rc == GL355_OK || rc == GL355_E_WITNESS) {
            GL355_HIP(ctx, ctx->d2h(rows, d_rows.p, n_units * n_words * 8));
            GL355_HIP(ctx, ctx->wait());
        }
    }
    if (failed_entry) *failed_entry = fo;
    if (rc != GL355_OK) return ctx->fail(rc, "circuit_witness_rows: the inputs do not satisfy the circuit");
    if (public_inputs_out) memcpy(public_inputs_out, pis.data(), (size_t)n_units * ch->n_pi * 8);
    return GL355_OK;
}

int32_t gl355_circuit_prove_tape_units(gl355_ctx* h, const gl355_circuit_handle* ch, uint32_t n_units, const uint64_t* inputs, uint64_t n_inputs,
                                       const uint8_t* blinding_keys, uint64_t* proofs, uint64_t* public_inputs_out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !inputs || !proofs) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_tape: null argument");
    if (ch->tape.empty()) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_tape: this artifact carries no witness tape");
    if (n_inputs != ch->n_inputs) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_tape: wrong number of input words");
    if (n_units == 0 || n_units > GL355_MAX_UNITS) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_tape: 1..GL355_MAX_UNITS units per call");
    const uint64_t n_words = (uint64_t)ch->row_idx.size() * ch->c.num_wires;
    std::vector<uint64_t> pis((size_t)ch->n_pi * n_units);
    uint64_t failed_unit = 0, failed_op = 0;
    auto witness_error = [&](int32_t rc) {
        char msg[128];
        snprintf(msg, sizeof msg, "circuit_prove_tape: witness generation of unit %llu failed at tape entry %llu", (unsigned long long)failed_unit,
                 (unsigned long long)failed_op);
        return ctx->fail(rc, msg);
    };
    if (ctx->device_replay && ch->d_tape && n_units > 1) {
        // witness rows generated where the prover reads them (witness_tape_dev.hip): the host uploads the inputs only.  A single unit
        // keeps the host replay: its latency (2-7 ms) beats the interpreter's (~20 ms, one lane for the sequential part)
        if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
        Scratch d_rows(ctx), aux(ctx);
        GL355_TRY(d_rows.get(n_units * n_words * 8));
        GL355_TRY(aux.get(circuit_replay_aux_bytes(ch, n_units)));
        const int32_t rc = circuit_replay_units_dev(ch, ctx->device, ctx->stream, n_units, inputs, d_rows.as<uint64_t>(), aux.p, pis.data(), &failed_unit, &failed_op);
        if (rc != GL355_OK) return rc == GL355_E_WITNESS ? witness_error(rc) : ctx->fail(rc, "circuit_prove_tape: device witness generation failed");
        if (public_inputs_out) memcpy(public_inputs_out, pis.data(), pis.size() * 8);
        return gl355_circuit_prove_rows_units(h, ch, n_units, d_rows.as<uint64_t>(), pis.data(), ch->n_pi, blinding_keys, proofs);
    }
    static thread_local std::vector<uint64_t> rows;      // one prover thread per context: reuse the row buffer
    rows.resize(n_words * n_units);
    const int32_t rc = circuit_replay_units(ch, ctx->replay_threads, n_units, inputs, rows.data(), pis.data(), &failed_unit, &failed_op);
    if (rc != GL355_OK) return witness_error(rc);
    if (public_inputs_out) memcpy(public_inputs_out, pis.data(), pis.size() * 8);
    return gl355_circuit_prove_rows_units(h, ch, n_units, rows.data(), pis.data(), ch->n_pi, blinding_keys, proofs);
}
int32_t gl355_circuit_prove_tape(gl355_ctx* h, const gl355_circuit_handle* ch, const uint64_t* inputs, uint64_t n_inputs, const uint8_t* blinding_key,
                                 uint64_t* proof, uint64_t proof_capacity_words, uint64_t* public_inputs_out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !proof) return ctx->fail(GL355_E_INVALID_ARG, "circuit_prove_tape: null argument");
    if (proof_capacity_words < gl355_proof_words(&ch->pd)) return ctx->fail(GL355_E_INVALID_ARG, "prove: proof buffer too small (see gl355_proof_words)");
    return gl355_circuit_prove_tape_units(h, ch, 1, inputs, n_inputs, blinding_key, proof, public_inputs_out);
}

int32_t gl355_semaphore_prove_units(gl355_ctx* h, const gl355_circuit_handle* ch, uint32_t n_units, const uint64_t* private_keys, const uint64_t* topics,
                                    const uint64_t* indices, const uint64_t* siblings, uint32_t height, const uint8_t* blinding_keys, uint64_t* proofs,
                                    uint64_t* public_inputs_out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !private_keys || !topics || !indices || !proofs || (!siblings && height)) return ctx->fail(GL355_E_INVALID_ARG, "semaphore_prove: null argument");
    if (ch->row_idx.size() != (size_t)height + 7 || ch->c.num_wires != 135)
        return ctx->fail(GL355_E_INVALID_ARG, "semaphore_prove: the artifact is not the Semaphore circuit of this tree height");
    if (n_units == 0 || n_units > GL355_MAX_UNITS) return ctx->fail(GL355_E_INVALID_ARG, "semaphore_prove: 1..GL355_MAX_UNITS units per call");
    const size_t per = (size_t)(height + 7) * 135;
    std::vector<uint64_t> rows(per * n_units), pis(12 * (size_t)n_units);
    for (uint32_t u = 0; u < n_units; u++)
        GL355_TRY(gl355_semaphore_witness(private_keys + 4 * u, topics + 4 * u, indices[u], siblings + (size_t)u * height * 4, height, rows.data() + u * per,
                                          pis.data() + 12 * u));
    if (public_inputs_out) memcpy(public_inputs_out, pis.data(), pis.size() * 8);
    return gl355_circuit_prove_rows_units(h, ch, n_units, rows.data(), pis.data(), 12, blinding_keys, proofs);
}
int32_t gl355_semaphore_prove(gl355_ctx* h, const gl355_circuit_handle* ch, const uint64_t private_key[4], const uint64_t topic[4],
                              uint64_t index, const uint64_t* siblings, uint32_t height, const uint8_t* blinding_key, uint64_t* proof,
                              uint64_t proof_capacity_words, uint64_t public_inputs_out[12]) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!ch || !proof) return ctx->fail(GL355_E_INVALID_ARG, "semaphore_prove: null argument");
    if (proof_capacity_words < gl355_proof_words(&ch->pd)) return ctx->fail(GL355_E_INVALID_ARG, "prove: proof buffer too small (see gl355_proof_words)");
    return gl355_semaphore_prove_units(h, ch, 1, private_key, topic, &index, siblings, height, blinding_key, proof, public_inputs_out);
}

}  // extern "C"
