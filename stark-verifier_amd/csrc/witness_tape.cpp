// Witness tape: a straight-line program that recomputes every wire of a circuit's non-trivial rows from
// a flat input vector.  It plays the role of plonky2's witness generators (`generate_partial_witness`,
// run inside `data.prove(pw)` at src/plonky2_semaphore/recursion.rs:167-168 and wrapper.rs:55): the
// recursive-verifier circuit's ~6000 gate rows (Poseidon, Reducing, Arithmetic, RandomAccess, BaseSum,
// ...) are a fixed function of the inner proofs' words.  The tape is recorded once by the host-side
// builder (stark-verifier_amd/gadgets.py) and replayed here per proof: sequential host work
// (about 5k Poseidon permutations with their S-box-input wires + ~0.5M field operations), single thread,
// no device involvement -- callers overlap it with the GPU prove of the previous proof.
//
// What one entry touches and does is stated in witness_tape.h, which the device interpreter (witness_tape_dev.hip) shares.
#include "gl355_internal.h"
#include "witness_tape.h"

#include <atomic>
#include <thread>
#include <vector>

using namespace gl355;

// entries [begin, end) of the tape on the (already initialised) rows: every entry is checked, then executed, so the caller gets the
// first entry in tape order that does not fit (GL355_E_INVALID_ARG) or that the data refuse (GL355_E_WITNESS)
static int32_t run_entries(const uint64_t* tape, uint64_t begin, uint64_t end, const uint64_t* inputs, uint64_t n_inputs, uint64_t* rows,
                           uint64_t n_words, uint32_t num_wires, uint64_t* failed_op) {
    for (uint64_t t = begin; t < end; t++) {
        const uint64_t* e = tape + 5 * t;
        int32_t rc = GL355_OK;
        if (!tape_entry_fits(e, n_inputs, n_words, num_wires)) rc = GL355_E_INVALID_ARG;
        else if (e[0] == GL355_TAPE_POSEIDON) {
            uint64_t* row = rows + e[1];
            uint64_t in[12];
            memcpy(in, row, sizeof in);
            if (!tape_poseidon_swap_ok(row)) rc = GL355_E_WITNESS;
            else gl355_poseidon_gate_witness(in, row[TAPE_POSEIDON_SWAP], row);
        } else if (tape_entry_exec(e, inputs, rows)) rc = GL355_E_WITNESS;
        if (rc != GL355_OK) {
            if (failed_op) *failed_op = t;
            return rc;
        }
    }
    return GL355_OK;
}

// The static check of a whole tape, done once when an artifact is loaded, so that the device interpreter can run without bounds
// checks.  Returns the first entry that does not fit, or ~0.
namespace gl355 {
uint64_t tape_validate(const uint64_t* tape, uint64_t n_ops, uint64_t n_inputs, uint64_t n_words, uint32_t num_wires) {
    if (num_wires < 135) return 0;
    for (uint64_t t = 0; t < n_ops; t++)
        if (!tape_entry_fits(tape + 5 * t, n_inputs, n_words, num_wires)) return t;
    return ~0ull;
}
}  // namespace gl355

extern "C" int32_t gl355_coset_interpolation_witness(uint32_t bits, uint32_t degree, uint64_t* wires) {
    CosetInterpShape s;
    if (!wires || bits > 0xFF || degree > 0xFF || !coset_interp_shape(bits | degree << 8, s)) return GL355_E_INVALID_ARG;
    for (uint32_t i = 0; i < s.start_int; i++) wires[i] = gl_canon(wires[i]);
    return coset_interp_fill(s, wires) ? GL355_E_WITNESS : GL355_OK;
}

extern "C" int32_t gl355_witness_replay(const uint64_t* tape, uint64_t n_ops, const uint64_t* inputs, uint64_t n_inputs,
                                        uint64_t* rows, uint64_t n_words, uint32_t num_wires, uint64_t* failed_op) {
    if (!tape || !rows || (!inputs && n_inputs) || num_wires < 135) return GL355_E_INVALID_ARG;
    if (failed_op) *failed_op = ~0ull;
    memset(rows, 0, n_words * 8);
    return run_entries(tape, 0, n_ops, inputs, n_inputs, rows, n_words, num_wires, failed_op);
}

// The same with the independent segments of a segmented tape (gadgets.py begin_segment / end_segment, e.g. the FRI query
// rounds of a verifier circuit) spread over `threads` host threads: entries [0, n_seq) run first on the calling thread, then
// segment k = the next seg_lens[k] entries.  The builder has checked that a segment reads only the sequential part and
// itself, so the rows are the same as those of the sequential replay; the reported failing entry is the smallest one.
extern "C" int32_t gl355_witness_replay_segmented(const uint64_t* tape, uint64_t n_ops, uint64_t n_seq, const uint64_t* seg_lens, uint32_t n_segs,
                                                  uint32_t threads, const uint64_t* inputs, uint64_t n_inputs, uint64_t* rows, uint64_t n_words,
                                                  uint32_t num_wires, uint64_t* failed_op) {
    if (!tape || !rows || (!inputs && n_inputs) || num_wires < 135 || (!seg_lens && n_segs) || n_seq > n_ops) return GL355_E_INVALID_ARG;
    uint64_t total = n_seq;
    for (uint32_t k = 0; k < n_segs; k++) total += seg_lens[k];
    if (total != n_ops) return GL355_E_INVALID_ARG;
    if (failed_op) *failed_op = ~0ull;
    memset(rows, 0, n_words * 8);
    int32_t rc = run_entries(tape, 0, n_seq, inputs, n_inputs, rows, n_words, num_wires, failed_op);
    if (rc != GL355_OK || n_segs == 0) return rc;
    if (threads <= 1) return run_entries(tape, n_seq, n_ops, inputs, n_inputs, rows, n_words, num_wires, failed_op);
    std::vector<uint64_t> start(n_segs + 1, n_seq);
    for (uint32_t k = 0; k < n_segs; k++) start[k + 1] = start[k] + seg_lens[k];
    const uint32_t nt = threads < n_segs ? threads : n_segs;
    std::vector<int32_t> rcs(nt, GL355_OK);
    std::vector<uint64_t> fails(nt, ~0ull);
    std::atomic<uint32_t> next{0};
    auto worker = [&](uint32_t t) {
        for (;;) {
            const uint32_t k = next.fetch_add(1);
            if (k >= n_segs) return;
            uint64_t f = ~0ull;
            const int32_t r = run_entries(tape, start[k], start[k + 1], inputs, n_inputs, rows, n_words, num_wires, &f);
            if (r != GL355_OK && f < fails[t]) { rcs[t] = r; fails[t] = f; }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(worker, t);
    worker(0);
    for (auto& th : pool) th.join();
    uint64_t best = ~0ull;
    for (uint32_t t = 0; t < nt; t++)
        if (rcs[t] != GL355_OK && fails[t] < best) { best = fails[t]; rc = rcs[t]; }
    if (failed_op && best != ~0ull) *failed_op = best;
    return rc;
}
