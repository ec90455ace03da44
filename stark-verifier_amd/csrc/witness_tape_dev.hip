// Witness generation of a recorded circuit ON THE DEVICE: the tape of witness_tape.cpp -- plonky2's witness
// generators run inside `data.prove(pw)` (src/plonky2_semaphore/recursion.rs:72-86,167-168, wrapper.rs:49-55) -- interpreted by
// the GPU, so a unit's ~6.4 MB of witness rows are produced where the prover consumes them: the host uploads the inner proof's
// flat words (175 KB) instead of the rows, and spends no core on the 4 174 Poseidon gate rows + ~155 k field operations per unit.
//
// The tape is a straight-line program with a sequential part (the in-circuit transcript, openings, vanishing identity) and 28
// independent segments (the FRI query rounds; the builder has checked that a segment reads only the sequential part and
// itself).  One 64-lane wave interprets one (unit, segment): lane 0 executes the scalar entries in order; a POSEIDON entry --
// a whole PoseidonGate row, wire layout chip/plonk/gates/poseidon.rs:329-380 -- runs the lane-parallel permutation (one state
// element per lane, MDS row through a 24-slot LDS ring) and every lane stores the S-box-input wires it owns.  This is latency-
// bound work on a handful of waves (8 units x 29 waves): tens of milliseconds per batch, but it runs on the context's side stream
// under the proving of the previous batch and takes ~0.1 % of the chip's issue slots.
//
// What an entry does is witness_tape.h's tape_entry_exec, the host replay's own code.  Every entry passed tape_entry_fits when the
// artifact was loaded (tape_validate, witness_tape.cpp), so the interpreter does not bounds-check; data-dependent failures
// (ASSERT_EQ, range conditions = an invalid inner proof) are reported as the smallest failing entry per unit, exactly like the
// host replay.
#include "gl355_internal.h"
#include "poseidon_lanes.cuh"
#include "witness_tape.h"

namespace gl355 {

// stores of one lane -> loads of another lane of the same wave, through global memory.  The lanes share one CU and therefore
// one vector L1 (write-through): WORKGROUP scope is enough -- the stores only have to complete (s_waitcnt).  An agent-scope fence
// here also writes back and invalidates the XCD's L2, ~67 000 times per batch, and costs every other kernel on the chip its L2
// hits (measured: -5 % job throughput).
#define TAPE_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")

struct TapeDevArgs {
    const uint64_t* tape;          // [n_ops][5]
    const uint64_t* seg_start;     // [n_segs + 1] entry indices (seg_start[0] = n_seq)
    uint64_t n_seq;
    const uint64_t* inputs; uint64_t n_inputs;     // [units][n_inputs]
    uint64_t* rows; uint64_t n_words;              // [units][n_words]
    unsigned long long* status;                    // [units]: smallest failing entry, ~0 = none
};

// one PoseidonGate row: lanes 0..11 hold the state; wires as gl355_poseidon_gate_witness (host_transcript.cpp).  The rounds are psd_lane_round
// (poseidon_lanes.cuh); the row's own part is the swap, the S-box-input wires stored ahead of each round, and the output wires.
GL_DEV void tape_poseidon_row(uint64_t* row, int li, uint64_t* ring) {
    const bool active = li < 12;
    const int me = active ? li : 0;
    const uint64_t in = active ? row[li] : 0;
    const uint64_t swap = row[TAPE_POSEIDON_SWAP];
    uint64_t s = in;
    if (li < 8) {
        const uint64_t partner = row[li ^ 4];
        if (li < 4) {
            const uint64_t delta = swap ? gl_canon(gl_sub(partner, in)) : 0;       // swap * (rhs - lhs)
            row[25 + li] = delta;
            s = gl_add(in, delta);
        } else {
            const uint64_t delta = swap ? gl_canon(gl_sub(in, partner)) : 0;
            s = gl_sub(in, delta);
        }
    }
    s = gl_add_canonical(s, PSD_ALL_RC[me]);
#pragma unroll 1
    for (int r = 0; r < 30; r++) {
        const uint64_t rc_next = PSD_ALL_RC[12 * (r + 1) + me];
        const bool full = r < 4 || r >= 26;
        // the S-box input (state + round constants) is a wire of the gate except in the very first round
        if (active) {
            if (r >= 1 && r < 4) row[29 + 12 * (r - 1) + li] = gl_canon(s);
            else if (r >= 26) row[87 + 12 * (r - 26) + li] = gl_canon(s);
            else if (r >= 4 && r < 26 && li == 0) row[65 + (r - 4)] = gl_canon(s);
        }
        s = psd_lane_round(s, rc_next, full || li == 0, active, me, ring);
    }
    if (active) row[12 + li] = gl_canon(s);
}

__global__ void __launch_bounds__(64) tape_replay_kernel(TapeDevArgs a, uint32_t phase) {
    __shared__ uint64_t ring[24];
    const int lane = threadIdx.x;
    const uint32_t u = blockIdx.y;
    const uint64_t begin = phase == 0 ? 0 : a.seg_start[blockIdx.x];
    const uint64_t end = phase == 0 ? a.n_seq : a.seg_start[blockIdx.x + 1];
    uint64_t* W = a.rows + (uint64_t)u * a.n_words;
    const uint64_t* in = a.inputs + (uint64_t)u * a.n_inputs;
    for (uint64_t t = begin; t < end; t++) {
        const uint64_t* p = a.tape + 5 * t;
        const uint64_t e[5] = {p[0], p[1], p[2], p[3], p[4]};      // the whole entry at once: one load latency, not one per operand
        int fail = 0;
        if (e[0] == GL355_TAPE_POSEIDON) {
            uint64_t* row = W + e[1];
            TAPE_FENCE();
            if (!tape_poseidon_swap_ok(row)) fail = 1;
            else tape_poseidon_row(row, lane & 15, ring);      // lanes 16..63 mirror lanes 0..15 of their group: same values, same stores
            TAPE_FENCE();
        } else if (lane == 0) {
            fail = tape_entry_exec(e, in, W);
        }
        fail = __shfl(fail, 0);      // lane 0 decides (a POSEIDON failure is seen by every lane alike)
        if (fail) {
            if (lane == 0) atomicMin(a.status + u, (unsigned long long)t);
            break;
        }
    }
}

// public inputs of every unit: rows[pi_pos[i]]
__global__ void tape_gather_kernel(const uint64_t* rows, uint64_t n_words, const uint64_t* pi_pos, uint32_t n_pi, uint64_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
    if (i < n_pi) out[(uint64_t)u * n_pi + i] = rows[(uint64_t)u * n_words + pi_pos[i]];
}

// enqueue the replay of n_units units on `stream`: d_inputs [units][n_inputs] -> d_rows [units][n_words] (zeroed first),
// d_status [units] (smallest failing entry or ~0), d_pis [units][n_pi]
int32_t tape_replay_dev(hipStream_t stream, const uint64_t* d_tape, const uint64_t* d_seg_start, uint64_t n_seq, uint32_t n_segs, uint32_t n_units,
                        const uint64_t* d_inputs, uint64_t n_inputs, uint64_t* d_rows, uint64_t n_words, const uint64_t* d_pi_pos, uint32_t n_pi,
                        uint64_t* d_status, uint64_t* d_pis) {
    if (hipMemsetAsync(d_rows, 0, (size_t)n_units * n_words * 8, stream) != hipSuccess) return GL355_E_HIP;
    if (hipMemsetAsync(d_status, 0xFF, (size_t)n_units * 8, stream) != hipSuccess) return GL355_E_HIP;
    TapeDevArgs a;
    a.tape = d_tape; a.seg_start = d_seg_start; a.n_seq = n_seq; a.inputs = d_inputs; a.n_inputs = n_inputs;
    a.rows = d_rows; a.n_words = n_words; a.status = reinterpret_cast<unsigned long long*>(d_status);
    if (n_seq) hipLaunchKernelGGL(tape_replay_kernel, dim3(1, n_units), dim3(64), 0, stream, a, 0u);
    if (n_segs) hipLaunchKernelGGL(tape_replay_kernel, dim3(n_segs, n_units), dim3(64), 0, stream, a, 1u);
    if (n_pi) hipLaunchKernelGGL(tape_gather_kernel, dim3((n_pi + 63) / 64, n_units), dim3(64), 0, stream, d_rows, n_words, d_pi_pos, n_pi, d_pis);
    return hipGetLastError() == hipSuccess ? GL355_OK : GL355_E_HIP;
}

}  // namespace gl355
