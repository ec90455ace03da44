// One entry {op, a, b, c, d} of the witness tape (include/gl355.h GL355_TAPE_*): what it touches and what it does, stated once for the
// host replay (witness_tape.cpp), the static check of a loaded artifact (tape_validate) and the device interpreter
// (witness_tape_dev.hip).  tape_entry_fits is all that stands between an untrusted tape and an access outside the rows:
// tape_entry_exec checks no offset.  The host runs both per entry; the device runs exec alone on a tape that passed fits at load.
// A POSEIDON entry has only its pre-condition here: the row is gl355_poseidon_gate_witness on the host and the lane-parallel
// tape_poseidon_row on the device.  Wire layouts follow the reference's chip/plonk/gates/*.rs (arithmetic.rs, arithmetic_extension.rs,
// poseidon.rs:329-380, poseidon_mds.rs, base_sum.rs, random_access.rs, reducing.rs, reducing_extension.rs) and coset_interp.h.
#pragma once
#include "../../include/gl355.h"
#include "coset_interp.h"
#include "gate_shape.h"

namespace gl355 {

// RandomAccessGate{bits 4, copies 4, extra constants 2}, the one shape the entry knows: a copy is {index, claimed element, 16 items},
// the index bits of all copies follow the two constants behind the last copy
enum { TAPE_RA_BITS = 4, TAPE_RA_COPIES = 4, TAPE_RA_STRIDE = 2 + (1 << TAPE_RA_BITS), TAPE_RA_BIT_WIRES = TAPE_RA_COPIES * TAPE_RA_STRIDE + 2 };
static_assert(TAPE_RA_STRIDE == 18 && TAPE_RA_BIT_WIRES == 74, "random_access.rs wire layout");
enum { TAPE_POSEIDON_SWAP = 24 };      // PoseidonGate's swap wire

// Does everything the entry reads and writes lie inside inputs[n_inputs] and W[n_words]?  Rows are num_wires >= 135 wide (the callers'
// pre-condition: the widest fixed layout here, PoseidonGate, has 135 wires).  No sum of operands is formed, so nothing wraps;
// the spans of BASE_SUM and REDUCING are their gates' (gate_shape.h).
GL_HD bool tape_entry_fits(const uint64_t* e, uint64_t n_inputs, uint64_t n_words, uint32_t num_wires) {
    const uint64_t a = e[1], b = e[2], c = e[3], d = e[4];
    auto ok = [&](uint64_t i, uint64_t span) { return i < n_words && span <= n_words - i; };
    auto row = [&](uint64_t i) { return ok(i, num_wires) && i % num_wires == 0; };
    // a gate of `count` limbs or coefficients inside a row: count is compared with num_wires before it is narrowed to the 32 bits of a gate parameter
    auto gate = [&](uint32_t type, uint64_t count) { GateShape g; return count <= num_wires && gate_fits(type, (uint32_t)count, num_wires, 0, g); };
    switch (e[0]) {
    case GL355_TAPE_CONST: return ok(a, 1);
    case GL355_TAPE_INPUT: return ok(a, 1) && b < n_inputs;
    case GL355_TAPE_COPY: case GL355_TAPE_ASSERT_EQ: case GL355_TAPE_LO32: case GL355_TAPE_HI32: return ok(a, 1) && ok(b, 1);
    case GL355_TAPE_ARITH: return ok(a, 4);
    case GL355_TAPE_ARITH_EXT: return ok(a, 8);
    case GL355_TAPE_POSEIDON: case GL355_TAPE_MDS_EXT: return row(a);
    case GL355_TAPE_BASE_SUM: return row(a) && b <= 63 && gate(GL355_GATE_BASE_SUM, b);
    case GL355_TAPE_RANDOM_ACCESS: return row(a) && b < TAPE_RA_COPIES;
    case GL355_TAPE_REDUCING: return row(a) && gate(c ? GL355_GATE_REDUCING_EXT : GL355_GATE_REDUCING, b);
    case GL355_TAPE_EXT_INV: return ok(a, 1) && ok(b, 1) && ok(c, 1) && ok(d, 1);
    case GL355_TAPE_COSET_INTERP: {
        CosetInterpShape s;
        return row(a) && b <= 0xFF && c <= 0xFF && coset_interp_shape((uint32_t)(b | c << 8), s) && s.num_wires <= num_wires;
    }
    default: return false;
    }
}

// a POSEIDON entry runs only on a row whose swap wire is a bit
GL_HD bool tape_poseidon_swap_ok(const uint64_t* row) { return row[TAPE_POSEIDON_SWAP] <= 1; }

// Executes an entry that passed tape_entry_fits, any opcode but POSEIDON.  0, or 1 when the data refuse it: ASSERT_EQ of unequal
// words, a BASE_SUM value of more than b bits, a RANDOM_ACCESS index >= 16, EXT_INV of (0, 0), COSET_INTERP with a zero shift.
GL_HD int tape_entry_exec(const uint64_t* e, const uint64_t* inputs, uint64_t* W) {
    const uint64_t x = e[1], b = e[2], c = e[3], d = e[4];
    switch (e[0]) {
    case GL355_TAPE_CONST: W[x] = gl_canon(b); break;
    case GL355_TAPE_INPUT: W[x] = gl_canon(inputs[b]); break;
    case GL355_TAPE_COPY: W[x] = W[b]; break;
    case GL355_TAPE_ASSERT_EQ: return W[x] != W[b];
    case GL355_TAPE_ARITH:      // {m0, m1, addend, out}: out = b m0 m1 + c addend
        W[x + 3] = gl_canon(gl_add(gl_mul(gl_mul(W[x], W[x + 1]), b), gl_mul(W[x + 2], c)));
        break;
    case GL355_TAPE_ARITH_EXT: {
        const gl2 pr = gl2_mul(gl2_make(W[x], W[x + 1]), gl2_make(W[x + 2], W[x + 3]));
        const gl2 r = gl2_canon(gl2_add(gl2_mul_base(pr, b), gl2_mul_base(gl2_make(W[x + 4], W[x + 5]), c)));
        W[x + 6] = r.c0; W[x + 7] = r.c1;
        break;
    }
    case GL355_TAPE_MDS_EXT:      // 12 extension inputs at wire 0 -> 12 outputs at wire 24
        for (int r = 0; r < 12; r++)
            for (int k = 0; k < 2; k++) {
                uint64_t acc = 0;
                for (int i = 0; i < 12; i++) acc = gl_add(acc, gl_mul_small(W[x + 2 * ((i + r) % 12) + k], GL_PSD_MDS_CIRC[i]));
                if (r == 0) acc = gl_add(acc, gl_mul_small(W[x + k], GL_PSD_MDS_DIAG0));
                W[x + 2 * (12 + r) + k] = gl_canon(acc);
            }
        break;
    case GL355_TAPE_BASE_SUM: {      // wire 0 -> b little-endian bits at wire 1
        const uint64_t v = W[x];
        if (v >> b) return 1;
        for (uint64_t i = 0; i < b; i++) W[x + 1 + i] = (v >> i) & 1;
        break;
    }
    case GL355_TAPE_RANDOM_ACCESS: {      // copy b: the claimed element and the index bits
        const uint64_t idx = W[x + TAPE_RA_STRIDE * b];
        if (idx >> TAPE_RA_BITS) return 1;
        W[x + TAPE_RA_STRIDE * b + 1] = W[x + TAPE_RA_STRIDE * b + 2 + idx];
        for (int k = 0; k < TAPE_RA_BITS; k++) W[x + TAPE_RA_BIT_WIRES + TAPE_RA_BITS * b + k] = (idx >> k) & 1;
        break;
    }
    case GL355_TAPE_REDUCING: {      // b = number of coefficients, c = 1 for ReducingExtensionGate
        const uint64_t n = b, ext = c;
        const uint64_t start_accs = 6 + (ext ? 2 * n : n);
        const gl2 alpha = gl2_make(W[x + 2], W[x + 3]);
        gl2 acc = gl2_make(W[x + 4], W[x + 5]);
        for (uint64_t i = 0; i < n; i++) {
            const gl2 cf = ext ? gl2_make(W[x + 6 + 2 * i], W[x + 7 + 2 * i]) : gl2_make(W[x + 6 + i], 0);
            acc = gl2_canon(gl2_add(gl2_mul(acc, alpha), cf));
            const uint64_t o = i == n - 1 ? 0 : start_accs + 2 * i;
            W[x + o] = acc.c0; W[x + o + 1] = acc.c1;
        }
        break;
    }
    case GL355_TAPE_LO32: W[x] = W[b] & 0xFFFFFFFFull; break;
    case GL355_TAPE_HI32: W[x] = W[b] >> 32; break;
    case GL355_TAPE_EXT_INV: {      // (a, b) <- ([c], [d])^-1
        if (W[c] == 0 && W[d] == 0) return 1;
        const gl2 r = gl2_canon(gl2_inv(gl2_make(W[c], W[d])));
        W[x] = r.c0; W[b] = r.c1;
        break;
    }
    case GL355_TAPE_COSET_INTERP: {      // b = subgroup bits, c = degree: shift, values and point are set, the rest is filled
        CosetInterpShape s;
        coset_interp_shape((uint32_t)(b | c << 8), s);
        return coset_interp_fill(s, W + x);
    }
    default: return 1;
    }
    return 0;
}

}  // namespace gl355
