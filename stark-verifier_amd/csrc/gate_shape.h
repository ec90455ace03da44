// What a gate (type, param) of a gl355_circuit reads and how many constraints it pushes, stated once for the verifier
// (verifier.cpp eval_gate), the quotient launcher (quotient.hip), gl355_quotient* (capi.hip), the artifact loader (circuit.hip) and
// the witness tape's BASE_SUM / REDUCING entries (witness_tape.h).  The device evaluators (quotient.hip gate_*) and the
// verifier's index their columns without a check of their own: gate_table_check is all that stands between an untrusted
// descriptor and a read outside the wires or the gate constants.  Wire layouts: chip/plonk/gates/*.rs, coset_interp.h.
#pragma once
#include <stdio.h>

#include "../../include/gl355.h"
#include "coset_interp.h"

namespace gl355 {

struct GateShape {
    uint32_t wires;        // one more than the largest wire index an evaluator of the gate reads
    uint32_t constants;    // gate constants (the columns behind the selectors) it reads
    uint32_t constraints;  // num_constraints of plonky2's gates/*.rs
    uint32_t routed;       // routed wires the quotient launcher insists on: CosetInterpolationGate's start_int, else 0
};

// false: an unknown type, a parameter that describes no gate (RANDOM_ACCESS with more than 8 bits, REDUCING* without a
// coefficient, what coset_interp_shape refuses) or whose shape does not fit 32 bits.  param is untrusted: every product is
// formed in 64 bits.  ARITHMETIC, ARITHMETIC_EXT and MUL_EXT read their constants whatever the number of operations is.
GL_HD bool gate_shape(uint32_t type, uint32_t param, GateShape& s) {
    const uint64_t p = param;
    uint64_t wires = 0, constants = 0, constraints = 0, routed = 0;
    switch (type) {
    case GL355_GATE_NOOP: break;
    case GL355_GATE_CONSTANT: wires = constants = constraints = p; break;
    case GL355_GATE_PUBLIC_INPUT: wires = constraints = 4; break;
    case GL355_GATE_BASE_SUM: wires = constraints = 1 + p; break;
    case GL355_GATE_POSEIDON: wires = 135; constraints = 123; break;
    case GL355_GATE_ARITHMETIC: wires = 4 * p; constants = 2; constraints = p; break;
    case GL355_GATE_ARITHMETIC_EXT: wires = 8 * p; constants = 2; constraints = 2 * p; break;
    case GL355_GATE_MUL_EXT: wires = 6 * p; constants = 1; constraints = 2 * p; break;
    case GL355_GATE_POSEIDON_MDS: wires = 48; constraints = 24; break;
    case GL355_GATE_RANDOM_ACCESS: {      // copies x {index, claimed element, 2^bits items} | extra constants | copies x bits
        const uint64_t bits = p & 0xFF, copies = (p >> 8) & 0xFF, extra = (p >> 16) & 0xFF;
        if (bits > 8) return false;
        wires = (2 + (1ull << bits)) * copies + extra + copies * bits;
        constants = extra;
        constraints = copies * (bits + 2) + extra;
        break;
    }
    case GL355_GATE_REDUCING:
    case GL355_GATE_REDUCING_EXT:         // output, alpha, old accumulator | coefficients | all accumulators but the last
        if (p == 0) return false;
        wires = 6 + (type == GL355_GATE_REDUCING_EXT ? 2 * p : p) + 2 * (p - 1);
        constraints = 2 * p;
        break;
    case GL355_GATE_COSET_INTERPOLATION: {
        CosetInterpShape c;
        if (!coset_interp_shape(param, c)) return false;
        wires = c.num_wires; constraints = c.num_constraints; routed = c.start_int;
        break;
    }
    default: return false;
    }
    if (wires > 0xFFFFFFFFull || constraints > 0xFFFFFFFFull) return false;
    s.wires = (uint32_t)wires; s.constants = (uint32_t)constants; s.constraints = (uint32_t)constraints; s.routed = (uint32_t)routed;
    return true;
}

// Does the gate exist, and do its wires and constants lie inside a circuit of num_wires wires and num_constants gate constants?
GL_HD bool gate_fits(uint32_t type, uint32_t param, uint32_t num_wires, uint32_t num_constants, GateShape& s) {
    return gate_shape(type, param, s) && s.wires <= num_wires && s.constants <= num_constants;
}

// Everything the gate table of a descriptor must satisfy before a kernel sees it.  GL355_OK, or GL355_E_INVALID_ARG with
// "<who>: gate <index> ..." in msg.
constexpr int GATE_MSG_LEN = 160;
inline int32_t gate_table_check(const gl355_circuit& c, const char* who, char msg[GATE_MSG_LEN]) {
    static const char* const NAMES[GL355_GATE_TYPE_MAX + 1] = {
        "NoopGate", "ConstantGate", "PublicInputGate", "BaseSumGate", "PoseidonGate", "ArithmeticGate", "ArithmeticExtensionGate",
        "MulExtensionGate", "PoseidonMdsGate", "RandomAccessGate", "ReducingGate", "ReducingExtensionGate", "CosetInterpolationGate"};
    msg[0] = 0;
    if (c.num_gates > GL355_MAX_GATES) {
        snprintf(msg, GATE_MSG_LEN, "%s: more than %d gates", who, GL355_MAX_GATES);
        return GL355_E_INVALID_ARG;
    }
    for (uint32_t g = 0; g < c.num_gates; g++) {
        const gl355_gate& gt = c.gates[g];
        GateShape s;
        if (gt.type > GL355_GATE_TYPE_MAX) snprintf(msg, GATE_MSG_LEN, "%s: gate %u has the unknown type %u", who, g, gt.type);
        else if (gt.selector_index >= c.num_selectors || gt.group_end > c.num_gates || gt.group_start > gt.group_end)
            snprintf(msg, GATE_MSG_LEN, "%s: gate %u (%s) has a bad selector group", who, g, NAMES[gt.type]);
        else if (!gate_shape(gt.type, gt.param, s))
            snprintf(msg, GATE_MSG_LEN, "%s: gate %u: no %s has the parameter 0x%x", who, g, NAMES[gt.type], gt.param);
        else if (s.wires > c.num_wires || s.constants > c.num_constants || s.routed > c.num_routed_wires)
            snprintf(msg, GATE_MSG_LEN, "%s: gate %u (%s, parameter 0x%x) does not fit: it reads %u wires (%u routed) and %u constants", who, g,
                     NAMES[gt.type], gt.param, s.wires, s.routed, s.constants);
        if (msg[0]) return GL355_E_INVALID_ARG;
    }
    return GL355_OK;
}

}  // namespace gl355
