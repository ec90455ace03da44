// Stand-alone check of the gate table (csrc/gate_shape.h) for tests/test_gate_shape_host.py, built under AddressSanitizer and UBSan with
// csrc/verifier.cpp, host_transcript.cpp and host_bn254.cpp.  One answer line per line of stdin:
//   type param num_wires num_constants num_routed   ->  ok wires constants constraints fits
//       ok = gate_shape; fits = gate_table_check of the one-gate descriptor with those three counts is GL355_OK (its refusal must name
//       gate 0 and the caller); gate_fits must say the same but for the routed wires, or the program exits 1
//   eval type param num_wires num_constants          ->  accepted constraints
//       the verifier's evaluator (gl355::verifier_eval_gate) on heap arrays of exactly num_wires extension elements and
//       num_constants constants: a read outside them is a sanitizer report, which aborts the run
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gl355_internal.h"

using namespace gl355;

namespace {

uint64_t rng_state = 0x6A7E5A9Eull;
uint64_t rnd() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a heap block of exactly n random extension elements
gl2* ext_block(uint32_t n) {
    gl2* p = (gl2*)malloc((size_t)n * sizeof(gl2));
    if (!p) { fprintf(stderr, "FAILED: out of memory\n"); exit(1); }
    for (uint32_t i = 0; i < n; i++) p[i] = gl2_make(rnd() % GL_P, rnd() % GL_P);
    return p;
}

}  // namespace

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long t, p, nw, nc, nr;
        if (sscanf(line, "eval %llu %llu %llu %llu", &t, &p, &nw, &nc) == 4) {
            gl2 *w = ext_block((uint32_t)nw), *k = ext_block((uint32_t)nc);
            const uint64_t pi_hash[4] = {rnd() % GL_P, rnd() % GL_P, rnd() % GL_P, rnd() % GL_P};
            const gl355_gate gt{(uint32_t)t, (uint32_t)p, 0, 0, 1};
            std::vector<gl2> c;
            const bool acc = verifier_eval_gate(gt, k, w, pi_hash, (uint32_t)nw, (uint32_t)nc, c);
            printf("%d %zu\n", (int)acc, c.size());
            free(w); free(k);
            continue;
        }
        if (sscanf(line, "%llu %llu %llu %llu %llu", &t, &p, &nw, &nc, &nr) != 5) { fprintf(stderr, "FAILED: cannot read '%s'\n", line); return 1; }
        GateShape s{0, 0, 0, 0}, s2;
        const bool ok = gate_shape((uint32_t)t, (uint32_t)p, s);
        gl355_circuit c;
        memset(&c, 0, sizeof c);
        c.num_wires = (uint32_t)nw; c.num_constants = (uint32_t)nc; c.num_routed_wires = (uint32_t)nr; c.num_selectors = 1; c.num_gates = 1;
        c.gates[0] = gl355_gate{(uint32_t)t, (uint32_t)p, 0, 0, 1};
        char msg[GATE_MSG_LEN];
        const int32_t rc = gate_table_check(c, "check", msg);
        const bool fits = rc == GL355_OK;
        if (fits ? msg[0] != 0 : rc != GL355_E_INVALID_ARG || strncmp(msg, "check: gate 0", 13) != 0) {
            fprintf(stderr, "FAILED: gate_table_check returns %d with the message '%s' for '%s'\n", rc, msg, line);
            return 1;
        }
        if (gate_fits((uint32_t)t, (uint32_t)p, (uint32_t)nw, (uint32_t)nc, s2) != (ok && s.wires <= nw && s.constants <= nc) ||
            fits != (ok && s.wires <= nw && s.constants <= nc && s.routed <= nr)) {
            fprintf(stderr, "FAILED: gate_shape, gate_fits and gate_table_check disagree for '%s'\n", line);
            return 1;
        }
        if (ok) printf("1 %u %u %u %d\n", s.wires, s.constants, s.constraints, (int)fits);
        else printf("0 0 0 0 %d\n", (int)fits);
    }
    return 0;
}
