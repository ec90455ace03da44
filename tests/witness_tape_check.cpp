// Stand-alone check of the witness tape's entry contract for tests/test_witness_tape_host.py, built under AddressSanitizer and UBSan
// with csrc/witness_tape.cpp, host_transcript.cpp and host_bn254.cpp: what tape_entry_fits (csrc/witness_tape.h) accepts, the host
// replay executes inside its rows; what it refuses, gl355_witness_replay refuses with GL355_E_INVALID_ARG at that entry.  The rows
// and the inputs are heap blocks of exactly the stated size, so an access outside them is a sanitizer report, which aborts the run.
// Every tape has one entry.  Prints one line per group of cases and exits 0, or names the first failing case and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "witness_tape.h"

using namespace gl355;

namespace {

constexpr uint32_t NW = 135;
constexpr uint64_t N_ROWS = 3, N_WORDS = N_ROWS * NW, N_INPUTS = 8, NONE = ~0ull;
constexpr uint64_t WRAP3 = 6148914691236517204ull;      // (2^64 - 4) / 3: 3 b + 4 = 2^64
static_assert(3 * WRAP3 + 4 == 0 && 4 * (1ull << 62) + 4 == 4, "the sums that wrapped");

// the test's own statement of an entry's operands: which of a..d the check looks at, which are wire offsets, and the span of a wire offset
struct OpInfo { const char* name; unsigned checked, wires; uint64_t span; };
const OpInfo OPS[15] = {
    {"CONST", 1, 1, 1}, {"INPUT", 3, 1, 1}, {"COPY", 3, 3, 1}, {"ASSERT_EQ", 3, 3, 1}, {"ARITH", 1, 1, 4}, {"ARITH_EXT", 1, 1, 8},
    {"POSEIDON", 1, 1, NW}, {"MDS_EXT", 1, 1, NW}, {"BASE_SUM", 3, 1, NW}, {"RANDOM_ACCESS", 3, 1, NW}, {"REDUCING", 7, 1, NW},
    {"LO32", 3, 3, 1}, {"HI32", 3, 3, 1}, {"EXT_INV", 15, 15, 1}, {"COSET_INTERP", 7, 1, NW}};
bool is_row_op(uint64_t op) { return op < 15 && OPS[op].span == NW; }

uint64_t rng_state = 0x7A9E355ull;
uint64_t rnd() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return rnd() % n; }
uint64_t word() { return below(4) ? rnd() % GL_P : below(20); }      // canonical; one in four is small, so that range conditions also hold

struct Entry { uint64_t e[5]; };
Entry entry(uint64_t op, uint64_t a, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0) { return Entry{{op, a, b, c, d}}; }

[[noreturn]] void die(const char* what, const Entry& t, long rc, uint64_t failed) {
    fprintf(stderr, "FAILED %s: entry {%llu, %llu, %llu, %llu, %llu} rc %ld failed_op %llu\n", what, (unsigned long long)t.e[0], (unsigned long long)t.e[1],
            (unsigned long long)t.e[2], (unsigned long long)t.e[3], (unsigned long long)t.e[4], rc, (unsigned long long)failed);
    exit(1);
}

// The one-entry tape through the C ABI on fresh heap blocks.  true = accepted (GL355_OK, or GL355_E_WITNESS at entry 0), false = refused
// (GL355_E_INVALID_ARG at entry 0); anything else, or a disagreement with tape_entry_fits, ends the run.
bool replay(const Entry& t, const char* what) {
    std::vector<uint64_t> tape(t.e, t.e + 5), inputs(N_INPUTS), rows(N_WORDS, 0x5555555555555555ull);
    for (auto& v : inputs) v = rnd();      // any u64: INPUT canonicalises
    uint64_t failed = 12345;
    const int32_t rc = gl355_witness_replay(tape.data(), 1, inputs.data(), N_INPUTS, rows.data(), N_WORDS, NW, &failed);
    const bool fits = tape_entry_fits(t.e, N_INPUTS, N_WORDS, NW);
    const bool consistent = fits ? (rc == GL355_OK && failed == NONE) || (rc == GL355_E_WITNESS && failed == 0) : rc == GL355_E_INVALID_ARG && failed == 0;
    if (!consistent) die(what, t, rc, failed);
    for (uint64_t v : rows)
        if (v >= GL_P) die("a row word is not canonical", t, rc, failed);
    return fits;
}
void accepted(const Entry& t, const char* what) { if (!replay(t, what)) die(what, t, GL355_E_INVALID_ARG, 0); }
void refused(const Entry& t, const char* what) { if (replay(t, what)) die(what, t, 0, NONE); }

// an accepted entry on rows of random canonical words (the replay itself starts from zero rows): the executor stays inside them
void exec_on_random_rows(const Entry& t) {
    if (t.e[0] == GL355_TAPE_POSEIDON) return;
    std::vector<uint64_t> inputs(N_INPUTS), rows(N_WORDS);
    for (auto& v : inputs) v = rnd();
    for (auto& v : rows) v = word();
    const int r = tape_entry_exec(t.e, inputs.data(), rows.data());
    if (r != 0 && r != 1) die("tape_entry_exec returns 0 or 1", t, r, 0);
    for (uint64_t v : rows)
        if (v >= GL_P) die("tape_entry_exec left a word that is not canonical", t, r, 0);
}

uint64_t any_row() { return NW * below(N_ROWS); }
bool coset_ok(uint64_t bits, uint64_t degree) {
    CosetInterpShape s;
    return bits <= 0xFF && degree <= 0xFF && coset_interp_shape((uint32_t)(bits | degree << 8), s) && s.num_wires <= NW;
}
// a valid entry of `op`; operands the entry does not use are arbitrary
Entry valid(uint64_t op) {
    Entry t = entry(op, 0, rnd(), rnd(), rnd());
    const OpInfo& o = OPS[op];
    for (int j = 0; j < 4; j++)
        if (o.wires >> j & 1) t.e[1 + j] = is_row_op(op) ? any_row() : below(N_WORDS - o.span + 1);
    switch (op) {
    case GL355_TAPE_INPUT: t.e[2] = below(N_INPUTS); break;
    case GL355_TAPE_BASE_SUM: t.e[2] = below(64); break;
    case GL355_TAPE_RANDOM_ACCESS: t.e[2] = below(4); break;
    case GL355_TAPE_REDUCING: t.e[3] = below(2); t.e[2] = 1 + below(t.e[3] ? 32 : 43); break;
    case GL355_TAPE_COSET_INTERP: t.e[2] = 2 + below(3); t.e[3] = 2 + below((1ull << t.e[2]) - 1); break;
    default: break;
    }
    return t;
}

void named_reducing_cases() {
    for (uint64_t a = 0; a < N_WORDS; a += NW) {
        const uint64_t bad[6][2] = {{1ull << 62, 1}, {(1ull << 62) + 32, 1}, {WRAP3, 0}, {0, 0}, {44, 0}, {33, 1}};
        for (auto& bc : bad) refused(entry(GL355_TAPE_REDUCING, a, bc[0], bc[1]), "REDUCING with a count that does not fit 135 wires");
        accepted(entry(GL355_TAPE_REDUCING, a, 43, 0), "REDUCING 43 base coefficients: 3 n + 4 <= 135");
        accepted(entry(GL355_TAPE_REDUCING, a, 32, 1), "REDUCING 32 extension coefficients: 4 n + 4 <= 135");
    }
    puts("named REDUCING cases: ok");
}

void boundaries() {
    for (uint64_t op = 0; op < 15; op++) {
        const OpInfo& o = OPS[op];
        for (int j = 0; j < 4; j++) {
            if (!(o.wires >> j & 1)) continue;
            Entry t = valid(op);
            t.e[1 + j] = N_WORDS - o.span;
            accepted(t, "an operand at n_words - span");
            t.e[1 + j] = N_WORDS - o.span + 1;
            refused(t, "an operand at n_words - span + 1");
        }
        if (is_row_op(op))
            for (uint64_t k = 0; k < N_ROWS; k++) {
                Entry t = valid(op);
                t.e[1] = NW * k + 1;
                refused(t, "a row operand that is no row start");
            }
    }
    accepted(entry(GL355_TAPE_INPUT, 7, N_INPUTS - 1), "INPUT b = n_inputs - 1");
    refused(entry(GL355_TAPE_INPUT, 7, N_INPUTS), "INPUT b = n_inputs");
    accepted(entry(GL355_TAPE_BASE_SUM, NW, 63), "BASE_SUM b = 63");
    refused(entry(GL355_TAPE_BASE_SUM, NW, 64), "BASE_SUM b = 64");
    accepted(entry(GL355_TAPE_RANDOM_ACCESS, NW, 3), "RANDOM_ACCESS b = 3");
    refused(entry(GL355_TAPE_RANDOM_ACCESS, NW, 4), "RANDOM_ACCESS b = 4");
    unsigned n_ok = 0;
    for (uint64_t bits = 0; bits <= 6; bits++)
        for (uint64_t degree = 0; degree <= 18; degree++) {
            const Entry t = entry(GL355_TAPE_COSET_INTERP, 2 * NW, bits, degree);
            if (coset_ok(bits, degree)) { accepted(t, "COSET_INTERP parameters coset_interp_shape accepts"); n_ok++; }
            else refused(t, "COSET_INTERP parameters coset_interp_shape refuses");
        }
    if (n_ok != 3 + 7 + 15) die("COSET_INTERP: bits 2..4 with degree 2..2^bits are the accepted shapes", entry(GL355_TAPE_COSET_INTERP, 0), n_ok, 0);
    refused(entry(GL355_TAPE_COSET_INTERP, 0, 256, 2), "COSET_INTERP b = 256");
    refused(entry(GL355_TAPE_COSET_INTERP, 0, 258, 2), "COSET_INTERP b = 256 + 2");
    refused(entry(GL355_TAPE_COSET_INTERP, 0, 2, 256), "COSET_INTERP c = 256");
    refused(entry(15, 0), "opcode 15");
    refused(entry((1ull << 32) + GL355_TAPE_CONST, 0), "opcode 2^32");
    puts("boundaries of every opcode: ok");
}

void sweep() {
    unsigned n_acc[15] = {0}, n_ref[15] = {0};
    for (int i = 0; i < 20000; i++) {
        const uint64_t op = below(15);
        const OpInfo& o = OPS[op];
        Entry t = valid(op);
        if (below(2)) {      // one operand the check looks at is replaced
            int j;
            do j = (int)below(4); while (!(o.checked >> j & 1));
            const uint64_t top = N_WORDS - o.span;
            const uint64_t repl[15] = {0, 1, 134, 135, 136, top - 1, top, top + 1, N_WORDS, 1ull << 32, 1ull << 62, (1ull << 62) + 32, WRAP3, 1ull << 63, ~0ull};
            t.e[1 + j] = repl[below(15)];
        }
        if (replay(t, "sweep")) { n_acc[op]++; exec_on_random_rows(t); }
        else n_ref[op]++;
    }
    bool thin = false;
    for (int op = 0; op < 15; op++) {
        const unsigned n = n_acc[op] + n_ref[op];
        printf("sweep %-14s %5u entries: %5.1f %% accepted, %5.1f %% refused\n", OPS[op].name, n, 100.0 * n_acc[op] / n, 100.0 * n_ref[op] / n);
        if (4 * n_acc[op] < n || 10 * n_ref[op] < n) thin = true;
    }
    if (thin) { fprintf(stderr, "FAILED sweep: an opcode has under 25 %% accepted or under 10 %% refused entries\n"); exit(1); }
}

}  // namespace

int main() {
    named_reducing_cases();
    boundaries();
    sweep();
    return 0;
}
