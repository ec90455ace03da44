// The circuit artifact (include/gl355.h "circuit artifacts", plonk.py export_blob) as gl355_circuit_load reads it,
// stated once and for the host alone: the table of header words, the version rules, the view of a parsed artifact and artifact_parse,
// the complete check of an untrusted artifact short of the commitment (the digest or cap comparison needs the device and stays in
// circuit.hip).  The loader, the provers' kernels, both tape interpreters and the verifier read a loaded circuit unchecked:
// artifact_parse is all that stands between an exporter's output and them.  Every header word is compared as the 64-bit word it is
// before it is narrowed, and every sum and product is formed in 64 bits.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/gl355.h"
#include "gate_shape.h"

namespace gl355 {

uint64_t tape_validate(const uint64_t* tape, uint64_t n_ops, uint64_t n_inputs, uint64_t n_words, uint32_t num_wires);      // witness_tape.cpp

// ---- the header: X(name, index); plonk.py ARTIFACT_WORDS states the same table for the writer --------------------------------------
#define GL355_ART_WORDS(X)                                                                                                             \
    X(MAGIC, 0) X(VERSION, 1)                                                                                                          \
    X(DEGREE_BITS, 2) X(RATE_BITS, 3) X(NUM_WIRES, 4) X(NUM_ROUTED_WIRES, 5) X(NUM_CONSTANTS, 6) X(NUM_SELECTORS, 7)                   \
    X(NUM_CHALLENGES, 8) X(MAX_DEGREE, 9) X(NUM_PARTIAL_PRODUCTS, 10) X(NUM_GATES, 11)                                                 \
    X(GATES, 12) /* GL355_MAX_GATES x {type, param, selector_index, group_start, group_end} */                                        \
    X(CAP_HEIGHT, 92) X(POW_BITS, 93) X(NUM_QUERIES, 94) X(N_FRI_LAYERS, 95) X(ZERO_KNOWLEDGE, 96) X(HASHER, 97)                       \
    X(BLIND_START, 98) X(N_BLIND, 99) X(Z_START, 100) X(N_Z_PAIRS, 101)                                                                \
    X(N_ROWS, 102) X(N_OPS, 103) X(N_INPUTS, 104) X(N_PI, 105)                                                                         \
    X(DIGEST, 106) /* 4 words */                                                                                                       \
    X(N_SEQ, 110) X(N_SEGS, 111) X(HDR_WORDS, 112)
enum {
#define X(name, at) ART_##name = at,
    GL355_ART_WORDS(X)
#undef X
};
struct ArtName { const char* name; uint32_t at; };
constexpr ArtName ART_NAMES[] = {
#define X(name, at) {"ART_" #name, at},
    GL355_ART_WORDS(X)
#undef X
};
enum { ART_GATE_TYPE, ART_GATE_PARAM, ART_GATE_SELECTOR, ART_GATE_GROUP_START, ART_GATE_GROUP_END, ART_GATE_WORDS };
static_assert(ART_GATES + ART_GATE_WORDS * GL355_MAX_GATES == ART_CAP_HEIGHT, "the gate table ends where the FRI parameters begin");
static_assert(ART_DIGEST + 4 == ART_N_SEQ, "four digest words");

constexpr uint64_t ART_MAGIC_VALUE = 0x5249433535334c47ull;      // "GL355CIR" little endian
constexpr uint64_t ART_VERSION_MIN = 2, ART_VERSION_MAX = 5;
// versions 3 and 5: the digest was computed elsewhere and is taken as given; the artifact ends with the expected constants_sigmas cap
inline bool art_external_digest(uint64_t version) { return version == 3 || version == 5; }
// versions 4 and 5: the arity bits of the FRI layers, n_fri_layers words directly after the header (2 and 3: every layer folds by 2)
inline bool art_arity_table(uint64_t version) { return version >= 4; }
constexpr uint32_t ART_MAX_FRI_LAYERS = 32;

// ---- what artifact_parse can say, after "circuit_load: ": X(name, code, text).  gate_table_check (gate_shape.h) adds its own four,
// which name the gate.  The last six are conditions on the circuit that every use of a handle refused or crashed on (prove_units,
// gl355_verify, gl355_commit_h); what only the prover asks (a final polynomial of two coefficients, at most 16 partial-product chunks,
// an LDE of at most 2^27 points) stays with the prover, since a handle may serve gl355_circuit_verify alone.
#define GL355_ART_REFUSALS(X)                                                                                                          \
    X(TRUNCATED, GL355_E_INVALID_ARG, "null or truncated artifact")                                                                    \
    X(VERSION, GL355_E_INVALID_ARG, "not a version-2..5 gl355 circuit artifact")                                                       \
    X(SHAPE, GL355_E_INVALID_ARG, "implausible circuit shape")                                                                         \
    X(GATE_PARAM, GL355_E_INVALID_ARG, "gate parameter out of range")                                                                  \
    X(GATE_WORD, GL355_E_INVALID_ARG, "a gate's type, selector or group is no 32-bit value")                                           \
    X(SIZES, GL355_E_INVALID_ARG, "implausible sizes")                                                                                 \
    X(SEGMENTATION, GL355_E_INVALID_ARG, "implausible tape segmentation")                                                              \
    X(CAP_HEIGHT, GL355_E_INVALID_ARG, "implausible cap height")                                                                       \
    X(FRI_LAYERS, GL355_E_INVALID_ARG, "implausible number of FRI layers")                                                             \
    X(LENGTH, GL355_E_INVALID_ARG, "artifact length does not match its header")                                                        \
    X(HASHER, GL355_E_INVALID_ARG, "unknown hasher")                                                                                   \
    X(ARITY_WORD, GL355_E_INVALID_ARG, "a FRI layer's arity bits are zero or no 32-bit value")                                         \
    X(ARITY_WIDE, GL355_E_UNSUPPORTED, "a FRI layer folds by 2, 4, 8 or 16")                                                           \
    X(ARITY_SUM, GL355_E_INVALID_ARG, "the FRI layers fold below one coefficient")                                                     \
    X(ARITY_CAP, GL355_E_INVALID_ARG, "a FRI layer is narrower than the cap")                                                          \
    X(ROW_INDEX, GL355_E_INVALID_ARG, "witness row index out of range")                                                                \
    X(PI_POSITION, GL355_E_INVALID_ARG, "public-input position out of range")                                                          \
    X(SEGMENTS, GL355_E_INVALID_ARG, "tape segments do not add up")                                                                    \
    X(BLINDING, GL355_E_INVALID_ARG, "blinding rows out of range")                                                                     \
    X(TAPE, GL355_E_INVALID_ARG, "malformed witness tape")                                                                             \
    X(PARAM_WORD, GL355_E_INVALID_ARG, "pow_bits, num_queries or zero_knowledge is no 32-bit value")                                   \
    X(MAX_DEGREE, GL355_E_INVALID_ARG, "max_degree is zero")                                                                           \
    X(CHALLENGES, GL355_E_UNSUPPORTED, "1 to 4 challenges")                                                                            \
    X(PARTIAL_PRODUCTS, GL355_E_INVALID_ARG, "inconsistent partial-product count")                                                     \
    X(SIZE, GL355_E_UNSUPPORTED, "unsupported size")                                                                                   \
    X(CAP_TOO_LARGE, GL355_E_INVALID_ARG, "cap_height too large")
enum ArtRefusal {
#define X(name, code, text) ART_R_##name,
    GL355_ART_REFUSALS(X)
#undef X
};
struct ArtRefusalText { int32_t code; const char* text; };
constexpr ArtRefusalText ART_REFUSALS[] = {
#define X(name, code, text) {code, text},
    GL355_ART_REFUSALS(X)
#undef X
};
constexpr int ART_MSG_LEN = GATE_MSG_LEN;
constexpr const char* ART_WHO = "circuit_load";

// ---- a parsed artifact: every field narrowed after its check, every section a pointer into the caller's words ------------------------
struct ArtifactView {
    struct Section { const uint64_t* p; uint64_t words; };
    uint32_t version;
    bool external_digest, arity_table;
    gl355_circuit c;                                  // gate slots from num_gates on are zero, whatever the artifact holds there
    uint32_t cap_height, pow_bits, num_queries, n_fri_layers;
    int32_t zero_knowledge, hasher;
    uint32_t fri_arity_bits[ART_MAX_FRI_LAYERS];      // [n_fri_layers]: the table, all ones for versions 2 and 3
    uint32_t blind_start, n_blind, z_start, n_z_pairs;
    uint64_t n_rows, n_ops, n_inputs, n_pi, n_seq, n_segs;
    const uint64_t* digest;                           // 4 words: this framework's digest (checked by the loader) or, versions 3 / 5, the one given
    // arity table | constants [num_selectors + num_constants][n] | sigmas [routed][n] | k_is [routed] | row_idx [n_rows] | pi positions [n_pi] |
    // tape [n_ops][5] | segment lengths [n_segs] | versions 3 / 5: the expected cap [2^cap_height][4].  constants and sigmas are adjacent.
    Section arity, constants, sigmas, k_is, row_idx, pi_pos, tape, seg_lens, cap;
};

inline int32_t art_refuse(ArtRefusal r, char msg[ART_MSG_LEN]) {
    snprintf(msg, ART_MSG_LEN, "%s: %s", ART_WHO, ART_REFUSALS[r].text);
    return ART_REFUSALS[r].code;
}

// GL355_OK and the view, or GL355_E_INVALID_ARG / GL355_E_UNSUPPORTED and "circuit_load: ..." in msg.  Needs no device.
inline int32_t artifact_parse(const uint64_t* blob, uint64_t words, ArtifactView& v, char msg[ART_MSG_LEN]) {
    constexpr uint64_t U32 = 0xFFFFFFFFull;
    msg[0] = 0;
    if (!blob || words < ART_HDR_WORDS) return art_refuse(ART_R_TRUNCATED, msg);
    const uint64_t version = blob[ART_VERSION];
    if (blob[ART_MAGIC] != ART_MAGIC_VALUE || version < ART_VERSION_MIN || version > ART_VERSION_MAX) return art_refuse(ART_R_VERSION, msg);
    memset(&v, 0, sizeof v);
    v.version = (uint32_t)version; v.external_digest = art_external_digest(version); v.arity_table = art_arity_table(version);
    // ---- the circuit scalars and the gate table
    const uint64_t degree_bits = blob[ART_DEGREE_BITS], rate_bits = blob[ART_RATE_BITS], num_wires = blob[ART_NUM_WIRES], routed = blob[ART_NUM_ROUTED_WIRES];
    const uint64_t num_constants = blob[ART_NUM_CONSTANTS], num_selectors = blob[ART_NUM_SELECTORS], num_challenges = blob[ART_NUM_CHALLENGES];
    const uint64_t max_degree = blob[ART_MAX_DEGREE], num_partial_products = blob[ART_NUM_PARTIAL_PRODUCTS], num_gates = blob[ART_NUM_GATES];
    for (uint32_t i = ART_DEGREE_BITS; i <= ART_NUM_GATES; i++)
        if (blob[i] > U32) return art_refuse(ART_R_SHAPE, msg);
    if (num_gates > GL355_MAX_GATES || degree_bits == 0 || degree_bits > 24 || num_wires == 0 || num_wires > 1024 || routed > num_wires ||
        num_selectors + num_constants > 64)
        return art_refuse(ART_R_SHAPE, msg);
    gl355_circuit& c = v.c;
    c.degree_bits = (uint32_t)degree_bits; c.rate_bits = (uint32_t)rate_bits; c.num_wires = (uint32_t)num_wires; c.num_routed_wires = (uint32_t)routed;
    c.num_constants = (uint32_t)num_constants; c.num_selectors = (uint32_t)num_selectors; c.num_challenges = (uint32_t)num_challenges;
    c.max_degree = (uint32_t)max_degree; c.num_partial_products = (uint32_t)num_partial_products; c.num_gates = (uint32_t)num_gates;
    for (uint32_t g = 0; g < c.num_gates; g++) {
        const uint64_t* p = blob + ART_GATES + ART_GATE_WORDS * g;
        // the parameter gate_table_check sees is the one the artifact states, not its low 32 bits
        if (p[ART_GATE_PARAM] > U32) return art_refuse(ART_R_GATE_PARAM, msg);
        if (p[ART_GATE_TYPE] > U32 || p[ART_GATE_SELECTOR] > U32 || p[ART_GATE_GROUP_START] > U32 || p[ART_GATE_GROUP_END] > U32) return art_refuse(ART_R_GATE_WORD, msg);
        c.gates[g].type = (uint32_t)p[ART_GATE_TYPE]; c.gates[g].param = (uint32_t)p[ART_GATE_PARAM]; c.gates[g].selector_index = (uint32_t)p[ART_GATE_SELECTOR];
        c.gates[g].group_start = (uint32_t)p[ART_GATE_GROUP_START]; c.gates[g].group_end = (uint32_t)p[ART_GATE_GROUP_END];
    }
    // every gate's type, selector group, wires and constants (gate_shape.h): the provers' kernels read the descriptor unchecked
    if (gate_table_check(c, ART_WHO, msg) != GL355_OK) return GL355_E_INVALID_ARG;
    // ---- sizes, and the length they add up to
    const uint64_t n = 1ull << degree_bits, n_sc = num_selectors + num_constants;
    const uint64_t n_rows = blob[ART_N_ROWS], n_ops = blob[ART_N_OPS], n_inputs = blob[ART_N_INPUTS], n_pi = blob[ART_N_PI];
    if (n_rows > n || n_ops > (1ull << 28) || n_pi > (1u << 20)) return art_refuse(ART_R_SIZES, msg);
    const uint64_t n_seq = blob[ART_N_SEQ], n_segs = blob[ART_N_SEGS];
    if (n_seq > n_ops || n_segs > n_ops) return art_refuse(ART_R_SEGMENTATION, msg);
    const uint64_t cap_height = blob[ART_CAP_HEIGHT], n_layers = blob[ART_N_FRI_LAYERS];
    if (cap_height > 20) return art_refuse(ART_R_CAP_HEIGHT, msg);
    if (n_layers > ART_MAX_FRI_LAYERS) return art_refuse(ART_R_FRI_LAYERS, msg);
    ArtifactView::Section* const sections[] = {&v.arity, &v.constants, &v.sigmas, &v.k_is, &v.row_idx, &v.pi_pos, &v.tape, &v.seg_lens, &v.cap};
    const uint64_t lengths[] = {v.arity_table ? n_layers : 0, n_sc * n, routed * n, routed, n_rows, n_pi, 5 * n_ops, n_segs,
                                v.external_digest ? 4ull << cap_height : 0};      // at most 2^34 words each
    uint64_t need = ART_HDR_WORDS;
    for (uint64_t len : lengths) need += len;
    if (words != need) return art_refuse(ART_R_LENGTH, msg);
    const uint64_t* p = blob + ART_HDR_WORDS;      // the length is right: every section lies inside the artifact
    for (int k = 0; k < 9; k++) { *sections[k] = {p, lengths[k]}; p += lengths[k]; }
    if (blob[ART_HASHER] != GL355_HASH_POSEIDON && blob[ART_HASHER] != GL355_HASH_BN254_POSEIDON) return art_refuse(ART_R_HASHER, msg);
    // ---- the arity table: what FriLayers::init refuses is refused here, by name
    const uint64_t lde_bits = degree_bits + rate_bits;
    uint64_t sum = 0;
    for (uint64_t l = 0; l < n_layers; l++) {
        const uint64_t a = v.arity_table ? v.arity.p[l] : 1;
        v.fri_arity_bits[l] = (uint32_t)a;
        if (!v.arity_table) continue;
        if (a == 0 || a > U32) return art_refuse(ART_R_ARITY_WORD, msg);
        if (a > GL355_MAX_FRI_ARITY_BITS) return art_refuse(ART_R_ARITY_WIDE, msg);
        sum += a;
        if (sum > degree_bits) return art_refuse(ART_R_ARITY_SUM, msg);
        if (lde_bits - sum < cap_height) return art_refuse(ART_R_ARITY_CAP, msg);
    }
    // ---- the sections' contents
    for (uint64_t i = 0; i < n_rows; i++)
        if (v.row_idx.p[i] >= n) return art_refuse(ART_R_ROW_INDEX, msg);
    for (uint64_t i = 0; i < n_pi; i++)
        if (v.pi_pos.p[i] >= n_rows * num_wires) return art_refuse(ART_R_PI_POSITION, msg);
    uint64_t tot = n_seq;      // no entry may exceed what is left, so the running sum cannot wrap around to n_ops
    for (uint64_t k = 0; k < n_segs; k++) {
        if (v.seg_lens.p[k] > n_ops - tot) return art_refuse(ART_R_SEGMENTS, msg);
        tot += v.seg_lens.p[k];
    }
    if (tot != n_ops) return art_refuse(ART_R_SEGMENTS, msg);
    const uint64_t blind_start = blob[ART_BLIND_START], n_blind = blob[ART_N_BLIND], z_start = blob[ART_Z_START], n_z_pairs = blob[ART_N_Z_PAIRS];
    if (blind_start > n || n_blind > n - blind_start || z_start > n || n_z_pairs > (n - z_start) / 2) return art_refuse(ART_R_BLINDING, msg);
    // every offset of the tape is checked here, once: the replays (host and device) of a loaded circuit cannot leave the rows
    if (n_ops && tape_validate(v.tape.p, n_ops, n_inputs, n_rows * num_wires, c.num_wires) != ~0ull) return art_refuse(ART_R_TAPE, msg);
    // ---- what every use of a handle asks of the circuit (the comment at GL355_ART_REFUSALS)
    if (blob[ART_POW_BITS] > U32 || blob[ART_NUM_QUERIES] > U32 || blob[ART_ZERO_KNOWLEDGE] > U32) return art_refuse(ART_R_PARAM_WORD, msg);
    if (max_degree == 0) return art_refuse(ART_R_MAX_DEGREE, msg);
    if (num_challenges == 0 || num_challenges > 4) return art_refuse(ART_R_CHALLENGES, msg);
    if (num_partial_products + 1 != (routed + max_degree - 1) / max_degree) return art_refuse(ART_R_PARTIAL_PRODUCTS, msg);
    if (rate_bits > 4 || lde_bits > 28) return art_refuse(ART_R_SIZE, msg);
    if (cap_height > lde_bits) return art_refuse(ART_R_CAP_TOO_LARGE, msg);
    v.cap_height = (uint32_t)cap_height; v.pow_bits = (uint32_t)blob[ART_POW_BITS]; v.num_queries = (uint32_t)blob[ART_NUM_QUERIES];
    v.n_fri_layers = (uint32_t)n_layers; v.zero_knowledge = (int32_t)blob[ART_ZERO_KNOWLEDGE]; v.hasher = (int32_t)blob[ART_HASHER];
    v.blind_start = (uint32_t)blind_start; v.n_blind = (uint32_t)n_blind; v.z_start = (uint32_t)z_start; v.n_z_pairs = (uint32_t)n_z_pairs;
    v.n_rows = n_rows; v.n_ops = n_ops; v.n_inputs = n_inputs; v.n_pi = n_pi; v.n_seq = n_seq; v.n_segs = n_segs;
    v.digest = blob + ART_DIGEST;
    return GL355_OK;
}

}  // namespace gl355
