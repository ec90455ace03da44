// The Halo2 witness tape on the host (halo2_tape.h): validation at load, and the sequential replay -- the second formulation the device
// interpreter (halo2_synth.hip) is compared with, and what a caller without a device runs.  The Poseidon rows follow the definition
// (bn245_poseidon/native.rs:45-62: constants, x^5, dense 5x5 MDS), one row per round as PoseidonBn254Chip::apply_permute assigns them
// (chip/native_chip/poseidon_bn254_chip.rs:203-233).
#include "gl355_internal.h"
#include "halo2_tape.h"
#include "host_mont.h"

namespace gl355 {
void host_bn254_poseidon_round(Fr s[5], int rnd);      // host_bn254.cpp
namespace {

void permute_rows(const H2Cols& c, const uint64_t* e) {
    const uint64_t row = e[1];
    Fr s[5];
    for (int i = 0; i < 5; i++) s[i] = Fr::from_words(h2_operand(c, e[2 + i]).w);
    for (int rnd = 0; rnd <= 68; rnd++) {
        for (int i = 0; i < 5; i++) {
            h2_w4 v;
            s[i].to_words(v.w);
            h2_store(c, H2_COL_STATE + i, row + rnd, v);
        }
        if (rnd < 68) host_bn254_poseidon_round(s, rnd);
    }
}

// rows an entry writes: [first, first + count) of the columns in `mask` (bit = advice column)
struct Writes { uint64_t first, rows; uint32_t mask; };
const uint32_t MASK_ARITH = 0x3FFF, MASK_QR = 0x3FF8, MASK_ABCQR = 0x1F, MASK_STATE = 0x1Fu << H2_COL_STATE;

}  // namespace

const char* halo2_tape_validate(const uint64_t* tape, uint64_t n_words, uint64_t n_inputs, uint32_t k, uint32_t n_advice, std::vector<uint64_t>* level_start) {
    if (!tape && n_words) return "null tape";
    if (n_words % H2_ENTRY_WORDS) return "the tape is not a whole number of entries (truncated?)";
    if (k < 1 || k > 28) return "k out of range";
    if (n_advice != H2_N_ADVICE) return "the advice columns are not AllChipConfig's 19";
    const uint64_t n = 1ull << k, n_entries = n_words / H2_ENTRY_WORDS;
    // the level that wrote each cell of the columns an operand may name (a b c q r and the state), + 1; 0 = not written
    static const int slot_of[H2_N_ADVICE] = {0, 1, 2, 3, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, 5, 6, 7, 8, 9};
    std::vector<uint32_t> writer(10 * n, 0);
    if (level_start) level_start->clear();
    uint64_t prev_level = 0;
    for (uint64_t t = 0; t < n_entries; t++) {
        const uint64_t* e = tape + H2_ENTRY_WORDS * t;
        const uint32_t op = (uint32_t)e[0] & 0xFF;
        const uint64_t level = e[0] >> 8, row = e[1];
        if (level < 1 || level >= 0xFFFFFFFFull) return "an entry's level is out of range";
        if (level < prev_level) return "the entries are not stored level-major";
        if (level > prev_level + 1) return "a level is empty";
        if (level != prev_level && level_start) level_start->push_back(t);
        prev_level = level;
        int n_ops = 0;
        Writes w[2] = {{0, 0, 0}, {0, 0, 0}};
        uint64_t span = 1;
        switch (op) {
        case H2_OP_CONST: n_ops = 0; w[0] = {0, 1, 1u << H2_COL_A}; break;
        case H2_OP_VALUE: n_ops = h2_kind(e[2]) == H2_K_INV_EXT ? 2 : 1; w[0] = {0, 1, MASK_QR}; break;      // an INV_EXT's second cell is the next word
        case H2_OP_MULADD: n_ops = 3; w[0] = {0, 1, MASK_ARITH}; break;
        case H2_OP_MULADD_EXT: n_ops = 6; span = 2; w[0] = {0, 2, MASK_ARITH}; break;
        case H2_OP_PACK: n_ops = 3; span = 3; w[0] = {0, 3, MASK_ABCQR}; break;
        case H2_OP_UNPACK: n_ops = 1; span = 8; w[0] = {0, 4, MASK_QR}; w[1] = {4, 4, MASK_ABCQR}; break;      // four value rows (q r and limbs), four sum rows
        case H2_OP_PERMUTE: n_ops = 5; span = H2_PERMUTE_ROWS; w[0] = {0, H2_PERMUTE_ROWS, MASK_STATE}; break;
        case H2_OP_ASSERT_EQ: n_ops = 2; span = 0; break;
        default: return "unknown op";
        }
        if (row >= n || row + span > n) return "an entry's rows are out of range";
        for (int i = 0; i < n_ops; i++) {
            const uint64_t o = e[2 + i];
            const uint32_t kind = h2_kind(o);
            if (kind == H2_K_INPUT) {
                if ((op != H2_OP_VALUE || i) && op != H2_OP_MULADD && op != H2_OP_MULADD_EXT) return "an input operand where a cell is required";
                if (h2_row(o) >= n_inputs) return "an input index is out of range";
                continue;
            }
            if (kind != H2_K_CELL && kind != H2_K_BIT && kind != H2_K_INV && kind != H2_K_INV_EXT) return "unknown operand kind";
            if (kind == H2_K_INV_EXT) {
                if (op != H2_OP_VALUE || i != 0) return "an INV_EXT operand that is not the first of a VALUE entry";
                if (h2_aux(o) > 1) return "an INV_EXT component is out of range";
            } else if (op == H2_OP_VALUE && i == 1) {
                if (kind != H2_K_CELL) return "the second operand of an INV_EXT is not a cell";
            } else if (kind != H2_K_CELL && op != H2_OP_MULADD && op != H2_OP_MULADD_EXT) return "a derived operand outside a MULADD entry";
            if (kind == H2_K_BIT && h2_aux(o) >= 64) return "a bit index is out of range";
            const uint32_t col = h2_col(o);
            if (col >= H2_N_ADVICE || slot_of[col] < 0) return "an operand's column is out of range";
            if (h2_row(o) >= n) return "an operand's row is out of range";
            const uint32_t wl = writer[(uint64_t)slot_of[col] * n + h2_row(o)];
            if (!wl || wl - 1 >= level) return "an operand is not written by an earlier level (forward reference)";
        }
        for (const Writes& ww : w)
            for (uint32_t col = 0; col < H2_N_ADVICE; col++) {
                if (!((ww.mask >> col) & 1) || slot_of[col] < 0) continue;
                for (uint64_t r = row + ww.first; r < row + ww.first + ww.rows; r++) {
                    uint32_t& cell = writer[(uint64_t)slot_of[col] * n + r];
                    if (cell) return "two entries write the same cell";
                    cell = (uint32_t)level + 1;
                }
            }
    }
    if (level_start) level_start->push_back(n_entries);
    return nullptr;
}

void halo2_replay_host(const uint64_t* tape, uint64_t n_entries, uint32_t k, const uint64_t* inputs, uint64_t* advice, uint64_t status[2]) {
    const H2Cols c = {advice, 1ull << k, inputs};
    memset(advice, 0, (size_t)H2_N_ADVICE * c.n * 32);
    status[0] = ~0ull;
    status[1] = 0;
    for (uint64_t t = 0; t < n_entries; t++) {
        const uint64_t* e = tape + H2_ENTRY_WORDS * t;
        int fail = 0;
        if (((uint32_t)e[0] & 0xFF) == H2_OP_PERMUTE) permute_rows(c, e);
        else fail = h2_exec(c, e);
        if (fail) {
            if (status[0] == ~0ull) status[0] = t;
            status[1]++;
        }
    }
}

}  // namespace gl355

extern "C" int32_t gl355_halo2_synthesize_host(const uint64_t* tape, uint64_t n_words, uint64_t n_inputs, uint32_t k, uint32_t n_advice, const uint64_t* inputs,
                                               uint64_t* advice_out, uint64_t* status) {
    if (!advice_out || !status || (n_inputs && !inputs)) return GL355_E_INVALID_ARG;
    try {
        if (gl355::halo2_tape_validate(tape, n_words, n_inputs, k, n_advice, nullptr)) return GL355_E_INVALID_ARG;
    } catch (const std::bad_alloc&) {      // the validator's table of writers: 40 bytes a row
        return GL355_E_OOM;
    }
    gl355::halo2_replay_host(tape, n_words / gl355::H2_ENTRY_WORDS, k, inputs, advice_out, status);
    return GL355_OK;
}
