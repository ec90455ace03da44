// The Halo2 witness tape (part 1 of the verifier circuit): the advice columns of a circuit recorded over AllChipConfig
// (chip/native_chip/all_chip.rs:22-30) as a straight-line program of CHIP-LEVEL entries, replayed per proof from the proof's words.  The
// recorder is stark-verifier_amd/halo2_goldilocks.py; the interpreters are halo2_synth.hip (device) and halo2_synth_host.cpp (host), which share
// everything in this header except the Poseidon rounds.
//
// An entry is 8 words:  w0 = op | level << 8,  w1 = first row,  w2..w7 = operands (CONST: the value's four words in w2..w5).
// An operand is one word: kind << 60 | aux << 48 | column << 40 | row (CELL, BIT, INV, INV_EXT) or kind << 60 | index (INPUT).
//   CELL   the four words of an advice cell an EARLIER LEVEL wrote
//   INPUT  inputs[index] (a proof word)
//   BIT    bit `aux` of the low word of a cell      (GoldilocksChip::to_bits' unassigned bits, goldilocks_chip.rs:317-332)
//   INV    the Goldilocks inverse of a cell, 0 for 0 (GoldilocksChip::is_zero's unassigned a_inv, goldilocks_chip.rs:285-292)
//   INV_EXT  component `aux` (0 or 1) of the inverse of y0 + y1 X in GF(p)[X] / (X^2 - 7), (0, 0) for (0, 0): y0 is the cell this word
//          names, y1 the CELL operand in the NEXT word.  Only the first operand of a VALUE entry may be one
//          (GoldilocksExtensionChip::div_extension's unassigned y_inv, goldilocks_extension_chip.rs:83-98)
// The advice columns are AllChipConfig's, in configure order: a b c q r | q_limbs[5] | r_limbs[4] | state[5].
//   CONST       assign_constant (arithmetic_chip.rs:236-253): a = the constant
//   VALUE       assign_value (:256-268): r = the operand (w2; an INV_EXT takes w3 as well), q = p - r, both in 16-bit limbs.  FAILS for r >= p.
//   MULADD      assign (:281-308): a b c from the operands' low words, a b + c = q p + r, limbs
//   MULADD_EXT  assign_ext (:310-349), two rows: (a0 + a1 X)(b0 + b1 X) + (c0 + c1 X) in GF(p)[X] / (X^2 - 7)
//   PACK        pack (:454-463), three mul_add_no_mod rows (:414-437): b = p^i, c = the sum so far, q = 0, r = c + a p^i
//   UNPACK      unpack (:466-486), eight rows: the four base-p digits as assign_value rows, then their inner product with p^i.
//               FAILS when the digits do not recompose the cell (they always do for digits this code derives; checked all the same)
//   PERMUTE     PoseidonBn254Chip::apply_permute (poseidon_bn254_chip.rs:203-233): the state before each of the 68 rounds on rows
//               row .. row + 67 and the result on row + 68, five state columns
//   ASSERT_EQ   assert_equal (:213-221) on two cells: writes nothing, FAILS when they differ (an invalid proof)
// A failing entry still writes its rows (gl355_plonk_check_witness then names the row); the smallest failing entry index and the
// number of failing entries are the status.  Entries are stored level-major: level = 1 + the largest level among the writers of its
// CELL / BIT / INV operands, so the entries of one level are independent and the tape order is a topological order.
// Level-major also means that a RUN of consecutive levels is one contiguous range of entries: the device replays a run of narrow levels
// without a PERMUTE in one launch (halo2_run_kernel, halo2_synth.hip), from that range and the run's slice of the level table.
#pragma once
#include <stdint.h>

#include <vector>

#include "gl_field.cuh"

namespace gl355 {

struct Ctx;

enum { H2_OP_CONST = 1, H2_OP_VALUE = 2, H2_OP_MULADD = 3, H2_OP_MULADD_EXT = 4, H2_OP_PACK = 5, H2_OP_UNPACK = 6, H2_OP_PERMUTE = 7, H2_OP_ASSERT_EQ = 8 };
enum { H2_K_NONE = 0, H2_K_CELL = 1, H2_K_INPUT = 2, H2_K_BIT = 3, H2_K_INV = 4, H2_K_INV_EXT = 5 };
enum { H2_ENTRY_WORDS = 8, H2_N_ADVICE = 19, H2_PERMUTE_ROWS = 69, H2_SPREAD_LANES = 8, H2_RUN_THREADS = 256, H2_RUN_MAX_DEFAULT = 256 };
enum { H2_COL_A = 0, H2_COL_B = 1, H2_COL_C = 2, H2_COL_Q = 3, H2_COL_R = 4, H2_COL_QL = 5, H2_COL_RL = 10, H2_COL_STATE = 14 };

typedef unsigned __int128 h2_u128;
struct h2_w4 { uint64_t w[4]; };

// the advice columns of one synthesis: [n_advice][n][4] plain integers
struct H2Cols {
    uint64_t* advice;
    uint64_t n;
    const uint64_t* inputs;
};

GL_HD uint32_t h2_kind(uint64_t o) { return (uint32_t)(o >> 60); }
GL_HD uint32_t h2_aux(uint64_t o) { return (uint32_t)(o >> 48) & 0xFF; }
GL_HD uint32_t h2_col(uint64_t o) { return (uint32_t)(o >> 40) & 0xFF; }
GL_HD uint64_t h2_row(uint64_t o) { return o & 0xFFFFFFFFFFull; }
GL_HD uint64_t* h2_cell(const H2Cols& c, uint32_t col, uint64_t row) { return c.advice + 4 * ((uint64_t)col * c.n + row); }

GL_HD void h2_store(const H2Cols& c, uint32_t col, uint64_t row, const h2_w4& v) {
    uint64_t* p = h2_cell(c, col, row);
    p[0] = v.w[0]; p[1] = v.w[1]; p[2] = v.w[2]; p[3] = v.w[3];
}
GL_HD void h2_store64(const H2Cols& c, uint32_t col, uint64_t row, uint64_t v) {
    uint64_t* p = h2_cell(c, col, row);
    p[0] = v; p[1] = 0; p[2] = 0; p[3] = 0;
}

// (w2 2^128 + w1 2^64 + w0) = q p + r with 0 <= r < p, by folding 2^64 = p + (2^32 - 1); q < 2^128 for w2 < 2^60
GL_HD void h2_divmod_p(uint64_t w2, uint64_t w1, uint64_t w0, h2_u128* q, uint64_t* r) {
    const h2_u128 H = ((h2_u128)w2 << 64) | w1;
    h2_u128 quo = H;
    h2_u128 t = H * GL_EPS + w0;                       // H < 2^68 here (callers), so this is below 2^101
    while (t >> 64) {
        const uint64_t hi = (uint64_t)(t >> 64);
        quo += hi;
        t = (h2_u128)hi * GL_EPS + (uint64_t)t;
    }
    uint64_t lo = (uint64_t)t;
    if (lo >= GL_P) { lo -= GL_P; quo += 1; }
    *q = quo;
    *r = lo;
}
GL_HD uint64_t h2_mulmod(uint64_t a, uint64_t b) {
    const h2_u128 t = (h2_u128)a * b;
    h2_u128 q; uint64_t r;
    h2_divmod_p(0, (uint64_t)(t >> 64), (uint64_t)t, &q, &r);
    return r;
}
GL_HD uint64_t h2_inverse(uint64_t a) {                // a^(p - 2), 0 for 0
    a = a >= GL_P ? a - GL_P : a;
    uint64_t r = 1, base = a;
    uint64_t e = GL_P - 2;
    for (int i = 0; i < 64; i++) {
        if (e & 1) r = h2_mulmod(r, base);
        base = h2_mulmod(base, base);
        e >>= 1;
    }
    return a ? r : 0;
}

GL_HD h2_w4 h2_operand(const H2Cols& c, uint64_t o) {
    h2_w4 v = {{0, 0, 0, 0}};
    const uint32_t kind = h2_kind(o);
    if (kind == H2_K_INPUT) { v.w[0] = c.inputs[h2_row(o)]; return v; }
    const uint64_t* p = h2_cell(c, h2_col(o), h2_row(o));
    if (kind == H2_K_CELL) { v.w[0] = p[0]; v.w[1] = p[1]; v.w[2] = p[2]; v.w[3] = p[3]; }
    else if (kind == H2_K_BIT) v.w[0] = (p[0] >> h2_aux(o)) & 1;
    else if (kind == H2_K_INV) v.w[0] = h2_inverse(p[0]);
    return v;
}

// INV_EXT: (y0 - y1 X) / (y0^2 - 7 y1^2); 7 is no square, so the norm is 0 only for (0, 0), whose "inverse" is then (0, 0)
GL_HD h2_w4 h2_inv_ext(const H2Cols& c, uint64_t o, uint64_t o1) {
    uint64_t y0 = h2_cell(c, h2_col(o), h2_row(o))[0], y1 = h2_cell(c, h2_col(o1), h2_row(o1))[0];
    y0 = y0 >= GL_P ? y0 - GL_P : y0;
    y1 = y1 >= GL_P ? y1 - GL_P : y1;
    const uint64_t s0 = h2_mulmod(y0, y0), s1 = h2_mulmod(h2_mulmod(y1, y1), 7);
    const uint64_t inv = h2_inverse(s0 >= s1 ? s0 - s1 : s0 + (GL_P - s1));
    h2_w4 v = {{0, 0, 0, 0}};
    v.w[0] = h2_aux(o) ? h2_mulmod(y1 ? GL_P - y1 : 0, inv) : h2_mulmod(y0, inv);
    return v;
}

// the q and r cells of a row with their 16-bit limbs (assign_q_and_r, arithmetic_chip.rs:511-534): five limbs of q, four of r
GL_HD void h2_store_q_r(const H2Cols& c, uint64_t row, const h2_w4& q, const h2_w4& r) {
    h2_store(c, H2_COL_Q, row, q);
    h2_store(c, H2_COL_R, row, r);
    for (int i = 0; i < 5; i++) {
        const int sh = 16 * i;
        const uint64_t limb = sh < 64 ? (q.w[0] >> sh) & 0xFFFF : (q.w[1] >> (sh - 64)) & 0xFFFF;
        h2_store64(c, H2_COL_QL + i, row, limb);
    }
    for (int i = 0; i < 4; i++) h2_store64(c, H2_COL_RL + i, row, (r.w[0] >> (16 * i)) & 0xFFFF);
}

GL_HD bool h2_below_p(const h2_w4& v) { return !(v.w[1] | v.w[2] | v.w[3]) && v.w[0] < GL_P; }

// BN254's r, for q = p - r (mod r) of a value that is not below p
#define H2_FR_MOD {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}

// assign_value: returns 1 when the value is not below p (the row is written all the same: q = p - r in the scalar field)
GL_HD int h2_value_row(const H2Cols& c, uint64_t row, const h2_w4& r) {
    const uint64_t mod[4] = H2_FR_MOD;
    h2_w4 q;
    h2_u128 br = (h2_u128)GL_P - r.w[0];
    q.w[0] = (uint64_t)br;
    uint64_t borrow = (uint64_t)(br >> 64) & 1;
    for (int i = 1; i < 4; i++) {
        br = (h2_u128)0 - r.w[i] - borrow;
        q.w[i] = (uint64_t)br;
        borrow = (uint64_t)(br >> 64) & 1;
    }
    if (borrow) {
        h2_u128 cy = 0;
        for (int i = 0; i < 4; i++) { cy += (h2_u128)q.w[i] + mod[i]; q.w[i] = (uint64_t)cy; cy >>= 64; }
    }
    h2_store_q_r(c, row, q, r);
    return h2_below_p(r) ? 0 : 1;
}

// one base-field row from a b + c (+ more, as (w2, w1, w0)): a b c q r and the limbs
GL_HD void h2_arith_row(const H2Cols& c, uint64_t row, uint64_t a, uint64_t b, uint64_t cc, uint64_t w2, uint64_t w1, uint64_t w0) {
    h2_u128 q; uint64_t r;
    h2_divmod_p(w2, w1, w0, &q, &r);
    const h2_w4 qv = {{(uint64_t)q, (uint64_t)(q >> 64), 0, 0}}, rv = {{r, 0, 0, 0}};
    h2_store_q_r(c, row, qv, rv);
    h2_store64(c, H2_COL_A, row, a);
    h2_store64(c, H2_COL_B, row, b);
    h2_store64(c, H2_COL_C, row, cc);
}
GL_HD void h2_add192(uint64_t (&t)[3], h2_u128 v) {
    h2_u128 s = (h2_u128)t[0] + (uint64_t)v;
    t[0] = (uint64_t)s;
    s = (s >> 64) + t[1] + (uint64_t)(v >> 64);
    t[1] = (uint64_t)s;
    t[2] += (uint64_t)(s >> 64);
}

// p^i, i < 4, as four words (the coefficients of pack / unpack)
GL_HD h2_w4 h2_p_pow(int i) {
    const h2_w4 t[4] = {{{1, 0, 0, 0}},
                        {{0xFFFFFFFF00000001ull, 0, 0, 0}},
                        {{0xFFFFFFFE00000001ull, 0xFFFFFFFE00000002ull, 0, 0}},
                        {{0xFFFFFFFD00000001ull, 0xFFFFFFF900000005ull, 0xFFFFFFFD00000005ull, 0}}};
    return t[i];
}
// mul_add_no_mod (arithmetic_chip.rs:414-437) with b = p^i: a (one word) p^i + acc modulo 2^256; the callers' sums stay below r
GL_HD h2_w4 h2_nomod_row(const H2Cols& c, uint64_t row, uint64_t a, int i, const h2_w4& acc) {
    const h2_w4 b = h2_p_pow(i);
    h2_w4 r;
    h2_u128 cy = 0;
    for (int j = 0; j < 4; j++) {
        cy += (h2_u128)a * b.w[j] + acc.w[j];
        r.w[j] = (uint64_t)cy;
        cy >>= 64;
    }
    const h2_w4 zero = {{0, 0, 0, 0}};
    h2_store64(c, H2_COL_A, row, a);
    h2_store(c, H2_COL_B, row, b);
    h2_store(c, H2_COL_C, row, acc);
    h2_store(c, H2_COL_Q, row, zero);
    h2_store(c, H2_COL_R, row, r);
    return r;
}

// every entry but PERMUTE.  -> 1 when the entry fails (its rows are written all the same)
GL_HD int h2_exec(const H2Cols& c, const uint64_t* e) {
    const uint32_t op = (uint32_t)e[0] & 0xFF;
    const uint64_t row = e[1];
    switch (op) {
    case H2_OP_CONST: {
        const h2_w4 v = {{e[2], e[3], e[4], e[5]}};
        h2_store(c, H2_COL_A, row, v);
        return 0;
    }
    case H2_OP_VALUE:
        return h2_value_row(c, row, h2_kind(e[2]) == H2_K_INV_EXT ? h2_inv_ext(c, e[2], e[3]) : h2_operand(c, e[2]));
    case H2_OP_MULADD: {
        const uint64_t a = h2_operand(c, e[2]).w[0], b = h2_operand(c, e[3]).w[0], cc = h2_operand(c, e[4]).w[0];
        const h2_u128 t = (h2_u128)a * b + cc;
        h2_arith_row(c, row, a, b, cc, 0, (uint64_t)(t >> 64), (uint64_t)t);
        return 0;
    }
    case H2_OP_MULADD_EXT: {
        uint64_t v[6];
        for (int i = 0; i < 6; i++) v[i] = h2_operand(c, e[2 + i]).w[0];
        const uint64_t a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3], c0 = v[4], c1 = v[5];
        uint64_t x[3] = {c0, 0, 0}, y[3] = {c1, 0, 0};
        h2_add192(x, (h2_u128)a0 * b0);
        const h2_u128 m = (h2_u128)a1 * b1;
        for (int i = 0; i < 7; i++) h2_add192(x, m);
        h2_add192(y, (h2_u128)a0 * b1);
        h2_add192(y, (h2_u128)a1 * b0);
        h2_arith_row(c, row, a0, b0, c0, x[2], x[1], x[0]);
        h2_arith_row(c, row + 1, a1, b1, c1, y[2], y[1], y[0]);
        return 0;
    }
    case H2_OP_PACK: {
        h2_w4 acc = {{0, 0, 0, 0}};
        for (int i = 0; i < 3; i++) acc = h2_nomod_row(c, row + i, h2_operand(c, e[2 + i]).w[0], i, acc);
        return 0;
    }
    case H2_OP_UNPACK: {
        const h2_w4 x = h2_operand(c, e[2]);
        uint64_t a[4] = {x.w[0], x.w[1], x.w[2], x.w[3]}, d[4];
        for (int k = 0; k < 4; k++) {                  // goldilocks_decompose (utils.rs:25-36): long division by p, four times
            uint64_t rem = 0;
            for (int i = 3; i >= 0; i--) {
                h2_u128 q;
                h2_divmod_p(0, rem, a[i], &q, &rem);   // rem < p, so the quotient is below 2^64
                a[i] = (uint64_t)q;
            }
            d[k] = rem;
        }
        for (int k = 0; k < 4; k++) {
            const h2_w4 dv = {{d[k], 0, 0, 0}};
            (void)h2_value_row(c, row + k, dv);        // a remainder is below p
        }
        h2_w4 acc = {{0, 0, 0, 0}};
        for (int k = 0; k < 4; k++) acc = h2_nomod_row(c, row + 4 + k, d[k], k, acc);
        return 0;                                      // four base-p digits recompose any scalar (r < p^4): UNPACK has no failing case

    }
    case H2_OP_ASSERT_EQ: {
        const h2_w4 x = h2_operand(c, e[2]), y = h2_operand(c, e[3]);
        int ne = 0;
        for (int j = 0; j < 4; j++) ne |= x.w[j] != y.w[j];
        return ne;
    }
    default:
        return 1;
    }
}

}  // namespace gl355

// a validated tape: the entries (host copy; device copy when loaded through a context) and the entry range of every level
struct gl355_halo2_tape {
    struct gl355::Ctx* ctx;
    uint32_t k, n_advice;
    uint64_t n_entries, n_inputs;
    std::vector<uint64_t> host;
    std::vector<uint64_t> level_start;      // [levels + 1] entry indices
    std::vector<uint32_t> level_permutes;   // [levels] PERMUTE entries of each level (device tapes: the kernel's form depends on it)
    uint64_t spread_max;                    // a level of at most this many entries with a PERMUTE among them runs the kernel's spread form
    uint64_t run_max;                       // a level of at most this many entries and no PERMUTE joins a run (halo2_run_kernel); 0: no runs
    std::vector<std::pair<uint32_t, uint32_t>> launches;      // device tapes: (first level, levels) of every launch of one synthesis, in order, planned
                                                              // at load (halo2_plan_launches); two or more levels: a run
    uint64_t* dev;
    uint64_t* dev_level_start;              // level_start on the device, uploaded once at load: a run reads its slice of it
};

namespace gl355 {
// -> nullptr, or what is wrong with the tape; fills level_start when given
const char* halo2_tape_validate(const uint64_t* tape, uint64_t n_words, uint64_t n_inputs, uint32_t k, uint32_t n_advice, std::vector<uint64_t>* level_start);
void halo2_replay_host(const uint64_t* tape, uint64_t n_entries, uint32_t k, const uint64_t* inputs, uint64_t* advice, uint64_t status[2]);
}  // namespace gl355
