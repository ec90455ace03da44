// The PLONK descriptor blob of include/gl355.h (stark-verifier_amd/halo2.py export_desc) on the host, stated once: the parser and its range
// checks, the shape that follows from the header, the permutation columns' queries, the pinned-key digest rule and the host interpreter of
// the register programs.  The blob is untrusted input to three entry points:
//   gl355_plonk_keygen (plonk_bn254.hip)         parses with PLK_MAX_K_DEVICE; adds: fixed values / mapping present, plk_perm_queries, at most
//                                                four rotations per column, the mapping's range (on the device); digest by plk_pinned_digest
//   gl355_plonk_check_witness (plonk_check.hip)  parses with PLK_MAX_K_DEVICE; adds: gate_emits equals the header's polynomial count, every
//                                                lookup's in_emits equals its tab_emits and is not zero; it does not ask for plk_perm_queries
//   gl355_plonk_vk_create (plonk_verifier.cpp)   parses with PLK_MAX_K_VERIFIER; adds: commitments present, plk_perm_queries, every key point
//                                                and s_g2 valid; digest by plk_pinned_digest unless one is given
// Checked here, for all three: magic and version, every header bound, every permutation and query column and rotation, every operand of
// every instruction, and the blob's length.  The readers of a program -- plk_eval_kernel, chk_eval_kernel and plk_run_program below --
// trust it on the strength of that check.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "host_fr.h"
#include "plonk_program.h"

namespace gl355 {

constexpr uint64_t PLK_MAGIC = 0x4B4C503535334C47ull;       // "GL355PLK"
constexpr uint32_t PLK_HDR = 24;
constexpr uint32_t PLK_MAX_K_DEVICE = 24;                   // keygen and the witness check hold columns of 2^k rows on the device
constexpr uint32_t PLK_MAX_K_VERIFIER = 28;                 // the two-adicity of Fr: the verifier allocates nothing of size 2^k

struct PlkLookup {
    std::vector<uint32_t> in_code, tab_code;
    uint32_t in_emits = 0, tab_emits = 0;                                 // the EMITs of each program: the lookup's width
};

struct PlkDesc {
    uint32_t k = 0, n_advice = 0, n_fixed = 0, n_instance = 0, n_perm = 0, n_lookups = 0, degree = 0, bf = 0, n_gate_polys = 0;
    uint64_t n = 0, usable = 0;
    Fr digest;
    std::vector<std::pair<uint32_t, uint32_t>> perm_cols;                 // (kind, index)
    std::vector<std::pair<int32_t, int32_t>> queries[3];                  // (column, rotation)
    std::vector<Fr> consts;
    std::vector<uint32_t> gate_code;
    std::vector<PlkLookup> lookups;
    // what follows from the header
    uint32_t kind_cols[3] = {0, 0, 0};                                    // advice, fixed, instance
    uint32_t n_pieces = 0, chunk_len = 0, n_sets = 0;                     // quotient pieces; columns per permutation product, and how many products
    uint32_t gate_emits = 0;                                              // the EMITs of the gate program
};

// nullptr, or what is wrong with the blob (a static string).  max_k: the caller's largest k
inline const char* plk_parse_desc(const uint64_t* desc, uint64_t words, uint32_t max_k, PlkDesc& d) {
    if (!desc || words < PLK_HDR) return "null or truncated descriptor";
    if (desc[0] != PLK_MAGIC || desc[1] != 1) return "not a version-1 gl355 PLONK descriptor";
    d.k = (uint32_t)desc[2]; d.n_advice = (uint32_t)desc[3]; d.n_fixed = (uint32_t)desc[4]; d.n_instance = (uint32_t)desc[5];
    d.n_perm = (uint32_t)desc[6]; d.n_lookups = (uint32_t)desc[7]; d.degree = (uint32_t)desc[8]; d.bf = (uint32_t)desc[9];
    const uint64_t nq[3] = {desc[10], desc[11], desc[12]}, n_consts = desc[13], gate_len = desc[14];
    d.n_gate_polys = (uint32_t)desc[15];
    if (desc[2] < 3 || desc[2] > max_k || desc[3] > 256 || desc[4] > 256 || desc[5] > 16 || desc[6] > 256 || desc[7] > 64 || desc[8] < 3 || desc[8] > 10 || desc[9] < 3 ||
        desc[9] > 64 || nq[0] > 1024 || nq[1] > 1024 || nq[2] > 64 || n_consts > 4096 || gate_len > (1u << 20) || desc[15] > (1u << 20))
        return "implausible circuit shape";
    d.n = 1ull << d.k;
    if (d.n < d.bf + 3ull) return "fewer rows than the blinding needs";
    d.usable = d.n - (d.bf + 1);
    d.digest = Fr::from_words(desc + 16);
    d.kind_cols[0] = d.n_advice; d.kind_cols[1] = d.n_fixed; d.kind_cols[2] = d.n_instance;
    d.n_pieces = d.degree - 1;
    d.chunk_len = d.degree - 2;
    d.n_sets = (d.n_perm + d.chunk_len - 1) / d.chunk_len;
    const uint64_t* p = desc + PLK_HDR;
    const uint64_t* end = desc + words;
    auto need = [&](uint64_t w) { return (uint64_t)(end - p) >= w; };
    if (!need(d.n_perm)) return "truncated descriptor";
    for (uint32_t j = 0; j < d.n_perm; j++, p++) {
        const uint32_t kind = (uint32_t)(*p >> 32), idx = (uint32_t)*p;
        if (kind > 2 || idx >= d.kind_cols[kind]) return "bad permutation column";
        d.perm_cols.push_back({kind, idx});
    }
    for (int kd = 0; kd < 3; kd++) {
        if (!need(nq[kd])) return "truncated descriptor";
        for (uint64_t q = 0; q < nq[kd]; q++, p++) {
            const int32_t col = (int32_t)(*p >> 32), rot = (int32_t)(uint32_t)*p;
            if (col < 0 || (uint32_t)col >= d.kind_cols[kd] || rot < -(int32_t)d.bf - 1 || rot > (int32_t)d.bf + 1) return "bad query";
            d.queries[kd].push_back({col, rot});
        }
    }
    if (!need(4 * n_consts)) return "truncated descriptor";
    for (uint64_t c = 0; c < n_consts; c++, p += 4) d.consts.push_back(Fr::from_words(p));
    auto read_code = [&](uint64_t len, std::vector<uint32_t>& code, uint32_t& emits) -> bool {
        if (!need(2 * len)) return false;
        code.assign(reinterpret_cast<const uint32_t*>(p), reinterpret_cast<const uint32_t*>(p) + 4 * len);
        p += 2 * len;
        emits = 0;
        for (uint64_t i = 0; i < len; i++) {                // every operand in range: the evaluators trust their program
            const uint32_t op = code[4 * i], dst = code[4 * i + 1];
            if (op > PLK_OP_MOV || dst >= PLK_MAX_REGS) return false;
            emits += op == PLK_OP_EMIT;
            for (int o = 0; o < (op == PLK_OP_ADD || op == PLK_OP_SUB || op == PLK_OP_MUL ? 2 : 1); o++) {
                const uint32_t v = code[4 * i + 2 + o], kind = v >> 24, idx = v & 0xFFFFFFu;
                if (kind == PLK_K_REG ? idx >= PLK_MAX_REGS : (kind == PLK_K_CONST ? idx >= n_consts : (kind > PLK_K_INSTANCE || idx >= nq[kind - PLK_K_ADVICE]))) return false;
            }
        }
        return true;
    };
    if (!read_code(gate_len, d.gate_code, d.gate_emits)) return "bad gate program";
    for (uint32_t l = 0; l < d.n_lookups; l++) {
        if (!need(2)) return "truncated descriptor";
        const uint64_t li = p[0], lt = p[1];
        p += 2;
        PlkLookup lk;
        if (li > (1u << 16) || lt > (1u << 16) || !read_code(li, lk.in_code, lk.in_emits) || !read_code(lt, lk.tab_code, lk.tab_emits)) return "bad lookup program";
        d.lookups.push_back(std::move(lk));
    }
    if (p != end) return "descriptor length does not match its header";
    return nullptr;
}

// The permutation argument reads every equality column at x (halo2's enable_equality queries it at rotation 0): per permutation column
// the query of its kind that does so.  false: a column has none
inline bool plk_perm_queries(const PlkDesc& d, std::vector<uint32_t>& out) {
    out.clear();
    for (auto& pc : d.perm_cols) {
        uint32_t found = ~0u;
        const auto& qs = d.queries[pc.first];
        for (uint32_t q = 0; q < qs.size() && found == ~0u; q++) if (qs[q].first == (int32_t)pc.second && qs[q].second == 0) found = q;
        if (found == ~0u) return false;
        out.push_back(found);
    }
    return true;
}

// The transcript's initial scalar (halo2: vk.transcript_repr, a hash of the PINNED verifying key -- shape, fixed commitments, permutation
// commitments): a non-zero digest field is taken as given (a host that computed halo2's own transcript_repr); a zero one stands for
// Keccak-256 over (the whole descriptor | fixed commitments | sigma commitments, all as little-endian u64), read as a big-endian integer
// mod r, so two circuits that differ only in fixed values or copy constraints never share a Fiat-Shamir prefix and a C caller cannot
// forget the step.  fixed_c / sigma_c: [n_fixed][8] / [n_perm][8] words (may be null where there are none)
inline Fr plk_pinned_digest(const uint64_t* desc, uint64_t words, const uint64_t* fixed_c, const uint64_t* sigma_c, const PlkDesc& d) {
    if (desc[16] | desc[17] | desc[18] | desc[19]) return d.digest;
    std::vector<uint64_t> pre(desc, desc + words);
    if (d.n_fixed) pre.insert(pre.end(), fixed_c, fixed_c + 8ull * d.n_fixed);
    if (d.n_perm) pre.insert(pre.end(), sigma_c, sigma_c + 8ull * d.n_perm);
    uint8_t hsh[32];
    keccak256_host(reinterpret_cast<const uint8_t*>(pre.data()), pre.size() * 8, hsh);
    uint64_t w[4];
    KeccakTranscript::from_be32(hsh, w);
    return Fr::from_words(w);
}

// the descriptor's register programs (include/gl355.h) at one point: ev[kind][query] are the claimed evaluations
inline Fr plk_run_program(const PlkDesc& d, const std::vector<uint32_t>& code, const std::vector<Fr> ev[3], const Fr& fold) {
    Fr regs[PLK_MAX_REGS];
    for (auto& r : regs) r = Fr::zero();
    Fr acc = Fr::zero();
    auto operand = [&](uint32_t o) -> Fr {
        const uint32_t kind = o >> 24, idx = o & 0xFFFFFFu;
        if (kind == PLK_K_REG) return regs[idx];
        if (kind == PLK_K_CONST) return d.consts[idx];
        return ev[kind - PLK_K_ADVICE][idx];
    };
    for (size_t pc = 0; pc < code.size() / 4; pc++) {
        const uint32_t op = code[4 * pc], dst = code[4 * pc + 1];
        const Fr x = operand(code[4 * pc + 2]);
        if (op == PLK_OP_EMIT) { acc = acc * fold + x; continue; }
        if (op == PLK_OP_NEG) regs[dst] = x.neg();
        else if (op == PLK_OP_MOV) regs[dst] = x;
        else {
            const Fr y = operand(code[4 * pc + 3]);
            regs[dst] = op == PLK_OP_ADD ? x + y : (op == PLK_OP_SUB ? x - y : x * y);
        }
    }
    return acc;
}

// a lookup expression list that is one column at the current rotation (the reference's nine range checks, arithmetic_chip.rs:140-151):
// the "compressed" column is the column itself, no program run, no copy.  -> (kind, column) or kind = 3
inline std::pair<uint32_t, uint32_t> plk_single_query(const std::vector<std::pair<int32_t, int32_t>> queries[3], const std::vector<uint32_t>& code) {
    if (code.size() == 4 && code[0] == PLK_OP_EMIT) {
        const uint32_t kind = code[2] >> 24, idx = code[2] & 0xFFFFFFu;
        if (kind >= PLK_K_ADVICE && kind <= PLK_K_INSTANCE) {
            const auto& q = queries[kind - PLK_K_ADVICE][idx];
            if (q.second == 0) return {kind - PLK_K_ADVICE, (uint32_t)q.first};
        }
    }
    return {3u, 0u};
}

}  // namespace gl355
