// The PLONK descriptor blob of include/gl355.h (stark-verifier_amd/halo2.py export_desc) parsed and range-checked on the host: what
// gl355_plonk_keygen (plonk_bn254.hip) and gl355_plonk_check_witness (plonk_check.hip) both start from.  Every program operand is checked
// here: the device evaluators trust their programs.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "host_fr.h"
#include "plonk_program.h"

namespace gl355 {

constexpr uint64_t PLK_MAGIC = 0x4B4C503535334C47ull;       // "GL355PLK"
constexpr uint32_t PLK_HDR = 24;

struct PlkLookup { std::vector<uint32_t> in_code, tab_code; };

struct PlkDesc {
    uint32_t k = 0, n_advice = 0, n_fixed = 0, n_instance = 0, n_perm = 0, n_lookups = 0, degree = 0, bf = 0, n_gate_polys = 0;
    uint64_t n = 0, usable = 0;
    Fr digest;
    std::vector<std::pair<uint32_t, uint32_t>> perm_cols;                 // (kind, index)
    std::vector<std::pair<int32_t, int32_t>> queries[3];                  // (column, rotation)
    std::vector<Fr> consts;
    std::vector<uint32_t> gate_code;
    std::vector<PlkLookup> lookups;
};

// nullptr, or what is wrong with the blob (a static string)
inline const char* plk_parse_desc(const uint64_t* desc, uint64_t words, PlkDesc& d) {
    if (!desc || words < PLK_HDR) return "null or truncated descriptor";
    if (desc[0] != PLK_MAGIC || desc[1] != 1) return "not a version-1 gl355 PLONK descriptor";
    d.k = (uint32_t)desc[2]; d.n_advice = (uint32_t)desc[3]; d.n_fixed = (uint32_t)desc[4]; d.n_instance = (uint32_t)desc[5];
    d.n_perm = (uint32_t)desc[6]; d.n_lookups = (uint32_t)desc[7]; d.degree = (uint32_t)desc[8]; d.bf = (uint32_t)desc[9];
    const uint64_t nq[3] = {desc[10], desc[11], desc[12]}, n_consts = desc[13], gate_len = desc[14];
    d.n_gate_polys = (uint32_t)desc[15];
    if (desc[2] < 3 || desc[2] > 24 || desc[3] > 256 || desc[4] > 256 || desc[5] > 16 || desc[6] > 256 || desc[7] > 64 || desc[8] < 3 || desc[8] > 10 || desc[9] < 3 ||
        desc[9] > 64 || nq[0] > 1024 || nq[1] > 1024 || nq[2] > 64 || n_consts > 4096 || gate_len > (1u << 20) || desc[15] > (1u << 20))
        return "implausible circuit shape";
    d.n = 1ull << d.k;
    if (d.n < d.bf + 3ull) return "fewer rows than the blinding needs";
    d.usable = d.n - (d.bf + 1);
    d.digest = Fr::from_words(desc + 16);
    const uint64_t* p = desc + PLK_HDR;
    const uint64_t* end = desc + words;
    auto need = [&](uint64_t w) { return (uint64_t)(end - p) >= w; };
    if (!need(d.n_perm)) return "truncated descriptor";
    const uint32_t kind_cols[3] = {d.n_advice, d.n_fixed, d.n_instance};
    for (uint32_t j = 0; j < d.n_perm; j++, p++) {
        const uint32_t kind = (uint32_t)(*p >> 32), idx = (uint32_t)*p;
        if (kind > 2 || idx >= kind_cols[kind]) return "bad permutation column";
        d.perm_cols.push_back({kind, idx});
    }
    for (int kd = 0; kd < 3; kd++) {
        if (!need(nq[kd])) return "truncated descriptor";
        for (uint64_t q = 0; q < nq[kd]; q++, p++) {
            const int32_t col = (int32_t)(*p >> 32), rot = (int32_t)(uint32_t)*p;
            if (col < 0 || (uint32_t)col >= kind_cols[kd] || rot < -(int32_t)d.bf - 1 || rot > (int32_t)d.bf + 1) return "bad query";
            d.queries[kd].push_back({col, rot});
        }
    }
    if (!need(4 * n_consts)) return "truncated descriptor";
    for (uint64_t c = 0; c < n_consts; c++, p += 4) d.consts.push_back(Fr::from_words(p));
    auto read_code = [&](uint64_t len, std::vector<uint32_t>& code) -> bool {
        if (!need(2 * len)) return false;
        code.assign(reinterpret_cast<const uint32_t*>(p), reinterpret_cast<const uint32_t*>(p) + 4 * len);
        p += 2 * len;
        for (uint64_t i = 0; i < len; i++) {                  // every operand in range: the evaluator trusts its program
            const uint32_t op = code[4 * i], dst = code[4 * i + 1];
            if (op > PLK_OP_MOV || dst >= PLK_MAX_REGS) return false;
            for (int o = 0; o < (op == PLK_OP_ADD || op == PLK_OP_SUB || op == PLK_OP_MUL ? 2 : 1); o++) {
                const uint32_t v = code[4 * i + 2 + o], kind = v >> 24, idx = v & 0xFFFFFFu;
                if (kind == PLK_K_REG ? idx >= PLK_MAX_REGS : (kind == PLK_K_CONST ? idx >= n_consts : (kind > PLK_K_INSTANCE || idx >= nq[kind - PLK_K_ADVICE]))) return false;
            }
        }
        return true;
    };
    if (!read_code(gate_len, d.gate_code)) return "bad gate program";
    for (uint32_t l = 0; l < d.n_lookups; l++) {
        if (!need(2)) return "truncated descriptor";
        const uint64_t li = p[0], lt = p[1];
        p += 2;
        PlkLookup lk;
        if (li > (1u << 16) || lt > (1u << 16) || !read_code(li, lk.in_code) || !read_code(lt, lk.tab_code)) return "bad lookup program";
        d.lookups.push_back(std::move(lk));
    }
    if (p != end) return "descriptor length does not match its header";
    return nullptr;
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
