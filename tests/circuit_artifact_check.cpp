// Stand-alone check of the circuit artifact's host statement (csrc/circuit_artifact.h) for tests/test_circuit_artifact_host.py, built under
// AddressSanitizer and UBSan with csrc/witness_tape.cpp and the two host units it calls into.
//   circuit_artifact_check names         the table of header words, one `name index` line each
//   circuit_artifact_check messages      what artifact_parse can say, one `code text` line each (gate_table_check's four are not listed)
//   circuit_artifact_check BASE          BASE: a file of little-endian u64 words, read into a heap block of exactly its length.  One case
//                                        per line of stdin, a list of edits of the base: `s i v` sets word i to v, `t n` truncates to n
//                                        words, `a v` appends a word (i and n decimal, v hex); an empty line is the base itself
// Every case is parsed from a heap block of exactly its length, so a read outside the artifact is a sanitizer report, which aborts the run.
// A refused case answers `refused <code> <message>`.  An accepted one answers its whole view,
//   ok version external_digest arity_table | the ten circuit scalars | num_gates x type/param/selector/start/end | cap_height pow_bits num_queries
//   n_fri_layers zero_knowledge hasher | the arity bits | blind_start n_blind z_start n_z_pairs | n_rows n_ops n_inputs n_pi n_seq n_segs |
//   the four digest words | offset:words of arity, constants, sigmas, k_is, row_idx, pi positions, tape, segment lengths, cap
// after every word of every section has been read through the view's pointers.
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "circuit_artifact.h"

using namespace gl355;

namespace {

void answer(const uint64_t* blob, uint64_t words) {
    ArtifactView v;
    char msg[ART_MSG_LEN];
    const int32_t rc = artifact_parse(blob, words, v, msg);
    if (rc != GL355_OK) { printf("refused %d %s\n", rc, msg); return; }
    const gl355_circuit& c = v.c;
    printf("ok %u %d %d | %u %u %u %u %u %u %u %u %u %u |", v.version, (int)v.external_digest, (int)v.arity_table, c.degree_bits, c.rate_bits, c.num_wires,
           c.num_routed_wires, c.num_constants, c.num_selectors, c.num_challenges, c.max_degree, c.num_partial_products, c.num_gates);
    for (uint32_t g = 0; g < c.num_gates; g++)
        printf(" %u/%u/%u/%u/%u", c.gates[g].type, c.gates[g].param, c.gates[g].selector_index, c.gates[g].group_start, c.gates[g].group_end);
    printf(" | %u %u %u %u %d %d |", v.cap_height, v.pow_bits, v.num_queries, v.n_fri_layers, v.zero_knowledge, v.hasher);
    for (uint32_t l = 0; l < v.n_fri_layers; l++) printf(" %u", v.fri_arity_bits[l]);
    printf(" | %u %u %u %u | %llu %llu %llu %llu %llu %llu |", v.blind_start, v.n_blind, v.z_start, v.n_z_pairs, (unsigned long long)v.n_rows,
           (unsigned long long)v.n_ops, (unsigned long long)v.n_inputs, (unsigned long long)v.n_pi, (unsigned long long)v.n_seq, (unsigned long long)v.n_segs);
    for (int i = 0; i < 4; i++) printf(" %llx", (unsigned long long)v.digest[i]);
    printf(" |");
    uint64_t sink = 0;
    for (const ArtifactView::Section* s : {&v.arity, &v.constants, &v.sigmas, &v.k_is, &v.row_idx, &v.pi_pos, &v.tape, &v.seg_lens, &v.cap}) {
        printf(" %llu:%llu", (unsigned long long)(s->p - blob), (unsigned long long)s->words);
        for (uint64_t i = 0; i < s->words; i++) sink ^= s->p[i];
    }
    printf("%s\n", sink == 0x355 ? " " : "");      // the reads above are kept
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: circuit_artifact_check names | messages | BASE\n"); return 2; }
    const std::string what = argv[1];
    if (what == "names") {
        for (const ArtName& n : ART_NAMES) printf("%s %u\n", n.name, n.at);
        return 0;
    }
    if (what == "messages") {
        for (const ArtRefusalText& r : ART_REFUSALS) printf("%d %s: %s\n", r.code, ART_WHO, r.text);
        return 0;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "FAILED: cannot open %s\n", argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const uint64_t n_base = (uint64_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    uint64_t* base = (uint64_t*)malloc(n_base * 8 + !n_base);      // exactly the artifact
    if (fread(base, 8, n_base, f) != n_base) { fprintf(stderr, "FAILED: cannot read %s\n", argv[1]); return 1; }
    fclose(f);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        struct Set { uint64_t at, value; };
        std::vector<Set> sets;
        std::vector<uint64_t> appended;
        uint64_t n = n_base;
        bool resized = false;
        for (std::string op; in >> op;) {
            uint64_t i = 0, val = 0;
            if (op == "s" && (in >> std::dec >> i >> std::hex >> val)) sets.push_back({i, val});
            else if (op == "t" && (in >> std::dec >> i) && i <= n_base) { n = i; resized = true; }
            else if (op == "a" && (in >> std::hex >> val)) { appended.push_back(val); resized = true; }
            else { fprintf(stderr, "FAILED: cannot read '%.60s'\n", line.c_str()); return 1; }
        }
        const uint64_t words = n + appended.size();
        for (const Set& s : sets)
            if (s.at >= words) { fprintf(stderr, "FAILED: word %llu of %llu in '%.60s'\n", (unsigned long long)s.at, (unsigned long long)words, line.c_str()); return 1; }
        if (resized) {      // a block of its own, of exactly the new length
            uint64_t* blob = (uint64_t*)malloc(words * 8 + !words);
            memcpy(blob, base, n * 8);
            for (size_t k = 0; k < appended.size(); k++) blob[n + k] = appended[k];
            for (const Set& s : sets) blob[s.at] = s.value;
            answer(blob, words);
            free(blob);
        } else {            // in place, and put back
            std::vector<uint64_t> old;
            for (const Set& s : sets) { old.push_back(base[s.at]); base[s.at] = s.value; }
            answer(base, words);
            for (size_t k = sets.size(); k-- > 0;) base[sets[k].at] = old[k];
        }
    }
    free(base);
    return 0;
}
