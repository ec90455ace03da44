// Stand-alone check of the Halo2 descriptor's host statement (csrc/plonk_desc.h) for tests/test_plonk_desc_host.py, built under
// AddressSanitizer and UBSan with csrc/host_keccak.cpp only.  One answer line per line of stdin:
//   max_k words w_0 .. w_{words-1} [c_0 ..]      (max_k and words decimal, every w and c a hex u64)
// A refused descriptor answers `refused <the parser's message>`.  An accepted one answers
//   ok k a f i perm lookups degree bf polys n usable | kind_cols x3 pieces chunk sets | gate_emits in/tab .. | perm_query .. (or `none`) |
//   the gate program's value, each lookup's input/table value [| the pinned digest, when commitment words c follow the descriptor]
// The programs run through plk_run_program over ev[kind] = a heap array of exactly that kind's query count and a constant pool of
// exactly the pool's size, so a read outside either is a sanitizer report, which aborts the run.  Evaluations and folds are seeded:
// four splitmix64 words from the state 0x355 + (a << 32) + b, as a 256-bit integer mod r; ev[kind][q] = (kind, q), y = (7, 0), theta = (8, 0).
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "plonk_desc.h"

using namespace gl355;

namespace {

Fr seeded(uint64_t a, uint64_t b) {
    uint64_t s = 0x355 + (a << 32) + b, w[4];
    for (auto& o : w) {      // splitmix64
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        o = z ^ (z >> 31);
    }
    return Fr::from_words(w);
}

void print_fr(const Fr& v) {
    uint64_t w[4];
    v.to_words(w);
    printf("%016llx%016llx%016llx%016llx", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]);
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned max_k;
        uint64_t words;
        if (!(in >> std::dec >> max_k >> words)) { fprintf(stderr, "FAILED: cannot read '%.60s'\n", line.c_str()); return 1; }
        std::vector<uint64_t> all;
        for (uint64_t v; in >> std::hex >> v;) all.push_back(v);
        if (all.size() < words) { fprintf(stderr, "FAILED: fewer words than announced in '%.60s'\n", line.c_str()); return 1; }
        const std::vector<uint64_t> desc(all.begin(), all.begin() + words), commit(all.begin() + words, all.end());      // exact heap blocks
        PlkDesc parsed;
        if (const char* what = plk_parse_desc(desc.data(), words, max_k, parsed)) { printf("refused %s\n", what); continue; }
        PlkDesc d = parsed;
        d.consts = std::vector<Fr>(parsed.consts.begin(), parsed.consts.end());           // capacity = size: the pool and nothing behind it
        printf("ok %u %u %u %u %u %u %u %u %u %llu %llu |", d.k, d.n_advice, d.n_fixed, d.n_instance, d.n_perm, d.n_lookups, d.degree, d.bf, d.n_gate_polys,
               (unsigned long long)d.n, (unsigned long long)d.usable);
        printf(" %u %u %u %u %u %u | %u", d.kind_cols[0], d.kind_cols[1], d.kind_cols[2], d.n_pieces, d.chunk_len, d.n_sets, d.gate_emits);
        for (auto& lk : d.lookups) printf(" %u/%u", lk.in_emits, lk.tab_emits);
        printf(" |");
        std::vector<uint32_t> pq;
        if (!plk_perm_queries(d, pq)) printf(" none");
        else for (uint32_t q : pq) printf(" %u", q);
        std::vector<Fr> ev[3];
        for (int kd = 0; kd < 3; kd++) {
            ev[kd] = std::vector<Fr>(d.queries[kd].size());
            for (size_t q = 0; q < ev[kd].size(); q++) ev[kd][q] = seeded(kd, q);
        }
        const Fr y = seeded(7, 0), theta = seeded(8, 0);
        printf(" | ");
        print_fr(plk_run_program(d, d.gate_code, ev, y));
        for (auto& lk : d.lookups) {
            printf(" ");
            print_fr(plk_run_program(d, lk.in_code, ev, theta));
            printf("/");
            print_fr(plk_run_program(d, lk.tab_code, ev, theta));
        }
        if (!commit.empty()) {
            if (commit.size() != 8ull * (d.n_fixed + d.n_perm)) { fprintf(stderr, "FAILED: %zu commitment words for %u columns\n", commit.size(), d.n_fixed + d.n_perm); return 1; }
            printf(" | ");
            print_fr(plk_pinned_digest(desc.data(), words, commit.data(), commit.data() + 8ull * d.n_fixed, d));
        }
        printf("\n");
    }
    return 0;
}
