// Stand-alone check of the host plan of an in-place Merkle update (csrc/merkle_update_plan.h) for tests/test_merkle_update_plan_host.py, built
// under AddressSanitizer and UBSan.  The header is pure host code, so nothing else is linked.  One answer line per line of stdin:
//   sub_bits cap_height lanes_log lanes16 full_log n_idx i_0 .. i_{n_idx-1}
//       ->  leaves=a,b,.. src=p,q,.. climb=L full=F fit=G |1:kernel:g,g,..|2:kernel:..
//   the sorted unique leaves, the position of each one's last occurrence, the climb layer, merkle_update_is_full for a tree of
//   2^(sub_bits + cap_height) leaves, merkle_update_grids_fit, then per layer 1 .. sub_bits the kernel merkle_update_kernel_of names and the
//   dirty node ids.  Every index is below 2^(sub_bits + cap_height), as the library checks before it plans.  The index array is a heap block of exactly
//   n_idx words: a read outside it is a sanitizer report, which aborts the run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "merkle_update_plan.h"

using namespace gl355;

static void print_list(const char* name, const uint64_t* v, uint64_t n) {
    printf("%s", name);
    for (uint64_t j = 0; j < n; j++) printf(j ? ",%llu" : "%llu", (unsigned long long)v[j]);
}

int main() {
    static char line[1 << 20];
    while (fgets(line, sizeof line, stdin)) {
        char* q = line;
        unsigned long long head[6];
        for (int k = 0; k < 6; k++) {
            char* end;
            head[k] = strtoull(q, &end, 10);
            if (end == q) { fprintf(stderr, "FAILED: cannot read '%s'\n", line); return 1; }
            q = end;
        }
        const uint32_t sub_bits = (uint32_t)head[0], cap_height = (uint32_t)head[1], lanes_log = (uint32_t)head[2], full_log = (uint32_t)head[4];
        const bool lanes16 = head[3] != 0;
        const uint64_t n_idx = head[5];
        uint64_t* idx = (uint64_t*)malloc(n_idx ? n_idx * 8 : 1);
        if (!idx) { fprintf(stderr, "FAILED: out of memory\n"); return 1; }
        for (uint64_t j = 0; j < n_idx; j++) {
            char* end;
            idx[j] = strtoull(q, &end, 10);
            if (end == q) { fprintf(stderr, "FAILED: %llu indices promised in '%s'\n", (unsigned long long)n_idx, line); return 1; }
            q = end;
        }
        MerkleUpdatePlan p;
        merkle_update_dedup(idx, n_idx, 1ull << (sub_bits + cap_height), p);
        free(idx);
        merkle_update_layers(sub_bits, 1ull << (sub_bits + cap_height), p);
        if (p.offset.size() != sub_bits + 2 || p.offset[sub_bits + 1] != p.nodes.size()) { fprintf(stderr, "FAILED: offsets do not cover the node list\n"); return 1; }
        print_list("leaves=", p.leaves.data(), p.leaves.size());
        print_list(" src=", p.src.data(), p.src.size());
        printf(" climb=%u full=%d fit=%d ", p.climb_layer, (int)merkle_update_is_full(p.leaves.size(), 1ull << (sub_bits + cap_height), full_log),
               (int)merkle_update_grids_fit(p));
        static const char* names[3] = {"level", "lanes", "climb"};
        for (uint32_t layer = 1; layer <= sub_bits; layer++) {
            printf("|%u:%s:", layer, names[merkle_update_kernel_of(p, layer, lanes_log, lanes16)]);
            print_list("", p.nodes.data() + p.offset[layer], p.count(layer));
        }
        printf("\n");
    }
    return 0;
}
