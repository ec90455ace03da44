// Stand-alone check of the pass plan of the BN254 Fr transform (csrc/bn254_fr_route.h) for tests/test_fr_route_host.py, built under AddressSanitizer
// and UBSan.  The header is pure host code, so nothing else is linked.  One answer line per line of stdin:
//   order log_n in_place        order: 0 = GATHER, 1 = DIF, 2 = FROM_BITREV
//       ->  ns=A,B,.. s0=A,B,.. flags=F tail=T | step | step | ..
//   ns, s0   the split of fr_split, passes in ascending s0
//   flags    no_gather, dif of every pass (comma separated, may be empty)
//   tail     1: a copy from WORK to OUT follows the last pass
//   a step, in launch order, is  S0+NS:fl:src>dst  with f = first, l = last (- where not) and src, dst of in, work, out
#include <stdio.h>

#include "bn254_fr_route.h"

using namespace gl355;

int main() {
    static const char* bufs[3] = {"in", "work", "out"};
    unsigned order, log_n, in_place;
    while (scanf("%u %u %u", &order, &log_n, &in_place) == 3) {
        if (order > FR_FROM_BITREV) { fprintf(stderr, "FAILED: order %u\n", order); return 1; }
        const FrSplit sp = fr_split(log_n);
        const FrRoute r = fr_route((FrOrder)order, log_n, in_place != 0);
        if (sp.n_passes < 1 || sp.n_passes > FR_MAX_PASSES || r.n_steps != sp.n_passes) { fprintf(stderr, "FAILED: %u passes, %u steps\n", sp.n_passes, r.n_steps); return 1; }
        printf("ns=");
        for (uint32_t k = 0; k < sp.n_passes; k++) printf("%s%u", k ? "," : "", sp.ns[k]);
        printf(" s0=");
        for (uint32_t k = 0; k < sp.n_passes; k++) printf("%s%u", k ? "," : "", sp.s0[k]);
        printf(" flags=%s%s%s tail=%d", r.no_gather ? "no_gather" : "", r.no_gather && r.dif ? "," : "", r.dif ? "dif" : "", r.tail_copy ? 1 : 0);
        for (uint32_t i = 0; i < r.n_steps; i++) {
            const FrStep& st = r.step[i];
            printf(" | %u+%u:%c%c:%s>%s", st.s0, st.ns, st.first ? 'f' : '-', st.last ? 'l' : '-', bufs[st.src], bufs[st.dst]);
        }
        printf("\n");
    }
    return 0;
}
