// Stand-alone check of the Goldilocks NTT route table (csrc/ntt_route.h) for tests/test_ntt_route_host.py, built under AddressSanitizer and UBSan.
// The header is pure host code, so nothing else is linked.  One answer line per line of stdin:
//   log_n n_cosets inverse in_bitrev out_bitrev pre post scale ratio out_contig cosets_contig slot0_zero batch_fits_y single_pass_max_log
//       ->  step | step | ..      or      refused CODE MESSAGE
//   a step is  form<LT,LOG_T,PRE,INV,PASS>[tables;flags] rows=R xf=X shift=K src>dst scope*bytes grid=A,B
//     tables  root (the two-level 4-step tables are fetched here), pre:T step:T post:T with T = 1 | 2 | full | 1full | nat, ratio, mid, scale
//     flags   bitrev_in, natural_out, canon, collapse
//     grid    the blocks of the step at batch 1 and at batch 135 (x * y; 0,0: the step launches through bitrev_permute)
//   instances
//       ->  form<LT,LOG_T,PRE,INV,PASS> of every compiled instance, separated by blanks
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "ntt_route.h"

using namespace gl355;

static std::string instance_name(NttForm form, int lt, int log_t, int pre, int inv, int pass) {
    char buf[96];
    snprintf(buf, sizeof buf, "%s<%d,%d,%d,%d,%d>", NTT_FORM_NAME[form], lt, log_t, pre, inv, pass);
    return buf;
}

static void print_step(const NttShape& sh, const NttStep& st) {
    static const char* bufs[3] = {"in", "out", "mid"};
    std::string tabs, flags;
    const auto add = [](std::string& s, const std::string& w) { s += (s.empty() ? "" : ",") + w; };
    if (st.fetch_step_root) add(tabs, "root");
    if (st.pre_tab) add(tabs, std::string("pre:") + NTT_TAB_NAME[st.pre_tab]);
    if (st.step_tab) add(tabs, std::string("step:") + NTT_TAB_NAME[st.step_tab]);
    if (st.post_tab) add(tabs, std::string("post:") + NTT_TAB_NAME[st.post_tab]);
    if (st.ratio_tab) add(tabs, "ratio");
    if (st.mid_tab) add(tabs, "mid");
    if (st.scale) add(tabs, "scale");
    if (st.in_bitrev) add(flags, "bitrev_in");
    if (st.out_natural) add(flags, "natural_out");
    if (st.canon) add(flags, "canon");
    if (st.collapse_cosets) add(flags, "collapse");
    const uint32_t n_cosets = st.collapse_cosets ? 1 : sh.n_cosets;
    const NttGrid g1 = ntt_step_grid(st, 1ull << st.batch_shift, n_cosets), g135 = ntt_step_grid(st, 135ull << st.batch_shift, n_cosets);
    printf("%s[%s;%s] rows=%u xf=%u shift=%u %s>%s %s*%u grid=%llu,%llu", instance_name(st.form, st.lt, st.log_t, st.pre, st.inv, st.pass).c_str(),
           tabs.c_str(), flags.c_str(), st.log_rows, st.xform_log_n, st.batch_shift, bufs[st.src], bufs[st.dst], st.scope, st.bytes_per_point,
           (unsigned long long)(g1.x * g1.y), (unsigned long long)(g135.x * g135.y));
}

int main() {
    static char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "instances", 9)) {
            bool first = true;
            ntt_for_each_instance([&](NttForm form, int lt, int log_t, int pre, int inv, int pass) {
                printf("%s%s", first ? "" : " ", instance_name(form, lt, log_t, pre, inv, pass).c_str());
                first = false;
            });
            printf("\n");
            continue;
        }
        unsigned v[14];
        char* q = line;
        for (int k = 0; k < 14; k++) {
            char* end;
            v[k] = (unsigned)strtoul(q, &end, 10);
            if (end == q) { fprintf(stderr, "FAILED: cannot read '%s'\n", line); return 1; }
            q = end;
        }
        NttShape sh;
        sh.log_n = v[0]; sh.n_cosets = v[1];
        sh.inverse = v[2]; sh.in_bitrev = v[3]; sh.out_bitrev = v[4];
        sh.pre = v[5]; sh.post = v[6]; sh.scale = v[7]; sh.ratio = v[8];
        sh.out_contig = v[9]; sh.cosets_contig = v[10]; sh.slot0_zero = v[11]; sh.batch_fits_y = v[12];
        sh.single_pass_max_log = v[13];
        NttRoute r;
        const int32_t rc = ntt_route(sh, r);
        if (rc != GL355_OK) {
            if (r.n_steps) { fprintf(stderr, "FAILED: a refusal with steps\n"); return 1; }
            printf("refused %d %s\n", rc, r.msg);
            continue;
        }
        if (r.n_steps < 1 || r.n_steps > 4) { fprintf(stderr, "FAILED: %u steps\n", r.n_steps); return 1; }
        for (uint32_t i = 0; i < r.n_steps; i++) {
            if (i) printf(" | ");
            print_step(sh, r.step[i]);
        }
        printf("\n");
    }
    return 0;
}
