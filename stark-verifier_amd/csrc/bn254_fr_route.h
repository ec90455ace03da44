// The route of a BN254 Fr transform as data: how its log_n stages split into passes of fr_fft_pass_kernel, in which order the passes are launched
// and which buffer each one reads and writes.  Pure host code without a HIP include, so that tests/fr_route_check.cpp can build it alone under the
// host sanitizers, like ntt_route.h and merkle_update_plan.h.  fr_launch (bn254_fr_fft.hip) fills one FrPass per step and launches it.
#pragma once
#include <stdint.h>

namespace gl355 {

constexpr uint32_t FR_MAX_PASSES = 4;      // log_n <= 31: ten stages and at most three passes of seven

// Stages per pass: min(10, log_n) in the first (s0 = 0: contiguous 1024-element tiles), the rest in the fewest passes of at most seven stages -- a
// 1024-element tile then keeps at least 8 adjacent columns -- whose sizes differ by at most one, the larger ones first.  s0: the stages below a pass.
struct FrSplit {
    uint32_t n_passes = 0;
    uint32_t ns[FR_MAX_PASSES] = {0}, s0[FR_MAX_PASSES] = {0};
};
inline FrSplit fr_split(uint32_t log_n) {
    FrSplit sp;
    sp.ns[sp.n_passes++] = log_n < 10 ? log_n : 10;
    const uint32_t rem = log_n - sp.ns[0], more = (rem + 6) / 7;
    for (uint32_t k = 0; k < more && sp.n_passes < FR_MAX_PASSES; k++) sp.ns[sp.n_passes++] = rem / more + (k < rem % more ? 1 : 0);
    for (uint32_t k = 1; k < sp.n_passes; k++) sp.s0[k] = sp.s0[k - 1] + sp.ns[k - 1];
    return sp;
}

enum FrOrder : uint8_t {
    FR_GATHER,        // natural in, natural out: decimation in time, the first pass reads bit-reversed (fr_ntt_run, bn254_fr_ntt_mont)
    FR_DIF,           // natural in, bit-reversed out: decimation in frequency from the top stage down (bn254_fr_ntt_mont_coset_dif)
    FR_FROM_BITREV,   // bit-reversed in, natural out: decimation in time without the gather (bn254_fr_ntt_mont_from_bitrev)
};
enum FrBuf : uint8_t { FR_BUF_IN, FR_BUF_WORK, FR_BUF_OUT };   // the caller's input, n elements of scratch, the caller's output

struct FrStep {
    uint32_t s0 = 0, ns = 0;
    // first: the pass that reads the input (conversion, pre-multipliers, zero padding beyond n_in); last: the pass that finishes the transform (post-multipliers
    // or scale, conversion, truncation to n_out) -- the kernel reads those fields of FrPass on that pass only
    bool first = false, last = false;
    FrBuf src = FR_BUF_IN, dst = FR_BUF_OUT;
};
struct FrRoute {
    uint32_t n_steps = 0;
    FrStep step[FR_MAX_PASSES];      // in launch order
    bool no_gather = false, dif = false;   // FrPass::no_gather, FrPass::dif of every pass
    bool tail_copy = false;          // n_out elements from WORK to OUT after the last pass
};

// in_place: the caller's input and output are the same array
inline FrRoute fr_route(FrOrder order, uint32_t log_n, bool in_place) {
    const FrSplit sp = fr_split(log_n);
    FrRoute r;
    r.n_steps = sp.n_passes;
    r.no_gather = order != FR_GATHER;
    r.dif = order == FR_DIF;
    for (uint32_t i = 0; i < r.n_steps; i++) {
        // dif runs from the highest s0 down; its last pass is the s0 = 0 one
        const uint32_t k = r.dif ? r.n_steps - 1 - i : i;
        FrStep& st = r.step[i];
        st.s0 = sp.s0[k]; st.ns = sp.ns[k];
        st.first = i == 0; st.last = i + 1 == r.n_steps;
        if (order == FR_GATHER) {
            // a pass reads and writes the same positions of its tile, the gathering one excepted: it cannot run in place, so the passes go through WORK, and
            // the last one may write straight to OUT unless it is the gathering one of an in-place transform
            st.src = st.first ? FR_BUF_IN : FR_BUF_WORK;
            st.dst = st.last && !(st.first && in_place) ? FR_BUF_OUT : FR_BUF_WORK;
        } else {
            // no pass gathers: the first goes IN -> OUT (IN may be OUT), the others run in place on OUT
            st.src = st.first ? FR_BUF_IN : FR_BUF_OUT;
            st.dst = FR_BUF_OUT;
        }
    }
    r.tail_copy = r.step[r.n_steps - 1].dst == FR_BUF_WORK;
    return r;
}

}  // namespace gl355
