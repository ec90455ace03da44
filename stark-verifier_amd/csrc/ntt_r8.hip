// The radix-8 pass kernels of the commit path (csrc/ntt_kernels.cuh), compiled with the 15-instruction inline-asm field product:
// at 6-8 waves per SIMD its hazard wait states are hidden and the shorter instruction stream wins (ntt.hip keeps the
// compiler-scheduled product for the radix-16 kernels, which run at 3 waves per SIMD).  a2 / a3 of SURVEY.md 8; reference call
// sites as in ntt.hip (plonky2 fft_with_options / coset_fft_with_options inside CircuitData::prove, access_set.rs:94).
#define GL_MUL_VARIANT 1
#include "gl355_internal.h"
#include "ntt_kernels.cuh"

namespace gl355 {

// Threads, waves per SIMD and LDS of each form (the grid is ntt_step_grid's):
//   rows        8192-point tiles: two 1024-thread blocks per CU need <= 64 VGPRs (0.65 -> 0.53 ms for 8 units' 2^13 -> 2^16 LDEs, a couple of spilled
//               dwords included); 4096-point tiles: four 512-thread blocks per CU (0.79 -> 0.76 ms against three at 68 VGPRs); a 16384-point tile at
//               4 waves per SIMD needs an EMPTY CU (all its VGPRs and 136 KB of LDS): alone it is the fastest form, under a many-context load the
//               blocks wait for CUs to drain (rocprof: 6 ms resident for 0.4 ms of work; 8 waves per SIMD measured no better: HISTORY round 3)
//   big columns forward column passes over 2^9 / 2^10 points on 8192-element tiles: the first pass of a 2^21 / 2^22-point transform whose second pass
//               is 4096-point rows; two 1024-thread blocks per CU at <= 64 VGPRs
//   natural     tiles of 4096 elements while 8 adjacent columns fit (LOG_T <= 9), 8192 elements for LOG_T = 10: two 1024-thread blocks per CU
//   all cosets  blocks over (column, tile)
hipError_t launch_step_r8(const NttStep& st, const PassArgs& a, hipStream_t s) {
    switch (st.form) {
        case NTT_ROWS8:
#define GL355_X(LT, LOG_T, PRE, INV, PASS)         \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) \
        return launch_pass(ntt_rows_r8_kernel<LT, PRE, (LT <= 13 ? 8 : 4), INV>, st, LT >= 13 ? 1024 : 512, tile_lds_bytes(LT), a, s);
            GL355_NTT_ROWS8_INSTANCES(GL355_X)
#undef GL355_X
            break;
        case NTT_COLS8:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_cols_r8_kernel<LOG_T, PRE, 4>, st, 512, tile_lds_bytes(LT), a, s);
            GL355_NTT_COLS8_INSTANCES(GL355_X)
#undef GL355_X
            break;
        case NTT_COLS8_BIG:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_cols_r8_kernel<LOG_T, false, 8, false, LT>, st, 1024, tile_lds_bytes(LT), a, s);
            GL355_NTT_COLS8_BIG_INSTANCES(GL355_X)
#undef GL355_X
            break;
        case NTT_COLS8_COSETS:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_cols_r8_cosets_kernel<LOG_T, 4>, st, 512, tile_lds_bytes(LT), a, s);
            GL355_NTT_COLS8_COSETS_INSTANCES(GL355_X)
#undef GL355_X
            break;
        case NTT_COLS8_NAT:      // one more pad word every 256 elements (lds_phys_t<1>)
#define GL355_X(LT, LOG_T, PRE, INV, PASS)                \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) \
        return launch_pass(ntt_cols_r8_nat_kernel<LT, LOG_T, PASS, (LT == 12 ? 4 : 8)>, st, 1 << (LT - 3), tile_lds_bytes(LT) + (8u << (LT - 8)), a, s);
            GL355_NTT_COLS8_NAT_INSTANCES(GL355_X)
#undef GL355_X
            break;
        default: break;
    }
    return hipErrorInvalidValue;     // not reached: ntt_route lets no step through whose instance is not listed
}

}  // namespace gl355
