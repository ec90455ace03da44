// The 24-bit-limb LDE passes (csrc/ntt_l24.cuh): launchers and the two table builders.  Compiled with the 15-instruction inline-asm field
// product like ntt_r8.hip (the coset-ratio products of the column pass and the 128-bit reductions of the limb products use it).
// a2 / a3 of SURVEY.md 8; reference call sites as in ntt.hip (plonky2 coset_fft_with_options inside CircuitData::prove, access_set.rs:94).
#define GL_MUL_VARIANT 1
#include "gl355_internal.h"
#include "ntt_l24.cuh"
#include <algorithm>

namespace gl355 {

// mid[64 u + v] = omega_4096^(bitrev6(u) v): cell (u, v) of the row tile holds output kA = bitrev6(u) of the first radix-64
// super-round (ntt_rows_l24s_kernel)
__global__ void build_mid_kernel(uint64_t root4096, uint64_t* out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 4096) return;
    const uint32_t u = g >> 6, v = g & 63;
    out[g] = gl_canon(gl_pow(root4096, (uint64_t)(__brev(u) >> 26) * v));
}

int32_t Ctx::l24_mid_table(const uint64_t** out) {
    return cached_table({3, 12}, 4096, out,
                        [&](uint64_t* d) { hipLaunchKernelGGL(build_mid_kernel, dim3(16), dim3(256), 0, stream, gl_root_of_unity(12), d); });
}

hipError_t launch_step_l24(const NttStep& st, const PassArgs& a, hipStream_t s) {
    switch (st.form) {
        // rows of 4096 points: a.batch << a.log_rows of them (forward, natural order in, bit-reversed canonical out, no multiplier tables).
        // The split-exchange kernel, one row per block, 33 KB of LDS.  (Its other launch shapes and the prefetching instantiation are timed in
        // profiles/r03_ubench_ntt_l24s.txt and r05_ubench_ntt_l24s.txt; the kernels it was measured against are in tools/ubench/ntt_l24_experiments.cuh.)
        case NTT_ROWS_L24: return launch_pass(ntt_rows_l24s_kernel<5, false>, st, 512, L24S_ROWS_LDS_BYTES, a, s);
        // 32-point column pass over all cosets: blocks over (column, 64-column tile).  Ratio table held in registers (116 VGPRs, 4 tiles per CU): no
        // load follows a store inside the coset loop (MODE 1 of the kernel; the variants that re-read it per coset or take one coset per block
        // measured slower: profiles/r03_ubench_ntt_l24s.txt (4))
        case NTT_COLS_L24_COSETS: return launch_pass(ntt_cols_l24s_cosets_kernel<6, 4, 1>, st, 256, 32 * 64 * 8, a, s);
        // column dimension 2, 4 or 8 (log_rows == 12): the streaming kernel, blocks over (256 columns, batch)
        case NTT_COLS_SMALL_COSETS:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_cols_small_cosets_kernel<LOG_T>, st, 256, 0, a, s);
            GL355_NTT_COLS_SMALL_COSETS_INSTANCES(GL355_X)
#undef GL355_X
            break;
        default: break;
    }
    return hipErrorInvalidValue;     // not reached: ntt_route lets no step through whose instance is not listed
}

}  // namespace gl355
