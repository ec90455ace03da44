// The j_* chains of gl355_bn254_g1_chain (GL355_BN_CHAIN_J, a test hook): j_add / j_madd / j_double of bn254_g1.cuh in a translation unit of
// their own -- a __noinline__ function is compiled once per unit, for all of its callers there, and the MSM / fixed-base kernels that call these
// came out with other register counts when this hook was one more caller in their unit.
#include "gl355_internal.h"
#include "bn254_hook.cuh"

namespace gl355 {

__global__ void bn254_j_chain_hook_kernel(const uint32_t* opnd, uint32_t n_opnd, const uint32_t* steps, uint32_t n_chains, uint32_t n_steps,
                                          uint32_t* trace) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chains) return;
    const uint32_t* st = steps + (uint64_t)c * n_steps;
    uint32_t* tr = trace + (uint64_t)c * n_steps * HK_REC;
    jac A = j_identity(), B = j_identity();
    for (uint32_t s = 0; s < n_steps; s++, tr += HK_REC) {
        const uint32_t kind = st[s] >> 28, k = st[s] & 0x0fffffffu;
        if (kind > GL355_BN_STEP_MADD || ((kind == GL355_BN_STEP_ADD || kind == GL355_BN_STEP_MADD) && k >= n_opnd)) { hk_rec_bad(tr); continue; }
        const uint32_t* o = opnd + (uint64_t)HK_OPND * (kind == GL355_BN_STEP_ADD || kind == GL355_BN_STEP_MADD ? k : 0);
        if (kind == GL355_BN_STEP_ADD) A = j_add(A, hk_jac(o));
        else if (kind == GL355_BN_STEP_DOUBLE) A = j_double(A);
        else if (kind == GL355_BN_STEP_ACC) B = j_add(B, A);
        else if (kind == GL355_BN_STEP_SELF) A = j_add(A, A);
        else A = j_madd(A, hk_u(o), hk_u(o + 9));
        hk_rec_jac(tr, kind == GL355_BN_STEP_ACC ? B : A, kind == GL355_BN_STEP_ACC ? 1 : 0);
    }
}
int32_t bn254_j_chain_hook(Ctx* ctx, const uint32_t* opnd, uint32_t n_opnd, const uint32_t* steps, uint32_t n_chains, uint32_t n_steps, uint32_t* trace) {
    hipLaunchKernelGGL(bn254_j_chain_hook_kernel, dim3((n_chains + 63) / 64), dim3(64), 0, ctx->stream, opnd, n_opnd, steps, n_chains, n_steps, trace);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

}  // namespace gl355
