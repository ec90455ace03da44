// Test hooks of the BN254 arithmetic (include/gl355.h "test hooks"; tests/test_gpu_bn254_arith.py): the shipped device functions of
// bn254_field.cuh / bn254_f29.cuh / bn254_g1.cuh / bn254_msm_acc.cuh on raw limbs, one lane per record or chain.  No product path calls them.
#include "bn254_msm_acc.cuh"
#include "bn254_hook.cuh"

namespace gl355 {
int32_t bn254_hash_fr_hook(Ctx* ctx, int32_t leave, const uint32_t* a, uint32_t* out, uint64_t n);      // merkle_bn254.hip
int32_t bn254_j_chain_hook(Ctx* ctx, const uint32_t* opnd, uint32_t n_opnd, const uint32_t* steps, uint32_t n_chains, uint32_t n_steps,
                           uint32_t* trace);                                                            // bn254_g1_hook.hip
template <int F> GL_DEV void hk_mont_op(int32_t op, const uint32_t* pa, const uint32_t* pb, uint32_t* po) {
    const u256 a = hk_u(pa);
    switch (op) {
    case GL355_BN_M_MUL: hk_put_u(po, m_mul<F>(a, hk_u(pb))); break;
    case GL355_BN_M_ADD: hk_put_u(po, m_add<F>(a, hk_u(pb))); break;
    case GL355_BN_M_SUB: hk_put_u(po, m_sub<F>(a, hk_u(pb))); break;
    case GL355_BN_M_CANON: hk_put_u(po, m_canon<F>(a)); break;
    case GL355_BN_M_FROM_INT: hk_put_u(po, m_from_int<F>(a)); break;
    case GL355_BN_M_TO_INT: hk_put_u(po, m_to_int<F>(a)); break;
    case GL355_BN_M_INV: hk_put_u(po, m_inv<F>(a)); break;
    case GL355_BN_M_IS_ZERO: hk_put_b(po, m_is_zero<F>(a)); break;
    default: hk_put_b(po, m_eq<F>(a, hk_u(pb))); break;
    }
}
__global__ void bn254_arith_hook_kernel(int32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* pa = a + 9 * i;
    const uint32_t* pb = b + 9 * i;
    uint32_t* po = out + 9 * i;
    if (op < GL355_BN_FQ) { hk_mont_op<F_R>(op, pa, pb, po); return; }
    if (op < GL355_BN_F29_MUL) { hk_mont_op<F_Q>(op - GL355_BN_FQ, pa, pb, po); return; }
    const f29 x = hk_f(pa);
    switch (op) {
    case GL355_BN_F29_MUL: hk_put_f(po, f29_mul(x, hk_f(pb))); break;
    case GL355_BN_F29_MUL_FR: hk_put_f(po, f29_mul_fr(x, hk_f(pb))); break;
    case GL355_BN_F29_ADD_NORM: hk_put_f(po, f29_norm(f29_add(x, hk_f(pb)))); break;
    case GL355_BN_F29_SUB_C2: hk_put_f(po, f29_sub(x, hk_f(pb), FQ29_C2)); break;
    case GL355_BN_F29_SUB_C4: hk_put_f(po, f29_sub(x, hk_f(pb), FQ29_C4)); break;
    case GL355_BN_F29_SUB_C8: hk_put_f(po, f29_sub(x, hk_f(pb), FQ29_C8)); break;
    case GL355_BN_F29_SUB_C16: hk_put_f(po, f29_sub(x, hk_f(pb), FQ29_C16)); break;
    case GL355_BN_F29_NEG_C2: hk_put_f(po, f29_neg(x, FQ29_C2)); break;
    case GL355_BN_F29_FROM_U256: hk_put_f(po, f29_from_u256(hk_u(pa))); break;
    case GL355_BN_F29_TO_U256: hk_put_u(po, f29_to_u256(x)); break;
    case GL355_BN_F29_LIFT: hk_put_f(po, f29_lift(hk_u(pa))); break;
    case GL355_BN_F29_LIFT_INL: hk_put_f(po, f29_lift_inl(hk_u(pa))); break;
    case GL355_BN_F29_LOWER: hk_put_u(po, f29_lower(x)); break;
    case GL355_BN_F29_IS_ZERO_MOD: hk_put_b(po, f29_is_zero_mod(x)); break;
    case GL355_BN_F29_TABLE_FORM: hk_put_u(po, msm_table_form(hk_u(pa))); break;
    default: hk_put_f(po, f29_norm(x)); break;
    }
}
// the point table of the bucket forms: msm_digits_kernel's conversion of each affine integer point (r_form: left in the R = 2^256 form, the table of msm_add_point)
__global__ void bn254_chain_table_kernel(const uint32_t* opnd, uint32_t n, uint32_t* pm, int32_t r_form) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* o = opnd + (uint64_t)HK_OPND * i;
    const u256 x = hk_u(o), y = hk_u(o + 9);
    const bool ident = u_is_zero(x) && u_is_zero(y);
    const u256 xr = m_from_int<F_Q>(x), yr = m_from_int<F_Q>(y);
    const u256 xm = ident ? u_zero() : (r_form ? xr : msm_table_form(xr)), ym = ident ? u_zero() : (r_form ? yr : msm_table_form(yr));
    uint32_t* d = pm + 16ull * i;
#pragma unroll
    for (int j = 0; j < 8; j++) { d[j] = xm.l[j]; d[8 + j] = ym.l[j]; }
}
GL_DEV void hk_rec_29(uint32_t* r, const jac29& p, uint32_t which) { hk_rec(r, p.x.l, p.y.l, p.z.l, nullptr, 9, p.ident, which); }
GL_DEV jac29 hk_jac29(const uint32_t* o, bool lift) {
    if (lift) return jac29_lift(hk_jac(o));
    jac29 p;
    p.x = hk_f(o); p.y = hk_f(o + 9); p.z = hk_f(o + 18); p.ident = o[27] != 0;
    return p;
}
__global__ void bn254_chain_hook_kernel(int32_t form, const uint32_t* opnd, uint32_t n_opnd, uint32_t* pm, const uint32_t* steps, uint32_t n_chains,
                                        uint32_t n_steps, uint32_t* trace) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chains) return;
    const uint32_t* st = steps + (uint64_t)c * n_steps;
    uint32_t* tr = trace + (uint64_t)c * n_steps * HK_REC;
    if (form == GL355_BN_CHAIN_JAC) {
        jac acc = j_identity();
        for (uint32_t s = 0; s < n_steps; s++, tr += HK_REC) {
            if ((st[s] & 0x7fffffffu) >= n_opnd) { hk_rec_bad(tr); continue; }
            acc = msm_add_point(pm, acc, st[s]);
            hk_rec_jac(tr, acc, 0);
        }
        return;
    }
    if (form == GL355_BN_CHAIN_XYZZ) {
        xyzz29 acc;
        acc.ident = true;
        for (uint32_t s = 0; s < n_steps; s++, tr += HK_REC) {
            if ((st[s] & 0x7fffffffu) >= n_opnd) { hk_rec_bad(tr); continue; }
            msm_add_point_xyzz(pm, acc, st[s]);
            hk_rec(tr, acc.x.l, acc.y.l, acc.zz.l, acc.zzz.l, 9, acc.ident, 0);
        }
        return;
    }
    if (form == GL355_BN_CHAIN_JAC29) {
        jac29 acc;
        acc.ident = true;
        for (uint32_t s = 0; s < n_steps; s++, tr += HK_REC) {
            if ((st[s] & 0x7fffffffu) >= n_opnd) { hk_rec_bad(tr); continue; }
            msm_add_point29(pm, acc, st[s]);
            hk_rec_29(tr, acc, 0);
        }
        return;
    }
    const bool lift = form == GL355_BN_CHAIN_RED29_LIFT;
    jac29 A, B;
    A.ident = B.ident = true;
    for (uint32_t s = 0; s < n_steps; s++, tr += HK_REC) {
        const uint32_t kind = st[s] >> 28, k = st[s] & 0x0fffffffu;
        if (kind > GL355_BN_STEP_SELF || (kind == GL355_BN_STEP_ADD && k >= n_opnd)) { hk_rec_bad(tr); continue; }
        if (kind == GL355_BN_STEP_ADD) jac29_add(A, hk_jac29(opnd + (uint64_t)HK_OPND * k, lift));
        else if (kind == GL355_BN_STEP_DOUBLE) jac29_double(A);
        else if (kind == GL355_BN_STEP_ACC) jac29_add(B, A);
        else { const jac29 t = A; jac29_add(A, t); }
        hk_rec_29(tr, kind == GL355_BN_STEP_ACC ? B : A, kind == GL355_BN_STEP_ACC ? 1 : 0);
    }
}
}  // namespace gl355

using namespace gl355;

extern "C" {
int32_t gl355_bn254_arith_batch(gl355_ctx* h, int32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    const bool two = op == GL355_BN_M_MUL || op == GL355_BN_M_ADD || op == GL355_BN_M_SUB || op == GL355_BN_M_EQ ||
                     op == (GL355_BN_FQ | GL355_BN_M_MUL) || op == (GL355_BN_FQ | GL355_BN_M_ADD) || op == (GL355_BN_FQ | GL355_BN_M_SUB) ||
                     op == (GL355_BN_FQ | GL355_BN_M_EQ) || (op >= GL355_BN_F29_MUL && op <= GL355_BN_F29_SUB_C16);
    const bool known = (op >= 0 && op <= GL355_BN_M_EQ) || (op >= GL355_BN_FQ && op <= (GL355_BN_FQ | GL355_BN_M_EQ)) ||
                       (op >= GL355_BN_F29_MUL && op <= GL355_BN_HASH_FR_LEAVE);
    if (!known) return ctx->fail(GL355_E_INVALID_ARG, "bn254_arith_batch: bad op");
    if (!a || !out || (two && !b)) return ctx->fail(GL355_E_INVALID_ARG, "bn254_arith_batch: null argument");
    if (n == 0) return GL355_OK;
    Staged sa(ctx), sb(ctx), so(ctx);
    GL355_TRY(sa.open(a, n * 36, 1));
    GL355_TRY(sb.open(two ? b : a, n * 36, 1));
    GL355_TRY(so.open(out, n * 36, 2));
    if (op >= GL355_BN_HASH_FR_ENTER) {
        GL355_TRY(bn254_hash_fr_hook(ctx, op == GL355_BN_HASH_FR_LEAVE, sa.as<uint32_t>(), so.as<uint32_t>(), n));
    } else {
        hipLaunchKernelGGL(bn254_arith_hook_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, sa.as<const uint32_t>(),
                           sb.as<const uint32_t>(), so.as<uint32_t>(), n);
        GL355_HIP(ctx, hipGetLastError());
    }
    return so.finish();
}
int32_t gl355_bn254_g1_chain(gl355_ctx* h, int32_t form, const uint32_t* operands, uint32_t n_operands, const uint32_t* steps, uint32_t n_chains,
                             uint32_t n_steps, uint32_t* trace) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (form < GL355_BN_CHAIN_XYZZ || form > GL355_BN_CHAIN_J) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_chain: bad form");
    if (!operands || !n_operands || !steps || !trace) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_chain: null argument");
    if ((uint64_t)n_chains * n_steps == 0) return GL355_OK;
    Staged so(ctx), ss(ctx), st(ctx);
    GL355_TRY(so.open(operands, (uint64_t)n_operands * HK_OPND * 4, 1));
    GL355_TRY(ss.open(steps, (uint64_t)n_chains * n_steps * 4, 1));
    GL355_TRY(st.open(trace, (uint64_t)n_chains * n_steps * HK_REC * 4, 2));
    Scratch pm(ctx);
    GL355_TRY(pm.get((uint64_t)n_operands * 64));
    if (form <= GL355_BN_CHAIN_JAC) {
        hipLaunchKernelGGL(bn254_chain_table_kernel, dim3((n_operands + 255) / 256), dim3(256), 0, ctx->stream, so.as<const uint32_t>(), n_operands,
                           pm.as<uint32_t>(), (int32_t)(form == GL355_BN_CHAIN_JAC));
        GL355_HIP(ctx, hipGetLastError());
    }
    if (form == GL355_BN_CHAIN_J) {
        GL355_TRY(bn254_j_chain_hook(ctx, so.as<const uint32_t>(), n_operands, ss.as<const uint32_t>(), n_chains, n_steps, st.as<uint32_t>()));
        return st.finish();
    }
    hipLaunchKernelGGL(bn254_chain_hook_kernel, dim3((n_chains + 63) / 64), dim3(64), 0, ctx->stream, form, so.as<const uint32_t>(), n_operands,
                       pm.as<uint32_t>(), ss.as<const uint32_t>(), n_chains, n_steps, st.as<uint32_t>());
    GL355_HIP(ctx, hipGetLastError());
    return st.finish();
}
}  // extern "C"
