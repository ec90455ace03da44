// Test hooks of the Goldilocks product forms, of the partial rounds and of the 16-lane Poseidon permutation (include/gl355.h "test hooks";
// tests/test_gpu_gl_arith.py, tests/test_gpu_poseidon_b3.py, tests/test_gpu_poseidon_lanes.py): the shipped device functions of gl_field.cuh / poseidon.cuh / poseidon_lanes.cuh on raw u64 words.  No
// product path calls them.
#include "gl355_internal.h"
#include "poseidon.cuh"
#include "poseidon_lanes.cuh"

namespace gl355 {

// N recombinations of psd_recombine's form in lock-step (the two carry steps of one fill the wait states of the others: see gl_mul_multi).  The
// permutation's rows are chained now (poseidon.cuh psd_fold_multi) and no shipped kernel calls this; GL355_GL_RECOMBINE_MULTI4 keeps driving it.
template <int N>
GL_DEV void psd_recombine_multi(const uint64_t (&al)[N], const uint64_t (&ah)[N], uint64_t (&out)[N]) {
    static_assert(N >= 3, "three or more: no wait states of their own");
    uint32_t t1[N], top[N], m[N];
    uint64_t c[N], r[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_add_co_u32_e64 %0, %1, %2, %3" : "=v"(t1[j]), "=s"(c[j]) : "v"((uint32_t)(al[j] >> 32)), "v"((uint32_t)ah[j]));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_addc_co_u32_e64 %0, %1, 0, %2, %1" : "=v"(top[j]), "+s"(c[j]) : "v"((uint32_t)(ah[j] >> 32)));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        const uint64_t x = ((uint64_t)t1[j] << 32) | (uint32_t)al[j];
        asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(r[j]), "=s"(c[j]) : "v"(top[j]), "v"(x));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        asm("v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(m[j]) : "s"(c[j]));
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = r[j] + (uint64_t)m[j];
}

// records per lane of an op (one lane takes that many CONSECUTIVE records), 0 for an unknown op
static int hk_gl_width(int32_t op) {
    switch (op) {
    case GL355_GL_MUL: case GL355_GL_MUL_MULTI1: case GL355_GL_MUL_FILL: case GL355_GL_SQR: case GL355_GL_SBOX: case GL355_GL_RECOMBINE: return 1;
    case GL355_GL_MUL_MULTI2: case GL355_GL_MUL2_FILL: return 2;
    case GL355_GL_MUL_MULTI3: return 3;
    case GL355_GL_MUL_MULTI4: case GL355_GL_SBOX4: case GL355_GL_RECOMBINE_MULTI4: return 4;
    case GL355_GL_PARTIAL_ROUNDS: case GL355_GL_ROW_DENSE: case GL355_GL_ROW_B3: return 12;
    default: return 0;
    }
}

template <int N> GL_DEV void hk_mul_multi(const uint64_t* a, const uint64_t* b, uint64_t* out) {
    uint64_t x[N], y[N], r[N];
#pragma unroll
    for (int j = 0; j < N; j++) { x[j] = a[j]; y[j] = b[j]; }
    gl_mul_multi<N>(x, y, r);
#pragma unroll
    for (int j = 0; j < N; j++) out[j] = r[j];
}

// The fillers of gl_mul_fill / gl_mul2_fill, of the shape of the partial rounds' term(k) (poseidon_lanes.cuh): fill(k), k = 0 .. 4, is two multiply-adds,
// the halves of the row element xr[k] times the MDS entry PSD_CIRC_DEV[k], into the accumulators al and ah, which start from the halves of a constant.
// Here the constant is the lane's first b and xr[k] = a (k + 1) + b (wrapping) of the lane's first record; the accumulators go to out[n + i] and
// out[2 n + i] of that record.
struct HkRow {
    uint64_t xr[5], al, ah;
    GL_DEV HkRow(uint64_t a, uint64_t b) {
#pragma unroll
        for (int k = 0; k < 5; k++) xr[k] = a * (uint64_t)(k + 1) + b;
        al = (uint32_t)b; ah = b >> 32;
    }
    GL_DEV void term(int k) {
        al += (uint64_t)(uint32_t)xr[k] * PSD_CIRC_DEV[k];
        ah += (uint64_t)(uint32_t)(xr[k] >> 32) * PSD_CIRC_DEV[k];
    }
};

__global__ void __launch_bounds__(256) gl_arith_hook_kernel(int32_t op, int32_t width, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    const uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * (uint64_t)width;
    if (i >= n) return;                     // n is a multiple of width: the lane's records are i .. i + width - 1 < n
    const uint64_t* pa = a + i;
    const uint64_t* pb = b + i;             // (b = a for the one-operand ops)
    uint64_t* po = out + i;
    switch (op) {
    case GL355_GL_MUL: po[0] = gl_mul(pa[0], pb[0]); break;
    case GL355_GL_MUL_MULTI1: hk_mul_multi<1>(pa, pb, po); break;
    case GL355_GL_MUL_MULTI2: hk_mul_multi<2>(pa, pb, po); break;
    case GL355_GL_MUL_MULTI3: hk_mul_multi<3>(pa, pb, po); break;
    case GL355_GL_MUL_MULTI4: hk_mul_multi<4>(pa, pb, po); break;
    case GL355_GL_MUL_FILL: {
        HkRow row(pa[0], pb[0]);
        po[0] = gl_mul_fill(pa[0], pb[0], [&](int k) { row.term(k); });
        po[n] = row.al; po[2 * n] = row.ah;
        break;
    }
    case GL355_GL_MUL2_FILL: {
        HkRow row(pa[0], pb[0]);
        const uint64_t x[2] = {pa[0], pa[1]}, y[2] = {pb[0], pb[1]};
        uint64_t r[2];
        gl_mul2_fill(x, y, r, [&](int k) { row.term(k); });
        po[0] = r[0]; po[1] = r[1];
        po[n] = row.al; po[2 * n] = row.ah;
        po[n + 1] = 0; po[2 * n + 1] = 0;
        break;
    }
    case GL355_GL_SQR: po[0] = gl_sqr(pa[0]); break;
    case GL355_GL_SBOX: po[0] = psd_sbox(pa[0]); break;
    case GL355_GL_SBOX4: {
        uint64_t x0 = pa[0], x1 = pa[1], x2 = pa[2], x3 = pa[3];
        psd_sbox4(x0, x1, x2, x3);
        po[0] = x0; po[1] = x1; po[2] = x2; po[3] = x3;
        break;
    }
    case GL355_GL_RECOMBINE: po[0] = psd_recombine(pa[0], pb[0]); break;
    case GL355_GL_PARTIAL_ROUNDS: {
        uint64_t s[12];
#pragma unroll
        for (int j = 0; j < 12; j++) s[j] = pa[j];
        psd_partial_rounds_b3(s);
#pragma unroll
        for (int j = 0; j < 12; j++) po[j] = s[j];
        break;
    }
    // the chained rows.  Their constants are wave-uniform scalar operands in the permutation, so here they come from the HEAD of b, the same for every
    // lane of the launch: b[0] selects, the constants follow from b[2] in the layout the device tables have
    case GL355_GL_ROW_DENSE: {      // one MDS layer on twelve raw words: row r = b[2 + r] + sum_i CIRC[i] a[(i + r) % 12] (+ 8 a[0] for r = 0)
        uint64_t s[12];
#pragma unroll
        for (int j = 0; j < 12; j++) s[j] = pa[j];
        psd_b3add rc = (psd_b3add)(b + 2);
        asm volatile("" : "+s"(rc));
        psd_mds(s, rc);
#pragma unroll
        for (int j = 0; j < 12; j++) po[j] = s[j];
        break;
    }
    case GL355_GL_ROW_B3: {         // the rows of a block of three on u = a[0 .. 11], x = a[0 .. 2]; additive constants b[2 + 2 r], b[3 + 2 r] (low, high half) of row r
        uint64_t u[12], x[3], o[12], lo, hi;
#pragma unroll
        for (int j = 0; j < 12; j++) { u[j] = pa[j]; o[j] = 0; }
        x[0] = u[0]; x[1] = u[1]; x[2] = u[2];
        constexpr int W = PSD_B3_ROW_WORDS;
        psd_b3add add = (psd_b3add)(b + 2);
        psd_b3tab mac = (psd_b3tab)PSD_B3_MAC;
        const uint64_t row = b[0];
        asm volatile("" : "+s"(mac), "+s"(add));
        PsdB3Row k;
        if (row == 0) {             // y_1: 12 terms, a lone fold
            psd_b3_load<12>(k, mac, add);
            __builtin_amdgcn_sched_barrier(0);
            psd_b3_dot<1, 13>(u, x, k, mac + W, add + 2, lo, hi);
            o[0] = psd_fold(lo, hi);
        } else if (row == 1) {      // y_2: 13 terms
            psd_b3_load<13>(k, mac + W, add + 2);
            __builtin_amdgcn_sched_barrier(0);
            psd_b3_dot<2, 14>(u, x, k, mac + 2 * W, add + 4, lo, hi);
            o[0] = psd_fold(lo, hi);
        } else {                    // the twelve outgoing lanes, four folds in lock-step at a time
            psd_b3_load<14>(k, mac + 2 * W, add + 4);
            __builtin_amdgcn_sched_barrier(0);
            psd_b3_out<0>(o, u, x, mac, add, k);
        }
#pragma unroll
        for (int j = 0; j < 12; j++) po[j] = o[j];
        break;
    }
    default: {      // GL355_GL_RECOMBINE_MULTI4
        const uint64_t al[4] = {pa[0], pa[1], pa[2], pa[3]}, ah[4] = {pb[0], pb[1], pb[2], pb[3]};
        uint64_t r[4];
        psd_recombine_multi<4>(al, ah, r);
        po[0] = r[0]; po[1] = r[1]; po[2] = r[2]; po[3] = r[3];
        break;
    }
    }
}

// one 16-lane group = one state, block = 64 threads = 4 states, as merkle_level_lanes_kernel: a group past the end clamps to state 0 (the ring
// exchange needs the whole wave) and skips its stores only
template <int FORM>
__global__ void __launch_bounds__(64) poseidon_lanes_hook_kernel(uint64_t* states, uint64_t count) {
    __shared__ uint64_t rings[4][24];
    const int li = threadIdx.x & 15, grp = threadIdx.x >> 4;
    uint64_t g = blockIdx.x * 4ull + grp;
    const bool valid = g < count;
    if (!valid) g = 0;
    uint64_t s = (li < 12) ? states[g * 12 + li] : 0;
    s = psd_permute_lanes<FORM>(s, li, rings[grp]);
    if (valid && li < 12) states[g * 12 + li] = gl_canon(s);
}

}  // namespace gl355

using namespace gl355;

extern "C" {
int32_t gl355_gl_arith_batch(gl355_ctx* h, int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    const int width = hk_gl_width(op);
    if (!width) return ctx->fail(GL355_E_INVALID_ARG, "gl_arith_batch: bad op");
    if (n % (uint64_t)width) return ctx->fail(GL355_E_INVALID_ARG, "gl_arith_batch: n is not a multiple of the op's records per lane");
    if (n == 0) return GL355_OK;
    const bool rows = op == GL355_GL_ROW_DENSE || op == GL355_GL_ROW_B3;
    if (rows && n < 36) return ctx->fail(GL355_E_INVALID_ARG, "gl_arith_batch: the row ops read 30 words of constants from the head of b: three lanes or more");
    const bool two = !(op == GL355_GL_SQR || op == GL355_GL_SBOX || op == GL355_GL_SBOX4 || op == GL355_GL_PARTIAL_ROUNDS);
    if (!a || !out || (two && !b)) return ctx->fail(GL355_E_INVALID_ARG, "gl_arith_batch: null argument");
    const uint64_t lanes = n / (uint64_t)width;
    if ((lanes + 255) / 256 > 0x7FFFFFFFull) return ctx->fail(GL355_E_UNSUPPORTED, "gl_arith_batch: too many records");
    const uint64_t out_words = (op == GL355_GL_MUL_FILL || op == GL355_GL_MUL2_FILL) ? 3 * n : n;
    Staged sa(ctx), sb(ctx), so(ctx);
    GL355_TRY(sa.open(a, n * 8, 1));
    GL355_TRY(sb.open(two ? b : a, n * 8, 1));
    GL355_TRY(so.open(out, out_words * 8, 2));
    hipLaunchKernelGGL(gl_arith_hook_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, op, (int32_t)width, sa.as<const uint64_t>(),
                       sb.as<const uint64_t>(), so.as<uint64_t>(), n);
    GL355_HIP(ctx, hipGetLastError());
    return so.finish();
}

int32_t gl355_poseidon_permute_lanes(gl355_ctx* h, int32_t form, uint64_t* states, uint64_t count) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (form != 0 && form != 3) return ctx->fail(GL355_E_INVALID_ARG, "poseidon_permute_lanes: form is 0 or 3");
    if (count == 0) return GL355_OK;
    if (!states) return ctx->fail(GL355_E_INVALID_ARG, "poseidon_permute_lanes: null states");
    if ((count + 3) / 4 > 0x7FFFFFFFull) return ctx->fail(GL355_E_UNSUPPORTED, "poseidon_permute_lanes: too many states");
    Staged s(ctx);
    GL355_TRY(s.open(states, count * 96, 3));
    const dim3 grid((uint32_t)((count + 3) / 4)), block(64);
    if (form == 3) hipLaunchKernelGGL(poseidon_lanes_hook_kernel<3>, grid, block, 0, ctx->stream, s.as<uint64_t>(), count);
    else hipLaunchKernelGGL(poseidon_lanes_hook_kernel<0>, grid, block, 0, ctx->stream, s.as<uint64_t>(), count);
    GL355_HIP(ctx, hipGetLastError());
    return s.finish();
}
}  // extern "C"
