// ParamsKZG of the reference's SNARK finalisation: setup, commit / commit_lagrange and the single-point opening, as
// `verify_inside_snark` reaches them (src/plonky2_verifier/verifier_api.rs:77-92, chip/native_chip/test_utils.rs:57-95), and the fixed-base
// multiplication the setup's powers of tau go through; the other fixed-base table, the window multiples of an SRS that gl355_bn254_g1_msm_prepare
// builds for the MSM, is here too (see msm_table_build_kernel for why).  The composites are host code over the Fr FFT (bn254_fr_fft.hip) and the MSM
// (bn254_msm.hip) plus the few kernels below; checked against oracle/bn254_curve_oracle.c.
#include "bn254_msm_acc.cuh"
#include <memory>

namespace gl355 {

// ================================================================ fixed-base batch multiplication ===================
// out[i] = scalars[i] * base for one base point: what ParamsKZG::setup does for the powers of tau ([s^i] G, verifier_api.rs:77).
// 8-bit windows over a table T[w][d] = d * 2^(8 w) * base (32 x 256 affine points, built per call): one mixed addition per non-zero
// byte of the scalar and one inversion per output -- no doublings in the main loop.
struct FbArgs {
    const uint64_t* base;       // [8] affine, canonical integers
    const uint64_t* scalars;    // [n][4]
    uint64_t n;
    uint32_t* win;              // [32][24]       2^(8 w) * base, Jacobian
    uint32_t* table;            // [32][256][16]  affine Montgomery x | y; d = 0 unused
    uint64_t* out;              // [n][8]
};
__global__ void fb_windows_kernel(FbArgs a) {                            // lane w: 8 w doublings of the base
    const uint32_t w = threadIdx.x;
    if (w >= 32) return;
    const u256 x = load256(a.base), y = load256(a.base + 4);
    jac p;
    if (u_is_zero(x) && u_is_zero(y)) p = j_identity();
    else { p.x = m_from_int<F_Q>(x); p.y = m_from_int<F_Q>(y); p.z = u_const(BN254C_FQ_ONE); }
    for (uint32_t k = 0; k < 8 * w; k++) p = j_double(p);
    j_store(a.win + 24 * w, p);
}
__global__ void __launch_bounds__(256) fb_table_kernel(FbArgs a) {       // lane (w, d): d * B_w by double-and-add, to affine
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 32 * 256) return;
    const uint32_t d = g & 255;
    const jac b = j_load(a.win + 24 * (g >> 8));
    jac acc = j_identity();
    for (int bit = 7; bit >= 0; bit--) {
        acc = j_double(acc);
        if ((d >> bit) & 1) acc = j_add(acc, b);
    }
    u256 x = u_zero(), y = u_zero();
    if (!j_is_identity(acc)) j_to_affine_mont(acc, x, y);
    uint32_t* t = a.table + 16ull * g;
#pragma unroll
    for (int j = 0; j < 8; j++) { t[j] = x.l[j]; t[8 + j] = y.l[j]; }
}
__global__ void __launch_bounds__(256) fb_mul_kernel(FbArgs a) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t* k = a.scalars + 4 * i;
    jac acc = j_identity();
    for (uint32_t w = 0; w < 32; w++) {
        const uint32_t d = (uint32_t)(k[w >> 3] >> (8 * (w & 7))) & 255u;
        if (!d) continue;
        const uint32_t* t = a.table + 16ull * (w * 256 + d);
        u256 x, y;
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) { x.l[j] = t[j]; y.l[j] = t[8 + j]; o |= t[j] | t[8 + j]; }
        if (o) acc = j_madd(acc, x, y);                                // a zero entry: d * B_w is the identity (base of small order)
    }
    uint64_t* dst = a.out + 8 * i;
    if (j_is_identity(acc)) {
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = 0;
        return;
    }
    u256 x, y;
    j_to_affine_mont(acc, x, y);
    store256(dst, m_to_int<F_Q>(x));
    store256(dst + 4, m_to_int<F_Q>(y));
}

// ================================================================ prepared bases of the MSM =========================
// The table gl355_bn254_g1_msm_prepare builds for bn254_msm.hip: tab[w][i] = 2^(c w) P_i in the bucket loops' table form, w < wps.  It lives in this unit
// because of j_double: the register budget of a __noinline__ device function follows the launch bounds of ALL the kernels that call it within a unit, and
// alone with this kernel (256 lanes per workgroup) j_double comes out at 179 VGPRs and the kernel at two waves per SIMD; next to fb_windows_kernel (no
// bound) it stays at four (profiles/bn254_curve_split_resources.txt).  One lane per base walks its windows by c doublings
// each (Jacobian, 8 x 32-bit form), keeps X | Y in the table slot and Z and the running product of the Zs in scratch, inverts the product once
// and walks back (Montgomery's trick along the lane's own chain: 3 products per window instead of an inversion).  A multiple of a point of this
// prime-order group is never the identity and never has y = 0, so no Z is zero.
struct MsmTabArgs {
    const uint64_t* points;     // [n][8] affine, canonical
    uint32_t* tab;              // [wps][n][16]
    uint32_t* zs;               // [wps - 1][chunk][8]  Z of window w + 1 (Montgomery)
    uint32_t* pre;              // [wps - 1][chunk][8]  Z_1 ... Z_(w + 1)
    uint64_t n, i0, chunk;      // this launch covers bases [i0, min(n, i0 + chunk))
    uint32_t c, wps;
};
__global__ void __launch_bounds__(256) msm_table_build_kernel(MsmTabArgs a) {
    const uint64_t li = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, i = a.i0 + li;
    if (li >= a.chunk || i >= a.n) return;
    const u256 x = load256(a.points + 8 * i), y = load256(a.points + 8 * i + 4);
    if (u_is_zero(x) && u_is_zero(y)) {
        for (uint32_t w = 0; w < a.wps; w++) {
            uint32_t* t = a.tab + 16ull * ((uint64_t)w * a.n + i);
#pragma unroll
            for (int j = 0; j < 16; j++) t[j] = 0;
        }
        return;
    }
    jac q;
    q.x = m_from_int<F_Q>(x); q.y = m_from_int<F_Q>(y); q.z = u_const(BN254C_FQ_ONE);
    {
        const u256 xt = msm_table_form(q.x), yt = msm_table_form(q.y);
        uint32_t* t = a.tab + 16ull * i;
#pragma unroll
        for (int j = 0; j < 8; j++) { t[j] = xt.l[j]; t[8 + j] = yt.l[j]; }
    }
    u256 prefix = q.z;
    for (uint32_t w = 1; w < a.wps; w++) {
        for (uint32_t d = 0; d < a.c; d++) q = j_double(q);
        uint32_t* t = a.tab + 16ull * ((uint64_t)w * a.n + i);
        uint32_t* z = a.zs + 8ull * ((uint64_t)(w - 1) * a.chunk + li);
        uint32_t* pr = a.pre + 8ull * ((uint64_t)(w - 1) * a.chunk + li);
        prefix = w == 1 ? q.z : m_mul<F_Q>(prefix, q.z);
#pragma unroll
        for (int j = 0; j < 8; j++) { t[j] = q.x.l[j]; t[8 + j] = q.y.l[j]; z[j] = q.z.l[j]; pr[j] = prefix.l[j]; }
    }
    if (a.wps < 2) return;
    u256 inv = m_inv<F_Q>(prefix);                            // 1 / (Z_1 ... Z_(wps - 1))
    for (uint32_t w = a.wps - 1; w >= 1; w--) {
        uint32_t* t = a.tab + 16ull * ((uint64_t)w * a.n + i);
        const uint32_t* z = a.zs + 8ull * ((uint64_t)(w - 1) * a.chunk + li);
        u256 zi = inv, zw, X, Y;
        if (w > 1) {
            const uint32_t* pr = a.pre + 8ull * ((uint64_t)(w - 2) * a.chunk + li);
            u256 pw;
#pragma unroll
            for (int j = 0; j < 8; j++) pw.l[j] = pr[j];
            zi = m_mul<F_Q>(inv, pw);                         // 1 / Z_w
        }
#pragma unroll
        for (int j = 0; j < 8; j++) { zw.l[j] = z[j]; X.l[j] = t[j]; Y.l[j] = t[8 + j]; }
        inv = m_mul<F_Q>(inv, zw);
        const u256 zi2 = m_mul<F_Q>(zi, zi);
        const u256 xt = msm_table_form(m_mul<F_Q>(X, zi2)), yt = msm_table_form(m_mul<F_Q>(Y, m_mul<F_Q>(zi2, zi)));
#pragma unroll
        for (int j = 0; j < 8; j++) { t[j] = xt.l[j]; t[8 + j] = yt.l[j]; }
    }
}

}  // namespace gl355

using namespace gl355;

// ================================================================ KZG composites ====================
// ParamsKZG::setup / commit / commit_lagrange and the single-point opening the SHPLONK prover reduces to, as the reference reaches them
// through verify_inside_snark (src/plonky2_verifier/verifier_api.rs:77-92, chip/native_chip/test_utils.rs:57-95; k = 23 in README.md:171-177).
// Scalars cross the ABI as plain 256-bit integers (4 x u64, any value: reduced on load); kernels work in Montgomery form.

// out[i] = tau^i (plain integers), i < n: the scalars of the powers-of-tau loop
__global__ void kzg_tau_powers_kernel(u256 tau_mont, uint64_t n, uint64_t* out) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    store256(out + 4 * i, m_to_int<F_R>(m_pow_u64<F_R>(tau_mont, i)));
}
// out[i] = L_i(tau) = (tau^n - 1) / n * w^i / (tau - w^i) (plain integers): the Lagrange basis of the 2^k domain at tau.  A lane takes KZG_LG_CHUNK
// consecutive i: one inversion per chunk (Montgomery's trick).  *bad is set if tau lies in the domain.
constexpr int KZG_LG_CHUNK = 16;
__global__ void __launch_bounds__(64) kzg_lagrange_kernel(u256 tau_mont, u256 w_mont, u256 w_inv_mont, u256 c_mont /* (tau^n - 1) / n */, uint64_t n,
                                                          uint64_t* out, uint64_t* pre /* n x 4 scratch */, uint32_t* bad) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t i0 = t * KZG_LG_CHUNK;
    if (i0 >= n) return;
    const uint64_t i1 = min(n, i0 + KZG_LG_CHUNK);
    u256 wi = m_pow_u64<F_R>(w_mont, i0);
    u256 acc = u_const(f_one<F_R>());
#pragma unroll 1
    for (uint64_t i = i0; i < i1; i++) {                 // forward: denominators (kept in out[]) and their running products
        const u256 d = m_sub<F_R>(tau_mont, wi);
        if (m_is_zero<F_R>(d)) atomicOr(bad, 1u);
        store256(pre + 4 * i, acc);
        store256(out + 4 * i, d);
        acc = m_mul<F_R>(acc, d);
        if (i + 1 < i1) wi = m_mul<F_R>(wi, w_mont);
    }
    u256 inv = m_inv<F_R>(acc);
#pragma unroll 1
    for (uint64_t i = i1; i-- > i0;) {                   // backward: 1 / d_i = inv * pre_i, then inv *= d_i; w^i steps down with w^-1
        const u256 d = load256(out + 4 * i);
        const u256 dinv = m_mul<F_R>(inv, load256(pre + 4 * i));
        inv = m_mul<F_R>(inv, d);
        store256(out + 4 * i, m_to_int<F_R>(m_mul<F_R>(m_mul<F_R>(c_mont, wi), dinv)));
        wi = m_mul<F_R>(wi, w_inv_mont);
    }
}
// Synthetic division by (X - z) as a blocked suffix Horner scan.  For an array A of m field elements and a point Z:
//     Q[i] = sum_{j > i} A[j] Z^(j - i - 1)  (i < m; Q[m-1] = 0),      E = sum_j A[j] Z^j.
// With A = the coefficients of p and Z = z: Q[0 .. n-2] are the coefficients of (p - p(z)) / (X - z) and E = p(z).
// Level kernels: (1) a lane's chunk value H_t = sum_{j in chunk t} A[j] Z^(j - start_t); the carries C_t = Q_H[t] of the array H at the
// point Z^chunk come from the next level (same problem, m / chunk elements); (3) a lane walks its chunk downwards from its carry.
constexpr uint32_t KZG_DIV_CHUNK = 64;
__global__ void kzg_div_chunk_kernel(const uint64_t* A, uint64_t m, u256 z_mont, int a_is_mont, uint64_t* H /* Montgomery */) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t s0 = t * KZG_DIV_CHUNK;
    if (s0 >= m) return;
    const uint64_t e0 = min(m, s0 + KZG_DIV_CHUNK);
    u256 h = u_zero();
#pragma unroll 1
    for (uint64_t j = e0; j-- > s0;) {
        const u256 a = a_is_mont ? load256(A + 4 * j) : m_from_int<F_R>(load256(A + 4 * j));
        h = m_add<F_R>(m_mul<F_R>(h, z_mont), a);
    }
    store256(H + 4 * t, h);
}
// carry == nullptr: the whole array is one chunk (m <= KZG_DIV_CHUNK), lane 0 only.  q_plain: write Q as plain integers (the top level)
__global__ void kzg_div_walk_kernel(const uint64_t* A, uint64_t m, u256 z_mont, int a_is_mont, const uint64_t* carry /* Montgomery, per chunk */,
                                    uint64_t* Q, int q_plain, uint64_t* E /* Montgomery; written by the lane of chunk 0 */) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t s0 = t * KZG_DIV_CHUNK;
    if (s0 >= m) return;
    const uint64_t e0 = min(m, s0 + KZG_DIV_CHUNK);
    u256 sacc = carry ? load256(carry + 4 * t) : u_zero();
#pragma unroll 1
    for (uint64_t j = e0; j-- > s0;) {
        store256(Q + 4 * j, q_plain ? m_to_int<F_R>(sacc) : sacc);         // Q[j] = the running suffix value before A[j] enters
        const u256 a = a_is_mont ? load256(A + 4 * j) : m_from_int<F_R>(load256(A + 4 * j));
        sacc = m_add<F_R>(m_mul<F_R>(sacc, z_mont), a);
    }
    if (t == 0 && E) store256(E, sacc);
}
__global__ void kzg_from_mont1_kernel(const uint64_t* in, uint64_t* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) store256(out, m_to_int<F_R>(load256(in)));
}

namespace gl355 {
// Q and E of the comment above the division kernels, levels chained on the stream; A and Q are device arrays (Q plain at the top level)
int32_t kzg_divide(Ctx* ctx, const uint64_t* A, uint64_t m, const Fr& z, int a_is_mont, uint64_t* Q, int q_plain, uint64_t* E_mont) {
    const u256 z_mont = to_u256(z.l);
    if (m <= KZG_DIV_CHUNK) {
        hipLaunchKernelGGL(kzg_div_walk_kernel, dim3(1), dim3(64), 0, ctx->stream, A, m, z_mont, a_is_mont, (const uint64_t*)nullptr, Q, q_plain, E_mont);
        GL355_HIP(ctx, hipGetLastError());
        return GL355_OK;
    }
    const uint64_t chunks = (m + KZG_DIV_CHUNK - 1) / KZG_DIV_CHUNK;
    Scratch sc(ctx);
    GL355_TRY(sc.get(chunks * 64));
    uint64_t* H = sc.as<uint64_t>();
    uint64_t* C = H + 4 * chunks;
    hipLaunchKernelGGL(kzg_div_chunk_kernel, dim3((uint32_t)((chunks + 63) / 64)), dim3(64), 0, ctx->stream, A, m, z_mont, a_is_mont, H);
    GL355_HIP(ctx, hipGetLastError());
    Fr zc = z;                                               // Z = z^chunk
    for (uint32_t k = 1; k < KZG_DIV_CHUNK; k <<= 1) zc = zc * zc;
    GL355_TRY(kzg_divide(ctx, H, chunks, zc, 1, C, 0, nullptr));
    hipLaunchKernelGGL(kzg_div_walk_kernel, dim3((uint32_t)((chunks + 63) / 64)), dim3(64), 0, ctx->stream, A, m, z_mont, a_is_mont, (const uint64_t*)C, Q, q_plain, E_mont);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

}  // namespace gl355

extern "C" {

int32_t gl355_bn254_g1_fixed_base_mul(gl355_ctx* h, const uint64_t base[8], const uint64_t* scalars, uint64_t n, uint64_t* out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!base || ((!scalars || !out) && n)) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_fixed_base_mul: null argument");
    if (n > (1ull << 26)) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_fixed_base_mul: more than 2^26 scalars");
    if (n == 0) return GL355_OK;
    Staged sb(ctx), ss(ctx), so(ctx);
    GL355_TRY(sb.open(base, 64, 1));
    GL355_TRY(ss.open(scalars, n * 32, 1));
    GL355_TRY(so.open(out, n * 64, 2));
    Scratch buf(ctx);
    GL355_TRY(buf.get((32 * 24 + 32 * 256 * 16) * 4 + 64));
    FbArgs a;
    a.base = sb.as<uint64_t>(); a.scalars = ss.as<uint64_t>(); a.n = n; a.out = so.as<uint64_t>();
    a.win = buf.as<uint32_t>(); a.table = a.win + 32 * 24;
    {
        ProfScope ps(ctx, "bn254_g1_fixed_base_mul", n * 96);
        hipLaunchKernelGGL(fb_windows_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(fb_table_kernel, dim3(32), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(fb_mul_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
        GL355_HIP(ctx, hipGetLastError());
    }
    return so.finish();
}

// Window width of a prepared base set.  With the buckets shared by all windows the reduction is paid once per scalar set, so wider windows than the
// per-window form's 17 - 20 bits pay: fewer windows = fewer additions in the bucket loops (n per window), until the buckets outnumber them.
static uint32_t msm_prepared_window_bits(uint32_t lg) {
    // ... and the top window should not be nearly empty (r < 2^254: a top window of two bits is four buckets of millions of points): the widest c from
    // lg - 1 down whose top window keeps at least c / 3 bits.  2^23: 22 (11 windows of 22 bits + 12 bits), 2^22, 2^21: 20, 2^20: 19, 2^18: 17
    // (k = 23 proof, ms of MSM kernels: c = 20 / 21 / 22 / 23 -> 409 / 440 / 408 / 480 before the mid-size bucket items grew; 417 without tables)
    for (uint32_t c = std::min(22u, std::max(13u, lg) - 1); c > 12; c--)
        if (254 - c * (253 / c) >= (c + 2) / 3) return c;
    return 12;
}
int32_t gl355_bn254_g1_msm_prepare(gl355_ctx* h, const uint64_t* points, uint64_t n, gl355_msm_bases** out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!points || !out || !n) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm_prepare: null argument or no points");
    uint32_t lg = 0;
    while ((1ull << lg) < n) lg++;
    const uint32_t c = msm_prepared_window_bits(lg), wps = 256 / c + 1;
    if (n > (1ull << 26) || n * wps >= (1ull << 31)) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_msm_prepare: too many points");
    std::unique_ptr<gl355_msm_bases> b(new gl355_msm_bases{ctx, nullptr, n, c, wps});
    void* tab = nullptr;
    GL355_TRY(ctx->alloc((size_t)wps * n * 64, &tab));
    b->tab = static_cast<uint32_t*>(tab);
    Staged sp(ctx);
    int32_t rc = sp.open(points, n * 64, 1);
    Scratch tmp(ctx);
    MsmTabArgs a;
    memset(&a, 0, sizeof a);
    a.points = sp.as<uint64_t>(); a.tab = b->tab; a.n = n; a.c = c; a.wps = wps;
    a.chunk = std::min<uint64_t>(n, 1ull << 20);
    if (rc == GL355_OK) rc = tmp.get((size_t)(wps - 1) * a.chunk * 64 + 64);
    if (rc != GL355_OK) { ctx->release(tab); return rc; }
    a.zs = tmp.as<uint32_t>(); a.pre = a.zs + 8ull * (wps - 1) * a.chunk;
    {
        ProfScope ps(ctx, "bn254_g1_msm_prepare", n * 64ull * (1 + wps));
        for (a.i0 = 0; a.i0 < n; a.i0 += a.chunk)
            hipLaunchKernelGGL(msm_table_build_kernel, dim3((uint32_t)((a.chunk + 255) / 256)), dim3(256), 0, ctx->stream, a);
    }
    if (hipGetLastError() != hipSuccess || ctx->wait() != hipSuccess) { ctx->release(tab); return ctx->fail(GL355_E_HIP, "bn254_g1_msm_prepare: kernel failed"); }
    *out = b.release();
    return GL355_OK;
}

// ---- KZG composites ------------------------------------------------------------------------------------------------------------
// ParamsKZG::setup(k, rng) with the secret handed in (verifier_api.rs:77): g[i] = [tau^i] G1, g_lagrange[i] = [L_i(tau)] G1, G1 = (1, 2).
// halo2 computes g_lagrange by an inverse FFT over the GROUP; here the Lagrange scalars are evaluated in Fr (one batched inversion per 16
// points) and go through the same fixed-base kernel as the powers.  g_lagrange may be NULL.  Outputs are affine points (n x 8 words).
int32_t gl355_kzg_setup(gl355_ctx* h, const uint64_t tau[4], uint32_t log_n, uint64_t* g, uint64_t* g_lagrange) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!tau || !g) return ctx->fail(GL355_E_INVALID_ARG, "kzg_setup: null argument");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "kzg_setup: log_n > 26");
    const uint64_t n = 1ull << log_n;
    uint64_t tau_h[4];                                        // tau may be device memory like every other operand
    if (ptr_is_device(tau)) { GL355_HIP(ctx, hipMemcpy(tau_h, tau, 32, hipMemcpyDeviceToHost)); } else memcpy(tau_h, tau, 32);
    const Fr t = Fr::from_words(tau_h);
    const u256 tau_mont = to_u256(t.l);
    Fr tn = t;                                                // tau^n
    for (uint32_t k = 0; k < log_n; k++) tn = tn * tn;
    // tau in the 2^log_n domain <=> tau^n = 1: refused whether or not the Lagrange bases are asked for (the header says so)
    if (tn == Fr::one()) return ctx->fail(GL355_E_INVALID_ARG, "kzg_setup: tau lies in the evaluation domain");
    Scratch sc(ctx);
    GL355_TRY(sc.get((g_lagrange ? 2 : 1) * n * 32 + 64));
    uint64_t* d_s = sc.as<uint64_t>();
    uint64_t* d_pre = d_s + 4 * n;                          // Lagrange pass only
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_s + 4 * n * (g_lagrange ? 2 : 1));
    const uint64_t gen[8] = {1, 0, 0, 0, 2, 0, 0, 0};
    {
        ProfScope ps(ctx, "kzg_setup_scalars", n * 32);
        hipLaunchKernelGGL(kzg_tau_powers_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, tau_mont, n, d_s);
        GL355_HIP(ctx, hipGetLastError());
    }
    GL355_TRY(gl355_bn254_g1_fixed_base_mul(h, gen, d_s, n, g));
    if (g_lagrange) {
        // c = (tau^n - 1) / n
        const Fr c = (tn - Fr::one()) * Fr::from_u64(n).inv();
        GL355_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
        {
            ProfScope ps(ctx, "kzg_setup_scalars", n * 32);
            const uint64_t lanes = (n + KZG_LG_CHUNK - 1) / KZG_LG_CHUNK;
            const Fr w = Fr::root_of_unity(log_n);
            hipLaunchKernelGGL(kzg_lagrange_kernel, dim3((uint32_t)((lanes + 63) / 64)), dim3(64), 0, ctx->stream, tau_mont, to_u256(w.l),
                               to_u256(w.inv().l), to_u256(c.l), n, d_s, d_pre, d_bad);
            GL355_HIP(ctx, hipGetLastError());
        }
        uint32_t bad = 0;
        GL355_HIP(ctx, ctx->d2h(&bad, d_bad, 4));
        GL355_HIP(ctx, ctx->wait());
        if (bad) return ctx->fail(GL355_E_INVALID_ARG, "kzg_setup: tau lies in the evaluation domain");
        GL355_TRY(gl355_bn254_g1_fixed_base_mul(h, gen, d_s, n, g_lagrange));
    }
    return GL355_OK;
}

// ParamsKZG::commit / commit_lagrange: result = sum_i poly[i] * g[i] over 2^log_n bases.  values_form = 0: `poly` are the scalars that go
// with the given bases as they are (coefficients with the monomial bases g, or evaluations with g_lagrange -- an MSM does not care);
// values_form = 1: `poly` are EVALUATIONS over the 2^log_n domain but `g` are the monomial bases: inverse FFT on a scratch copy, then the MSM.
int32_t gl355_kzg_commit(gl355_ctx* h, const uint64_t* g, const uint64_t* poly, uint32_t log_n, int32_t values_form, uint64_t result[8]) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!g || !poly || !result) return ctx->fail(GL355_E_INVALID_ARG, "kzg_commit: null argument");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "kzg_commit: log_n > 26");
    const uint64_t n = 1ull << log_n;
    if (!values_form) return gl355_bn254_g1_msm(h, g, poly, n, result);
    Scratch sc(ctx);
    GL355_TRY(sc.get(n * 32));
    uint64_t* d_c = sc.as<uint64_t>();
    GL355_HIP(ctx, hipMemcpyAsync(d_c, poly, n * 32, ptr_is_device(poly) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (log_n) GL355_TRY(fr_ntt_run(ctx, d_c, log_n, d_c, n, log_n, 1, nullptr));
    return gl355_bn254_g1_msm(h, g, d_c, n, result);
}

// The single-point KZG opening (what halo2's multiopen provers reduce to per rotation set): eval = p(z), witness = commit((p - p(z)) / (X - z)).
// `coeffs` are the 2^log_n coefficients of p, `g` the monomial bases.  quotient (optional, 2^log_n x 4 words, device or host) receives the
// quotient's coefficients (the last one is 0).
int32_t gl355_kzg_open(gl355_ctx* h, const uint64_t* g, const uint64_t* coeffs, uint32_t log_n, const uint64_t z[4], uint64_t eval[4],
                       uint64_t witness[8], uint64_t* quotient) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!g || !coeffs || !z || !eval || !witness) return ctx->fail(GL355_E_INVALID_ARG, "kzg_open: null argument");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "kzg_open: log_n > 26");
    const uint64_t n = 1ull << log_n;
    Staged sp(ctx);
    GL355_TRY(sp.open(coeffs, n * 32, 1));
    Scratch sq(ctx);
    GL355_TRY(sq.get(n * 32 + 64));
    uint64_t* d_q = sq.as<uint64_t>();
    uint64_t* d_e = d_q + 4 * n;
    {
        ProfScope ps(ctx, "kzg_divide", n * 64);
        uint64_t z_h[4];
        if (ptr_is_device(z)) { GL355_HIP(ctx, hipMemcpy(z_h, z, 32, hipMemcpyDeviceToHost)); } else memcpy(z_h, z, 32);
        GL355_TRY(kzg_divide(ctx, sp.as<uint64_t>(), n, Fr::from_words(z_h), 0, d_q, 1, d_e));
        hipLaunchKernelGGL(kzg_from_mont1_kernel, dim3(1), dim3(64), 0, ctx->stream, (const uint64_t*)d_e, d_e + 4);
        GL355_HIP(ctx, hipGetLastError());
    }
    if (ptr_is_device(eval)) GL355_HIP(ctx, hipMemcpyAsync(eval, d_e + 4, 32, hipMemcpyDeviceToDevice, ctx->stream));
    else GL355_HIP(ctx, ctx->d2h(eval, d_e + 4, 32));
    if (quotient) GL355_HIP(ctx, hipMemcpyAsync(quotient, d_q, n * 32, ptr_is_device(quotient) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    GL355_HIP(ctx, ctx->wait());
    return gl355_bn254_g1_msm(h, g, d_q, n, witness);
}

}  // extern "C"
