// The radix-2 FFT over BN254 G1: elements are points, twiddles are Fr scalars.  halo2_proofs derives the Lagrange bases of a KZG
// parameter set from its monomial bases this way (ParamsKZG::downsize / g_to_lagrange: g_lagrange = inverse FFT of g[0 .. 2^k)), which is
// what a deployment with ceremony parameters -- public [tau^i] G1 and no tau -- has instead of ParamsKZG::setup (verifier_api.rs:77).
//
// Schedule: decimation in time.  The input pass reads the caller's affine points in bit-reversed order, checks them (coordinates < q,
// y^2 = x^3 + 3; G1 has cofactor 1) and writes Montgomery Jacobian points (96 B each) to a resident buffer; one kernel per stage runs the
// butterflies (a, b) -> (a + w^j b, a - w^j b) on it; the output pass scales by 1/n (inverse) and converts to affine canonical integers.
// The cost is the scalar multiplication w^j b (~2.9k Fq products; a stage moves 1.6 GB at 2^23, 0.3 ms of HBM time against seconds of
// VALU work), so it must not diverge: every lane follows the same fixed-window signed-digit schedule -- 4 doublings, then one addition
// of a table entry d P, |d| <= 8 -- whatever its twiddle.  A zero digit adds the identity from entry 0 (a branch of a few instructions
// inside the addition, not a skipped addition), a negative one the entry with y negated.  The per-lane table (9 Jacobian points) is
// indexed by the lane's digit and so lives in scratch.
#include "bn254_g1.cuh"

namespace gl355 {

constexpr int G1F_WIN = 4;                                   // window bits; digits in [-8, 8]
constexpr int G1F_WINDOWS = 256 / G1F_WIN;

// [k] P for a plain 256-bit integer k (any value; the windows cover all 256 bits, the top carry enters as a 65th digit of 0 or 1)
GL_DEV jac g1_mul_signed_window(const jac& p, const u256& k) {
    jac tab[9];
    tab[0] = j_identity();
    tab[1] = p;
    tab[2] = j_double(p);
    tab[3] = j_add_inl(tab[2], p);
    tab[4] = j_double(tab[2]);
    tab[5] = j_add_inl(tab[4], p);
    tab[6] = j_double(tab[3]);
    tab[7] = j_add_inl(tab[6], p);
    tab[8] = j_double(tab[4]);
    // signed recoding from the bottom: raw = nibble + carry-in; raw >= 8 becomes raw - 16 and carries one.  neg bit i = carry out of window i.
    uint64_t neg = 0;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < G1F_WINDOWS; i++) {
        const uint32_t raw = ((k.l[i >> 3] >> (4 * (i & 7))) & 15u) + c;
        c = raw >= 8u ? 1u : 0u;
        neg |= (uint64_t)c << i;
    }
    jac acc = c ? p : tab[0];
#pragma unroll 1
    for (int i = G1F_WINDOWS - 1; i >= 0; i--) {
#pragma unroll
        for (int d = 0; d < G1F_WIN; d++) acc = j_double(acc);
        const uint32_t cin = i ? (uint32_t)(neg >> (i - 1)) & 1u : 0u, cout = (uint32_t)(neg >> i) & 1u;
        const uint32_t raw = ((k.l[i >> 3] >> (4 * (i & 7))) & 15u) + cin;
        const uint32_t mag = cout ? 16u - raw : raw;
        jac t = tab[mag];
        const u256 ny = m_sub<F_Q>(u_zero(), t.y);
#pragma unroll
        for (int l = 0; l < 8; l++) t.y.l[l] = cout ? ny.l[l] : t.y.l[l];
        acc = j_add_inl(acc, t);
    }
    return acc;
}

// data[i] = in[bitrev(i)] as a Montgomery Jacobian point; *bad |= 1 for a coordinate >= q or a point off the curve ((0, 0) = identity)
__global__ void __launch_bounds__(256) g1_fft_load_kernel(const uint64_t* in, uint32_t* data, uint32_t log_n, uint32_t* bad) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= (1ull << log_n)) return;
    const uint64_t src = log_n ? __brevll(i) >> (64 - log_n) : 0;
    const u256 x = load256(in + 8 * src), y = load256(in + 8 * src + 4);
    jac p = j_identity();
    if (!(u_is_zero(x) && u_is_zero(y))) {
        const bool canon = u_eq(u_cond_sub(x, BN254C_FQ_MOD), x) && u_eq(u_cond_sub(y, BN254C_FQ_MOD), y);
        p.x = m_from_int<F_Q>(x);
        p.y = m_from_int<F_Q>(y);
        p.z = u_const(BN254C_FQ_ONE);
        const u256 one = u_const(BN254C_FQ_ONE), b3 = m_add<F_Q>(m_add<F_Q>(one, one), one);
        const u256 rhs = m_add<F_Q>(m_mul<F_Q>(m_mul<F_Q>(p.x, p.x), p.x), b3);
        if (!canon || !m_eq<F_Q>(m_mul<F_Q>(p.y, p.y), rhs)) atomicOr(bad, 1u);
    }
    j_store(data + 24 * i, p);
}

// decimation-in-time stage s (half span 2^(s-1)): one butterfly per lane, twiddle w_n^(j n / 2^s) from tw (Montgomery, w_n^i for i < n / 2)
__global__ void __launch_bounds__(256) g1_fft_stage_kernel(uint32_t* data, const uint64_t* tw, uint32_t log_n, uint32_t s) {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= (1ull << (log_n - 1))) return;
    const uint64_t half = 1ull << (s - 1);
    const uint64_t j = t & (half - 1), base = (t >> (s - 1)) << s;
    uint32_t* pu = data + 24 * (base + j);
    uint32_t* pv = pu + 24 * half;
    const jac u = j_load(pu);
    jac v = j_load(pv);
    if (j) v = g1_mul_signed_window(v, m_to_int<F_R>(load256(tw + 4 * (j << (log_n - s)))));   // digits of the canonical integer
    jac vn = v;
    vn.y = m_sub<F_Q>(u_zero(), v.y);
    j_store(pu, j_add_inl(u, v));
    j_store(pv, j_add_inl(u, vn));
}

// out[i] = affine canonical form of data[i] (times the plain integer `scale` when use_scale); the identity is written as zeros
__global__ void __launch_bounds__(256) g1_fft_store_kernel(const uint32_t* data, uint64_t* out, uint64_t n, u256 scale, int use_scale) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    jac p = j_load(data + 24 * i);
    if (use_scale) p = g1_mul_signed_window(p, scale);
    uint64_t* dst = out + 8 * i;
    if (j_is_identity(p)) {
#pragma unroll
        for (int l = 0; l < 8; l++) dst[l] = 0;
        return;
    }
    u256 x, y;
    j_to_affine_mont(p, x, y);
    store256(dst, m_to_int<F_Q>(x));
    store256(dst + 4, m_to_int<F_Q>(y));
}

// in / out: device arrays of 2^log_n affine points (may alias: every input is read before the first output is written).  Nothing is
// written to `out` when an input is refused.
static int32_t g1_fft_run(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, bool inverse, const char* who) {
    const uint64_t n = 1ull << log_n;
    Scratch sc(ctx);
    GL355_TRY(sc.get(n * 96 + (n / 2 + 1) * 32 + 64));
    uint32_t* data = sc.as<uint32_t>();
    uint64_t* tw = reinterpret_cast<uint64_t*>(data + 24 * n);
    uint32_t* d_bad = reinterpret_cast<uint32_t*>(tw + 4 * (n / 2 + 1));
    const uint32_t blk = (uint32_t)((n + 255) / 256), hblk = (uint32_t)((n / 2 + 255) / 256);
    GL355_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    {
        ProfScope ps(ctx, "bn254_g1_fft_load", n * (64 + 96));
        hipLaunchKernelGGL(g1_fft_load_kernel, dim3(blk), dim3(256), 0, ctx->stream, in, data, log_n, d_bad);
        GL355_HIP(ctx, hipGetLastError());
    }
    uint32_t bad = 0;
    GL355_HIP(ctx, ctx->d2h(&bad, d_bad, 4));
    GL355_HIP(ctx, ctx->wait());
    if (bad) return ctx->fail(GL355_E_INVALID_ARG, who);
    if (log_n) {
        GL355_TRY(bn254_fr_twiddles(ctx, log_n, inverse, tw));
        ProfScope ps(ctx, "bn254_g1_fft", n * 192ull * log_n);
        for (uint32_t s = 1; s <= log_n; s++)
            hipLaunchKernelGGL(g1_fft_stage_kernel, dim3(hblk), dim3(256), 0, ctx->stream, data, tw, log_n, s);
        GL355_HIP(ctx, hipGetLastError());
    }
    {
        uint64_t n_inv[4];
        Fr::from_u64(n).inv().to_words(n_inv);
        const u256 scale = to_u256(n_inv);                                        // n^-1 mod r, plain
        ProfScope ps(ctx, "bn254_g1_fft_store", n * (96 + 64));
        hipLaunchKernelGGL(g1_fft_store_kernel, dim3(blk), dim3(256), 0, ctx->stream, data, out, n, scale, inverse && log_n ? 1 : 0);
        GL355_HIP(ctx, hipGetLastError());
    }
    return GL355_OK;
}

}  // namespace gl355

using namespace gl355;

extern "C" {

// in place, natural order in and out: p[k] <- sum_i [w^(ik)] p[i] with gl355_bn254_fr_ntt's w (inverse: w^-1 and the 1/n)
int32_t gl355_bn254_g1_fft(gl355_ctx* h, uint64_t* points, uint32_t log_n, int32_t inverse) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!points) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_fft: null points");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_fft: log_n > 26 unsupported");
    const uint64_t n = 1ull << log_n;
    Staged sp(ctx);
    GL355_TRY(sp.open(points, n * 64, 3));
    GL355_TRY(g1_fft_run(ctx, sp.as<uint64_t>(), sp.as<uint64_t>(), log_n, inverse != 0, "bn254_g1_fft: a coordinate >= q or a point off the curve"));
    return sp.finish();
}

// ParamsKZG::downsize / g_to_lagrange: g_lagrange = inverse G1 FFT of the first 2^log_n monomial bases.  The inverse transform of
// [tau^j] G is [(1/n) sum_j tau^j w^-ij] G = [L_i(tau)] G, the bases gl355_kzg_setup makes from tau itself.
int32_t gl355_kzg_lagrange_from_powers(gl355_ctx* h, const uint64_t* g, uint64_t n_points, uint32_t log_n, uint64_t* g_lagrange) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!g || !g_lagrange) return ctx->fail(GL355_E_INVALID_ARG, "kzg_lagrange_from_powers: null argument");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "kzg_lagrange_from_powers: log_n > 26 unsupported");
    const uint64_t n = 1ull << log_n;
    if (n_points < n) return ctx->fail(GL355_E_INVALID_ARG, "kzg_lagrange_from_powers: fewer than 2^log_n monomial bases");
    Staged si(ctx), so(ctx);
    GL355_TRY(si.open(g, n * 64, 1));
    GL355_TRY(so.open(g_lagrange, n * 64, 2));
    GL355_TRY(g1_fft_run(ctx, si.as<uint64_t>(), so.as<uint64_t>(), log_n, true, "kzg_lagrange_from_powers: a coordinate >= q or a point off the curve"));
    return so.finish();
}

}  // extern "C"
