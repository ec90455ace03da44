// The scalar-field FFT of the reference's SNARK finalisation.
//
// `verify_inside_snark` (src/plonky2_verifier/verifier_api.rs:57-96) runs ParamsKZG::setup (:77), keygen_vk / keygen_pk (:78-79) and
// create_proof (:90) of halo2_proofs at k = 20..23 (chip/native_chip/test_utils.rs:57-95; README: ~505 s, the largest wall-time
// item of the product).  Inside, almost all of the time is two primitives of `halo2_proofs::arithmetic` over halo2curves' bn256; this is
//   best_fft       radix-2 FFT over the scalar field Fr (2-adicity 28, ROOT_OF_UNITY = 7^((r-1)/2^28))          -> gl355_bn254_fr_ntt
// (the other one, best_multiexp, is bn254_msm.hip).  halo2_proofs / halo2curves are un-vendored dependencies; the kernels follow their
// published definitions and are checked against oracle/bn254_curve_oracle.c (itself pinned by halo2curves' ROOT_OF_UNITY).
//
// Arithmetic: 8 x 32-bit limbs, Montgomery form with R = 2^256 (bn254_field.cuh).  A transform is a few passes over HBM with its stages in LDS
// (fr_fft_pass_kernel): ten in the first pass, at most seven in each later one.  bn254_fr_route.h states that split and which buffer each pass reads
// and writes; fr_launch below is the one place that fills and launches the passes.  The coset and resident forms the PLONK prover uses
// (plonk_bn254.hip) are parameters of the same pass.
#include "bn254_field.cuh"
#include "bn254_fr_route.h"
#include <vector>

namespace gl355 {

// ================================================================ Fr FFT ===========================================
// tw[i] = w^i (Montgomery), i < count, in two steps: lo[j] = w^j (j < 1024) and hi[j] = w^(1024 j) by exponentiation (a few thousand
// entries), then one product per entry.  (One exponentiation per entry -- ~30 products each -- cost more than the transform it served:
// 1.5e7 against 1.0e7 field products at k = 20.)
__global__ void fr_twiddle_seed_kernel(uint64_t* lo, uint64_t* hi, uint64_t n_hi, u256 w_mont) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < 1024) store256(lo + 4 * i, m_pow_u64<F_R>(w_mont, i));
    else if (i - 1024 < n_hi) store256(hi + 4 * (i - 1024), m_pow_u64<F_R>(w_mont, (i - 1024) << 10));
}
__global__ void fr_twiddle_kernel(uint64_t* tw, uint64_t count, const uint64_t* lo, const uint64_t* hi) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    store256(tw + 4 * i, m_mul<F_R>(load256(lo + 4 * (i & 1023)), load256(hi + 4 * (i >> 10))));
}
// the same powers as PLAIN integers times a plain factor f: (lo hi) R * f * R^-1 = lo hi f
__global__ void fr_power_plain_kernel(uint64_t* tab, uint64_t count, const uint64_t* lo, const uint64_t* hi, u256 f) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    store256(tab + 4 * i, m_canon<F_R>(m_mul<F_R>(m_mul<F_R>(load256(lo + 4 * (i & 1023)), load256(hi + 4 * (i >> 10))), f)));
}
// the same powers in Montgomery form times a Montgomery factor
__global__ void fr_power_mont_kernel(uint64_t* tab, uint64_t count, const uint64_t* lo, const uint64_t* hi, u256 f_mont) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= count) return;
    store256(tab + 4 * i, m_mul<F_R>(m_mul<F_R>(load256(lo + 4 * (i & 1023)), load256(hi + 4 * (i >> 10))), f_mont));
}

// the block constants of the coset form (FrPass::btw): out[2^(t-1) + b] = gpow[t] * w_(2^t)^rev(b), 1 <= t <= log_n, b < 2^(t-1); gpow[t] = g^(n / 2^t)
// (Montgomery, from the host), w_(2^t)^r = tw[r 2^(log_n - t)].  Entry 0 is unused.
__global__ void fr_coset_twiddle_kernel(const uint64_t* tw, const uint64_t* gpow, uint32_t log_n, uint64_t* out) {
    const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (e == 0 || e >= (1ull << log_n)) return;
    const uint32_t t = 64 - __clzll((unsigned long long)e);                   // 2^(t-1) <= e < 2^t
    const uint64_t b = e - (1ull << (t - 1));
    const uint64_t r = t > 1 ? __brevll(b) >> (64 - (t - 1)) : 0;
    store256(out + 4 * e, m_mul<F_R>(load256(tw + 4 * (r << (log_n - t))), load256(gpow + 4 * t)));
}
// Several decimation-in-time stages per pass over HBM: a workgroup takes a tile of 2^ns "rows" at stride 2^s0 times C adjacent
// columns (1024 elements, 32 KB of LDS as 8 limb planes so that lanes hit consecutive banks) through stages s0+1 .. s0+ns.  The first
// pass (s0 = 0: contiguous 1024-element blocks, ten stages) also does the bit reversal and the conversion to Montgomery form on its
// loads, the last one the conversion back (and the 1/n of the inverse) on its stores: k = 20 is three passes (10 + 5 + 5 stages)
// instead of 23 (conversion, bit reversal, 20 stages, conversion).  fr_launch fills one of these per step of the route.
struct FrPass {
    const uint64_t* in;         // first pass: the caller's data (natural order, plain integers); later passes: == out
    uint64_t* out;
    const uint64_t* tw;         // w_n^k, k < n / 2, Montgomery form
    uint32_t log_n, s0, ns;
    uint32_t first, last, use_scale;
    u256 scale;
    // coset forms (coeff_to_extended / extended_to_coeff): the first pass reads n_in <= n inputs (zero beyond) times pre[i] (Montgomery),
    // the last pass writes n_out <= n outputs times post[i] (plain integers, the 1/n included) instead of `scale`
    uint64_t n_in, n_out;
    const uint64_t* pre;
    const uint64_t* post;
    // resident form (the PLONK prover, plonk_bn254.hip): inputs already in Montgomery form / outputs left in it (post and scale are then
    // Montgomery values too)
    uint32_t in_mont, out_mont;
    // no_gather: the first pass reads element i where the classic form reads bitrev(i) -- either the input already is in bit-reversed order
    // (decimation in time then gives natural-order output without the scattered 32-byte reads: 1.05 of the 1.85 ms of a 2^23-point transform
    // went into that one pass), or `dif` is set: decimation in frequency, natural-order input, stages from the top down with the butterfly
    // (u + v, (u - v) w), bit-reversed output.  The passes of a dif transform run from the highest s0 down; `first` then marks the pass that
    // reads the input (conversion, pre-multipliers, zero padding), `last` the s0 = 0 pass.
    uint32_t no_gather, dif;
    // (every dif launch of the library passes `btw`: the per-position butterfly above is exercised by tools/ubench/ubench_fr_fft.hip alone)
    // COSET form (bn254_fr_ntt_mont_coset_dif): out[bitrev(k)] = sum_i in[i] g^i w^(ik) with NO multiplication by g^i up front and no per-position
    // twiddles.  Write a block of 2^s values as the coset transform of its own shift g': its halves u, v combine as (u + G v, u - G v) with the ONE
    // constant G = g'^(2^(s-1)) per block, and the halves are coset transforms again, with shifts g' and g' w_(2^s).  btw[2^(t-1) + b] holds the constant of
    // block b of the t-th stage from the top (fr_coset_twiddle_kernel): g^(n / 2^t) w_(2^t)^rev(b).  Stages run from the top down as for `dif`; in a pass over
    // the high stages a tile sees a handful of blocks, so its twiddle loads are broadcasts instead of 32-byte pieces of as many cache lines.
    const uint64_t* btw;
};
__global__ void __launch_bounds__(256) fr_fft_pass_kernel(FrPass a) {
    __shared__ uint32_t lds[8][1024];
    const uint32_t tile_elems = min(1024u, 1u << a.log_n), C = tile_elems >> a.ns, log_c = 31 - __clz(C);
    const uint32_t tid = threadIdx.x;
    // tiles: (hi, c_blk) with c_blk < 2^s0 / C
    const uint32_t cblks = (1u << a.s0) >> log_c;
    const uint64_t hi = blockIdx.x / cblks, c0 = (uint64_t)(blockIdx.x % cblks) << log_c;
    const uint64_t base = (hi << (a.s0 + a.ns)) + c0;
    for (uint32_t e = tid; e < tile_elems; e += 256) {
        const uint32_t r = e >> log_c, c = e & (C - 1);
        const uint64_t i = base + ((uint64_t)r << a.s0) + c;
        u256 x;
        if (a.first) {
            const uint64_t src = a.no_gather ? i : __brevll(i) >> (64 - a.log_n);
            if (src < a.n_in) {
                x = a.in_mont ? load256(a.in + 4 * src) : m_from_int<F_R>(load256(a.in + 4 * src));
                if (a.pre) x = m_mul<F_R>(x, load256(a.pre + 4 * src));
            } else x = u_zero();
        } else x = load256(a.in + 4 * i);
#pragma unroll
        for (int l = 0; l < 8; l++) lds[l][e] = x.l[l];
    }
    __syncthreads();
    // (Two stages per LDS round trip -- four rows per lane in registers -- were built and measured: the pass kernel grows from 81 to 170 VGPRs
    // (three waves per SIMD instead of six) and evaluate_h at k = 23 went from 594 to 641 ms, 744 ms capped at 128 VGPRs with spills.  One
    // stage per round trip at six waves stays.  Round 4, after the product was written by hand: the product inlined into the butterfly (no call,
    // no operand moves) and both of a thread's twiddles fetched before its first product changed nothing -- evaluate_h 452.5 and 458 against
    // 451 ms -- the pass is neither call- nor twiddle-latency-bound; it runs at 0.72 of the VALU rate of its mix.  The butterflies on nine
    // 29-bit limbs (bn254_f29.cuh: inlined product against twiddles in the 2^261 form, sums reduced on the top limb, 36 KB of LDS) were built
    // too: evaluate_h 442 against 435 ms -- the product it saves is paid back in limb planes, normalisations and a block less per CU.)
    const bool block_tw = a.btw != nullptr, dif_fly = a.dif && !block_tw;
    for (uint32_t it = 1; it <= a.ns; it++) {
        const uint32_t st = a.dif ? a.ns + 1 - it : it;
        const uint32_t s = a.s0 + st, lh = st - 1, half = 1u << lh;
        for (uint32_t b = tid; b < tile_elems / 2; b += 256) {
            const uint32_t q = b >> log_c, c = b & (C - 1);
            const uint32_t pos = q & (half - 1);
            const uint32_t r_lo = ((q >> lh) << (lh + 1)) | pos;
            const uint32_t e0 = (r_lo << log_c) | c, e1 = e0 + (half << log_c);
            const uint64_t j = ((uint64_t)pos << a.s0) + c0 + c;
            // block form: the pair's block of 2^s values is number (global index >> s) = hi 2^(ns - st) + (q >> lh)
            const u256 w = block_tw ? load256(a.btw + 4 * ((1ull << (a.log_n - s)) + (hi << (a.ns - st)) + (q >> lh)))
                                    : load256(a.tw + 4 * (j << (a.log_n - s)));
            u256 u, v;
#pragma unroll
            for (int l = 0; l < 8; l++) { u.l[l] = lds[l][e0]; v.l[l] = lds[l][e1]; }
            u256 p, m;
            if (dif_fly) { p = m_add<F_R>(u, v); m = m_mul<F_R>(m_sub<F_R>(u, v), w); }
            else { v = m_mul<F_R>(v, w); p = m_add<F_R>(u, v); m = m_sub<F_R>(u, v); }
#pragma unroll
            for (int l = 0; l < 8; l++) { lds[l][e0] = p.l[l]; lds[l][e1] = m.l[l]; }
        }
        __syncthreads();
    }
    for (uint32_t e = tid; e < tile_elems; e += 256) {
        const uint32_t r = e >> log_c, c = e & (C - 1);
        const uint64_t i = base + ((uint64_t)r << a.s0) + c;
        u256 x;
#pragma unroll
        for (int l = 0; l < 8; l++) x.l[l] = lds[l][e];
        if (a.last) {
            if (i >= a.n_out) continue;
            if (a.out_mont) {
                if (a.post) x = m_mul<F_R>(x, load256(a.post + 4 * i));
                else if (a.use_scale) x = m_mul<F_R>(x, a.scale);
            } else if (a.post) x = m_canon<F_R>(m_mul<F_R>(x, load256(a.post + 4 * i)));
            else x = a.use_scale ? m_canon<F_R>(m_mul<F_R>(x, a.scale)) : m_to_int<F_R>(x);
        }
        store256(a.out + 4 * i, x);
    }
}

static dim3 fr_blocks(uint64_t count) { return dim3((uint32_t)((count + 255) / 256)); }

// The seed of a table of `count` powers of w (Montgomery), in scratch of the context: what fr_twiddle_kernel and the fr_power_*_kernels multiply up
struct FrSeed {
    Scratch mem;
    const uint64_t* lo = nullptr;      // w^j, j < 1024
    const uint64_t* hi = nullptr;      // w^(1024 j), j < ceil(count / 1024)
    explicit FrSeed(Ctx* ctx) : mem(ctx) {}
    int32_t launch(const Fr& w, uint64_t count) {
        const uint64_t n_hi = (count + 1023) / 1024;
        GL355_TRY(mem.get((1024 + n_hi) * 32));
        uint64_t* p = mem.as<uint64_t>();
        lo = p;
        hi = p + 4 * 1024;
        hipLaunchKernelGGL(fr_twiddle_seed_kernel, fr_blocks(1024 + n_hi), dim3(256), 0, mem.ctx->stream, p, p + 4 * 1024, n_hi, to_u256(w.l));
        return GL355_OK;
    }
};
// w_n^i (Montgomery), i < n / 2, for the forward or the inverse transform of 2^log_n points: what every pass of fr_fft_pass_kernel reads.
// `tw` holds n / 2 + 1 elements.
int32_t bn254_fr_twiddles(Ctx* ctx, uint32_t log_n, bool inverse, uint64_t* tw) {
    const uint64_t count = std::max<uint64_t>(1, (1ull << log_n) / 2);
    // omega_n = ROOT^(2^(28 - log_n)), or its inverse
    const Fr w = inverse ? Fr::root_of_unity(log_n).inv() : Fr::root_of_unity(log_n);
    FrSeed seed(ctx);
    GL355_TRY(seed.launch(w, count));
    hipLaunchKernelGGL(fr_twiddle_kernel, fr_blocks(count), dim3(256), 0, ctx->stream, tw, count, seed.lo, seed.hi);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}
// tab[i] = f * base^i (Montgomery), i < count (base, f: plain integers; f = 1 for plain powers)
int32_t bn254_fr_power_table(Ctx* ctx, const uint64_t base[4], const uint64_t f[4], uint64_t count, uint64_t* tab) {
    FrSeed seed(ctx);
    GL355_TRY(seed.launch(Fr::from_words(base), count));
    // (lo hi) R * (f R) * R^-1 = lo hi f R: Montgomery again
    hipLaunchKernelGGL(fr_power_mont_kernel, fr_blocks(count), dim3(256), 0, ctx->stream, tab, count, seed.lo, seed.hi, to_u256(Fr::from_words(f).l));
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

// One transform of 2^log_n points: out[k] = post[k] (or scale) * sum_i pre[i] in[i] w^(ik), i < n_in (zero beyond), k < n_out, with the index order of
// input and output that `order` names (bn254_fr_route.h).  The entry points below fill one of these; fr_launch turns it into passes.
struct FrJob {
    FrOrder order = FR_GATHER;
    const uint64_t* in = nullptr;
    uint64_t* out = nullptr;           // may be `in`
    uint64_t* work = nullptr;          // FR_GATHER: n elements of scratch
    uint64_t n_in = 0, n_out = 0;
    uint32_t log_n = 0;
    const uint64_t* tw = nullptr;      // bn254_fr_twiddles of the direction
    const uint64_t* btw = nullptr;     // FR_DIF: the block constants of the coset (FrPass::btw)
    const uint64_t* pre = nullptr;     // Montgomery
    const uint64_t* post = nullptr;    // in the form of the output: plain integers, or Montgomery with out_mont
    bool use_scale = false;            // without post: every output times `scale`, in the form of the output too
    u256 scale = {};
    bool in_mont = false, out_mont = false;      // the data is resident in Montgomery form / stays in it
};
static int32_t fr_launch(Ctx* ctx, const FrJob& j) {
    const FrRoute r = fr_route(j.order, j.log_n, j.in == j.out);
    const uint64_t* const src[3] = {j.in, j.work, j.out};        // by FrBuf
    uint64_t* const dst[3] = {nullptr, j.work, j.out};
    const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (1ull << j.log_n) / 1024);
    for (uint32_t i = 0; i < r.n_steps; i++) {
        const FrStep& st = r.step[i];
        FrPass pa;
        memset(&pa, 0, sizeof pa);
        pa.in = src[st.src]; pa.out = dst[st.dst];
        pa.tw = j.tw; pa.btw = j.btw;
        pa.log_n = j.log_n; pa.s0 = st.s0; pa.ns = st.ns;
        pa.first = st.first; pa.last = st.last;
        pa.no_gather = r.no_gather; pa.dif = r.dif;
        pa.in_mont = j.in_mont; pa.out_mont = j.out_mont;
        // read by the first pass alone ...
        pa.n_in = j.n_in; pa.pre = j.pre;
        // ... and by the last one alone, wherever it writes
        pa.n_out = j.n_out; pa.post = j.post; pa.use_scale = j.use_scale; pa.scale = j.scale;
        hipLaunchKernelGGL(fr_fft_pass_kernel, dim3(tiles), dim3(256), 0, ctx->stream, pa);
    }
    if (r.tail_copy) GL355_HIP(ctx, hipMemcpyAsync(j.out, j.work, j.n_out * 32, hipMemcpyDeviceToDevice, ctx->stream));
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

// The resident forms of the PLONK prover (plonk_bn254.hip): n values in Montgomery form in, n out, w from `tw` (bn254_fr_twiddles: the caller picks the direction).
// Natural order in and out; every output times scale_plain if given (the 1 / n of an inverse transform).  `work`: n elements of scratch; in may equal out.
int32_t bn254_fr_ntt_mont(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t scale_plain[4] /* or null */, uint64_t* work) {
    if (log_n == 0) {
        GL355_HIP(ctx, hipMemcpyAsync(out, in, 32, hipMemcpyDeviceToDevice, ctx->stream));        // (the scale of a 1-point transform: not needed by any caller)
        return GL355_OK;
    }
    FrJob j;
    j.order = FR_GATHER; j.in = in; j.out = out; j.work = work;
    j.n_in = j.n_out = 1ull << log_n; j.log_n = log_n; j.tw = tw;
    j.in_mont = j.out_mont = true;
    if (scale_plain) { j.use_scale = true; j.scale = to_u256(Fr::from_words(scale_plain).l); }
    return fr_launch(ctx, j);
}
// The coset transform in block form, natural-order input, BIT-REVERSED output: out[bitrev(k)] = sum_i in[i] shift^i w^(ik) for i < n_in (zero beyond), with NO
// table of shift^i, no product per element up front and none of the scattered twiddle loads of the high stages (FrPass::btw).  `btw`: n elements,
// filled here for this shift (one product per entry: 0.1 ms at 2^23) -- callers transform many columns per shift and pass fill = false after the first.
int32_t bn254_fr_ntt_mont_coset_dif(Ctx* ctx, const uint64_t* in, uint64_t n_in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t shift_plain[4],
                                    uint64_t* btw, bool fill) {
    const uint64_t n = 1ull << log_n;
    if (log_n == 0) {
        GL355_HIP(ctx, hipMemcpyAsync(out, in, 32, hipMemcpyDeviceToDevice, ctx->stream));
        return GL355_OK;
    }
    if (fill) {
        // gpow[t] = shift^(n / 2^t), t = 1 .. log_n (Montgomery): repeated squaring from the bottom
        std::vector<u256> gp(log_n + 1);
        memset(gp.data(), 0, gp.size() * sizeof(u256));
        Fr g = Fr::from_words(shift_plain);
        for (uint32_t t = log_n; t >= 1; t--) {
            gp[t] = to_u256(g.l);
            g = g * g;
        }
        Scratch d(ctx);
        GL355_TRY(d.get(gp.size() * 32));
        GL355_HIP(ctx, hipMemcpyAsync(d.p, gp.data(), gp.size() * 32, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(fr_coset_twiddle_kernel, fr_blocks(n), dim3(256), 0, ctx->stream, tw, d.as<uint64_t>(), log_n, btw);
        GL355_HIP(ctx, hipGetLastError());
        GL355_HIP(ctx, ctx->wait());                                     // gp is pageable host memory
    }
    FrJob j;
    j.order = FR_DIF; j.in = in; j.out = out;
    j.n_in = n_in; j.n_out = n; j.log_n = log_n; j.tw = tw; j.btw = btw;
    j.in_mont = j.out_mont = true;
    return fr_launch(ctx, j);
}
// Bit-reversed input (what bn254_fr_ntt_mont_coset_dif leaves) to natural-order output, no gather either: out[k] = post[k] * sum_i in[bitrev(i)] w^(ik).
// Every pass reads and writes the same positions of its tile, so in may equal out.
int32_t bn254_fr_ntt_mont_from_bitrev(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, const uint64_t* tw, const uint64_t* post) {
    FrJob j;
    j.order = FR_FROM_BITREV; j.in = in; j.out = out;
    j.n_in = j.n_out = 1ull << log_n; j.log_n = log_n; j.tw = tw; j.post = post;
    j.in_mont = j.out_mont = true;
    return fr_launch(ctx, j);
}

// The public forms on plain integers.  in: 2^log_in values, out: n_out values of the 2^log_n-point transform (log_n >= 1), natural order; shift == nullptr: the
// plain transform.  in may equal out.
int32_t fr_ntt_run(Ctx* ctx, const uint64_t* in, uint32_t log_in, uint64_t* out, uint64_t n_out, uint32_t log_n, int32_t inverse, const uint64_t* shift) {
    const uint64_t n = 1ull << log_n, n_in = 1ull << log_in;
    FrJob j;
    j.order = FR_GATHER; j.in = in; j.out = out;
    j.n_in = n_in; j.n_out = n_out; j.log_n = log_n;
    uint64_t scale_w[4] = {1, 0, 0, 0};
    if (inverse) Fr::from_u64(n).inv().to_words(scale_w);                    // n^-1 mod r, plain
    j.use_scale = inverse != 0;
    j.scale = to_u256(scale_w);
    // coset: powers of the shift multiply the inputs of the forward form, powers of its inverse (and 1/n) the outputs of the inverse form
    Fr sh = Fr::zero();
    if (shift) {
        sh = Fr::from_words(shift);
        if (sh.is_zero()) return ctx->fail(GL355_E_INVALID_ARG, "bn254_fr_coset_ntt: the shift must not be zero");
        if (inverse) sh = sh.inv();
    }
    const uint64_t n_pow = shift ? (inverse ? n_out : n_in) : 0;
    Scratch tw(ctx), work(ctx), pw(ctx);
    GL355_TRY(tw.get((n / 2 + 1) * 32));
    GL355_TRY(work.get(n * 32));                             // the first pass reads the data bit-reversed: it cannot run in place
    if (n_pow) GL355_TRY(pw.get(n_pow * 32));
    j.tw = tw.as<uint64_t>(); j.work = work.as<uint64_t>();
    ProfScope ps(ctx, "bn254_fr_ntt", (n_in + n_out) * 32);
    GL355_TRY(bn254_fr_twiddles(ctx, log_n, inverse != 0, tw.as<uint64_t>()));
    if (n_pow) {
        FrSeed seed(ctx);
        GL355_TRY(seed.launch(sh, n_pow));
        if (inverse) {
            hipLaunchKernelGGL(fr_power_plain_kernel, fr_blocks(n_pow), dim3(256), 0, ctx->stream, pw.as<uint64_t>(), n_pow, seed.lo, seed.hi, j.scale);
            j.post = pw.as<uint64_t>();
        } else {
            hipLaunchKernelGGL(fr_twiddle_kernel, fr_blocks(n_pow), dim3(256), 0, ctx->stream, pw.as<uint64_t>(), n_pow, seed.lo, seed.hi);
            j.pre = pw.as<uint64_t>();
        }
    }
    return fr_launch(ctx, j);
}
}  // namespace gl355

using namespace gl355;

extern "C" {

int32_t gl355_bn254_fr_ntt(gl355_ctx* h, uint64_t* data, uint32_t log_n, int32_t inverse) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!data) return ctx->fail(GL355_E_INVALID_ARG, "bn254_fr_ntt: null data");
    if (log_n > 26) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_fr_ntt: log_n > 26 unsupported (Fr has 2-adicity 28)");
    const uint64_t n = 1ull << log_n;
    if (log_n == 0) return GL355_OK;
    Staged sd(ctx);
    GL355_TRY(sd.open(data, n * 32, 3));
    GL355_TRY(fr_ntt_run(ctx, sd.as<uint64_t>(), log_n, sd.as<uint64_t>(), n, log_n, inverse, nullptr));
    return sd.finish();
}

int32_t gl355_bn254_fr_coset_ntt(gl355_ctx* h, const uint64_t* in, uint32_t log_small, uint32_t log_n, const uint64_t shift[4], int32_t inverse,
                                 uint64_t* out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!in || !out || !shift) return ctx->fail(GL355_E_INVALID_ARG, "bn254_fr_coset_ntt: null argument");
    if (in == out) return ctx->fail(GL355_E_INVALID_ARG, "bn254_fr_coset_ntt: in and out must differ");
    if (log_n > 26 || log_small > log_n) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_fr_coset_ntt: needs log_small <= log_n <= 26");
    if (log_n == 0) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_fr_coset_ntt: log_n == 0");
    const uint64_t n = 1ull << log_n, ns = 1ull << log_small;
    // forward: 2^log_small coefficients -> 2^log_n evaluations on shift * <omega_n>; inverse: 2^log_n evaluations -> 2^log_small coefficients
    const uint64_t n_in = inverse ? n : ns, n_out = inverse ? ns : n;
    Staged si(ctx), so(ctx);
    GL355_TRY(si.open(in, n_in * 32, 1));
    GL355_TRY(so.open(out, n_out * 32, 2));
    GL355_TRY(fr_ntt_run(ctx, si.as<uint64_t>(), inverse ? log_n : log_small, so.as<uint64_t>(), n_out, log_n, inverse, shift));
    return so.finish();
}

}  // extern "C"
