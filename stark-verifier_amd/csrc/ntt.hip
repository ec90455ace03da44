// Batched radix-2 Goldilocks NTT / inverse NTT / coset NTT / LDE for gfx950 (a2, a3, a5 of SURVEY.md 8).
//
// Replaces plonky2_field::fft::{fft_with_options, ifft_with_options}, PolynomialCoeffs::{lde,
// coset_fft_with_options}, PolynomialValues::{ifft, coset_ifft} and plonky2_util::{transpose,
// reverse_index_bits_in_place}, reached from the reference inside CircuitBuilder::build /
// CircuitData::prove (src/plonky2_semaphore/access_set.rs:91,94; recursion.rs:167-168).
// Conventions pinned by the reference's verifier: omega_N = 7^((p-1)/N) (chip/fri_chip.rs:162-163),
// coset generator 7 (chip/plonk/plonk_verifier_chip.rs:225-227), bit-reversed evaluation order
// (chip/fri_chip.rs:245-264).
//
// Design (MI355X-first, not plonky2's layer-by-layer loop):
//   * one workgroup owns a TILE of 2^LT elements (LT = 12..14) held in LDS (160 KiB/CU);
//     each thread keeps 16 elements in VGPRs and runs radix-16 decimation-in-frequency rounds
//     (4 butterfly layers per LDS round-trip), so a 2^12 tile needs 3 LDS exchanges, not 12;
//   * sizes up to 2^14 are ONE pass over HBM; larger sizes use the 4-step split N = N1*N2:
//     a "column" pass (tiles of N1 rows x TC adjacent columns, every global access a full
//     TC*8-byte segment) and a "row" pass (contiguous rows), each a single read + single write;
//   * DIF produces bit-reversed order for free, which is exactly the Merkle-leaf order the FRI
//     commit wants, so the commit path never runs a separate permutation or transpose;
//   * coset scaling, the 1/n of the inverse transform and the 4-step twiddles are fused into the
//     load / store of the passes (two-level power tables: g^e = lo[e & 4095] * hi[e >> 12]);
//   * the LDE runs the 2^rate_bits cosets as independent size-n transforms (the first rate_bits
//     layers of the zero-padded size-N transform are trivial); coset c's output is the contiguous
//     block bitrev(c) of the bit-reversed result, and workgroup id % n_cosets selects the coset so
//     that with 8 cosets each XCD's L2 keeps exactly one coset's power table.
// Which kernels run for a transform is decided in ONE place, ntt_route (ntt_route.h, pure host code): it turns the shape of a plan into at most
// four steps -- kernel instance, tables, flags, profile scope -- and ntt_run below only executes them.  The instances that exist are listed once, in
// that header; this unit compiles the radix-16 forms of the list, ntt_r8.hip the radix-8 forms, ntt_l24.hip the 24-bit-limb forms, each with its own
// field product.  tests/ntt_route_check.cpp prints the route of every shape the callers in capi.hip can build and tests/test_ntt_route_host.py
// holds every listed instance to be reached by one of them (docs/history/ntt_route.md has the table).
// Field products: the compiler-scheduled formulation (gl_field.cuh, GL_MUL_VARIANT 2).  These kernels run 2-4 waves per SIMD
// between LDS exchanges, so what matters is that the 16 independent butterflies of a thread interleave freely; the
// inline-asm formulation has fewer instructions but serialises each product (measured: 4-7 % slower single-pass tiles).
#ifndef GL_MUL_VARIANT
#define GL_MUL_VARIANT 2
#endif
#include "gl355_internal.h"
#include "ntt_kernels.cuh"

namespace gl355 {

// out[c][i] = in[c][bitrev(i)] over 2^log_n entries of `width` u64 each (a5:
// reverse_index_bits_in_place; out-of-place, or in place via swap when in == out).
__global__ void bitrev_permute_kernel(const uint64_t* in, uint64_t* out, uint32_t log_n, uint32_t width,
                                      uint64_t in_col_stride, uint64_t out_col_stride, uint32_t batch) {
    const uint64_t n = 1ull << log_n;
    const uint64_t total = n * batch;
    for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < total;
         g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t col = g >> log_n, i = g & (n - 1);
        const uint64_t j = brev((uint32_t)i, log_n);
        if (in == out) {
            if (i < j) {
                for (uint32_t w = 0; w < width; w++) {
                    uint64_t* pa = out + col * out_col_stride + i * width + w;
                    uint64_t* pb = out + col * out_col_stride + j * width + w;
                    uint64_t ta = *pa, tb = *pb;
                    *pa = tb; *pb = ta;
                }
            }
        } else {
            for (uint32_t w = 0; w < width; w++)
                out[col * out_col_stride + i * width + w] = in[col * in_col_stride + j * width + w];
        }
    }
}

// The same permutation for width == 1 and log_n >= 10 at HBM speed: index i = (a | m | b) with 5-bit a, b maps to
// (rev b | rev m | rev a), so for a fixed middle part m the 32 x 32 block over (a, b) is read as 32 contiguous 256-byte rows,
// transposed (with both coordinates bit-reversed) through LDS, and written as 32 contiguous rows of block rev(m).  In place,
// block m and block rev(m) are exchanged by one workgroup (the one with m <= rev m).  The element-wise kernel above scatters
// 8-byte accesses and takes longer than the transform it follows (3.7 ms vs 2.8 ms at 2^20 x 135).
// (64 x 64 tiles -- 512-byte rows on both sides, 66 KB of LDS per block -- measured twice as slow: 1.33 vs 0.61 ms at 2^20 x 135.)
__global__ void __launch_bounds__(256) bitrev_tiled_kernel(const uint64_t* in, uint64_t* out, uint32_t log_n, uint64_t in_col_stride,
                                                         uint64_t out_col_stride) {
    __shared__ uint64_t t0[32][33], t1[32][33];
    const uint32_t mid_bits = log_n - 10;
    // Block order (round 5): a tile's 32 rows are 2^(log_n - 5) words apart -- 1 MB at 2^22 points -- so a block touches 32 pages on the read side
    // and 32 on the write side, and with m = blockIdx the write side of neighbouring blocks (rev m) is scattered over the whole column: 1.8 TB/s at
    // 2^22, 1.7 at 2^23 against 2.5 at 2^21.  256 consecutive blocks now take every combination of the LOW four and the HIGH four bits of m: their
    // reads (low bits vary) and their writes (rev of the high bits varies) both fall into 32 runs of 4 KB.
    uint32_t m = blockIdx.x;
    if (mid_bits >= 8) m = ((m >> 4 & 15u) << (mid_bits - 4)) | ((m >> 8) << 4) | (m & 15u);
    const uint32_t rm = brev(m, mid_bits);
    const bool in_place = in == out;
    if (in_place && m > rm) return;
    const uint64_t col = blockIdx.y;
    const uint64_t* src = in + col * in_col_stride;
    uint64_t* dst = out + col * out_col_stride;
    const uint32_t x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    const uint32_t hi_shift = log_n - 5;
    const bool both = in_place && m != rm;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t a = y0 + 8 * k;
        t0[a][x] = src[((uint64_t)a << hi_shift) | ((uint64_t)m << 5) | x];
        if (both) t1[a][x] = src[((uint64_t)a << hi_shift) | ((uint64_t)rm << 5) | x];
    }
    __syncthreads();
    const uint32_t rx = brev(x, 5);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t bp = y0 + 8 * k;                 // output row = rev(b), output column x = rev(a)
        dst[((uint64_t)bp << hi_shift) | ((uint64_t)rm << 5) | x] = t0[rx][brev(bp, 5)];
        if (both) dst[((uint64_t)bp << hi_shift) | ((uint64_t)m << 5) | x] = t1[rx][brev(bp, 5)];
    }
}

// out[r][c] = in[c][perm(r)] : column-major [cols][rows] -> row-major [rows][cols], optionally
// reading row bitrev(r) (a5: transpose; used to export plonky2-layout leaves).  32x32 LDS tiles.
__global__ void transpose_kernel(const uint64_t* in, uint64_t* out, uint64_t rows, uint32_t cols,
                                 uint64_t in_col_stride, uint32_t out_row_stride, uint32_t log_rows_brev) {
    __shared__ uint64_t tile[32][33];
    const uint64_t r0 = (uint64_t)blockIdx.x * 32;
    const uint32_t c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const uint32_t c = c0 + k;
        const uint64_t r = r0 + tx;
        if (c < cols && r < rows) {
            const uint64_t rr = log_rows_brev ? brev((uint32_t)r, log_rows_brev) : r;
            tile[k][tx] = in[(uint64_t)c * in_col_stride + rr];
        }
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const uint64_t r = r0 + k;
        const uint32_t c = c0 + tx;
        if (c < cols && r < rows) out[r * out_row_stride + c] = tile[tx][k];
    }
}

// full-size multiplier tables (built once per (bases, size), cached on the context): they trade one
// modmul + one gather per element for a coalesced 8-byte read that stays L2-resident per XCD
__global__ void build_pow_table_kernel(const uint64_t* lo, const uint64_t* hi, uint32_t n_cosets, uint64_t n, uint64_t* out) {
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (g >= n * n_cosets) return;
    const uint64_t c = g / n, i = g % n;
    out[g] = gl_canon(gl_mul(lo[c * 4096 + (i & 4095)], hi[c * 4096 + (i >> 12)]));
}
// step_full[r * N2 + i2] = omega^(bitrev(r, l1) * i2): the 4-step twiddle in the column pass's store order
__global__ void build_step_table_kernel(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, uint64_t* out) {
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (g >= (1ull << (l1 + l2))) return;
    const uint64_t r = g >> l2, i2 = g & ((1ull << l2) - 1);
    const uint64_t e = (uint64_t)brev((uint32_t)r, l1) * i2;
    out[g] = gl_canon(gl_mul(lo[e & 4095], hi[e >> 12]));
}

// step_t[i2 * N1 + k1] = omega^(k1 * i2): the 4-step twiddles in the store order of pass A of the natural -> natural flow
__global__ void build_nat_step_table_kernel(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, uint64_t* out) {
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (g >= (1ull << (l1 + l2))) return;
    const uint64_t i2 = g >> l1, k1 = g & ((1ull << l1) - 1);
    const uint64_t e = k1 * i2;
    out[g] = gl_canon(gl_mul(lo[e & 4095], hi[e >> 12]));
}

// n = 1: the transform of a single point is that point, in every direction and on every coset (g^0 = 1, 1/n = 1).  What is left of the
// contract is the canonical output: one word per column, at the column stride, nothing between the columns touched.
__global__ void canon_points_kernel(const uint64_t* in, uint64_t* out, uint64_t in_col_stride, uint64_t out_col_stride, uint32_t batch) {
    const uint64_t col = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (col < batch) out[col * out_col_stride] = gl_canon(in[col * in_col_stride]);
}

// ------------------------------------------------------------------------------------------------
// host side: ntt_run executes the route that ntt_route (ntt_route.h) gives for the plan's shape
// ------------------------------------------------------------------------------------------------
// the radix-16 forms and the single points; (4 waves per SIMD measured no better for rows: HISTORY rounds 2-3)
static hipError_t launch_step_r16(const NttStep& st, const PassArgs& a, hipStream_t s) {
    switch (st.form) {
        case NTT_POINTS: {
            const NttGrid g = ntt_step_grid(st, a.batch, a.n_cosets);
            hipLaunchKernelGGL(canon_points_kernel, dim3((uint32_t)g.x), dim3(256), 0, s, a.in, a.out, a.in_col_stride, a.out_col_stride, a.batch);
            return hipGetLastError();
        }
        case NTT_ROWS16:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_rows_kernel<LT, LOG_T, INV>, st, 1 << (LT - 4), tile_lds_bytes(LT), a, s);
            GL355_NTT_ROWS16_INSTANCES(GL355_X)
#undef GL355_X
            break;
        case NTT_COLS16:
#define GL355_X(LT, LOG_T, PRE, INV, PASS) \
    if (GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS)) return launch_pass(ntt_cols_kernel<LOG_T, INV>, st, 256, tile_lds_bytes(LT), a, s);
            GL355_NTT_COLS16_INSTANCES(GL355_X)
#undef GL355_X
            break;
        default: break;
    }
    return hipErrorInvalidValue;     // not reached: ntt_route lets no step through whose instance is not listed
}

static hipError_t launch_step(const NttStep& st, const PassArgs& a, hipStream_t s) {
    switch (st.form) {
        case NTT_POINTS: case NTT_ROWS16: case NTT_COLS16: return launch_step_r16(st, a, s);
        case NTT_ROWS_L24: case NTT_COLS_L24_COSETS: case NTT_COLS_SMALL_COSETS: return launch_step_l24(st, a, s);
        default: return launch_step_r8(st, a, s);
    }
}

int32_t ntt_run(Ctx* ctx, const NttPlan& p) {
    if (p.log_n == 0 && p.batch == 0) return GL355_OK;
    const uint64_t n = 1ull << (p.log_n & 63);
    NttShape sh;
    sh.log_n = p.log_n; sh.n_cosets = p.n_cosets;
    sh.inverse = p.inverse; sh.in_bitrev = p.in_bitrev; sh.out_bitrev = p.out_bitrev;
    sh.pre = p.pre_lo != nullptr; sh.post = p.post_lo != nullptr; sh.scale = p.scale != 1; sh.ratio = p.coset_ratio != 0;
    sh.out_contig = p.out_col_stride == n; sh.cosets_contig = p.coset_out_stride == n; sh.slot0_zero = p.coset_slot[0] == 0;
    sh.batch_fits_y = p.batch <= 65535;
    sh.single_pass_max_log = ctx->ntt_single_pass_max_log;
    NttRoute route;
    const int32_t rc = ntt_route(sh, route);
    if (rc != GL355_OK) return ctx->fail(rc, route.msg);

    Scratch mid(ctx);
    const uint64_t *step_lo = nullptr, *step_hi = nullptr;
    for (uint32_t i = 0; i < route.n_steps; i++) {
        const NttStep& st = route.step[i];
        if (st.form == NTT_BITREV) {
            GL355_TRY(bitrev_permute(ctx, p.out, p.out, p.log_n, 1, p.out_col_stride, p.out_col_stride, p.batch));
            continue;
        }
        PassArgs a;
        memset(&a, 0, sizeof a);
        a.batch = p.batch << st.batch_shift;
        a.log_n = st.xform_log_n;
        a.log_rows = st.log_rows;
        a.tw = ctx->twr(4, p.inverse);
        a.tw_r8 = ctx->twr(3, p.inverse);
        a.in_bitrev = st.in_bitrev; a.out_natural = st.out_natural; a.canon = st.canon;
        a.scale = st.scale ? p.scale : 1;
        if (st.collapse_cosets) a.n_cosets = 1;               // slot 0 at offset 0: the coset blocks are rows of the column
        else {
            a.n_cosets = p.n_cosets;
            a.coset_out_stride = p.coset_out_stride;
            for (uint32_t c = 0; c < p.n_cosets; c++) a.coset_slot[c] = p.coset_slot[c];
        }
        // buffers: a pass that reads the output of a single-coset pass finds it in that coset's block
        if (st.dst == NTT_BUF_MID) GL355_TRY(mid.get(((uint64_t)p.batch << p.log_n) * 8));
        const uint64_t slot0 = a.n_cosets == 1 ? (uint64_t)a.coset_slot[0] * a.coset_out_stride : 0;
        a.in = st.src == NTT_BUF_IN ? p.in : st.src == NTT_BUF_OUT ? p.out + slot0 : mid.as<uint64_t>();
        a.out = st.dst == NTT_BUF_OUT ? p.out : mid.as<uint64_t>();
        a.in_col_stride = st.batch_shift ? 1ull << st.xform_log_n : st.src == NTT_BUF_IN ? p.in_col_stride : st.src == NTT_BUF_OUT ? p.out_col_stride : n;
        a.out_col_stride = st.batch_shift ? 1ull << st.xform_log_n : st.dst == NTT_BUF_OUT ? p.out_col_stride : n;
        // tables, each built on first use and cached on the context, in this order
        if (st.fetch_step_root) {
            const uint64_t root = gl_root_of_unity(st.xform_log_n);
            GL355_TRY(ctx->pow_tables(p.inverse ? gl_inv(root) : root, &step_lo, &step_hi));
        }
        switch (st.pre_tab) {
            case NTT_TAB_TWO_LEVEL: a.pre_hi = p.pre_hi; [[fallthrough]];
            case NTT_TAB_ONE_LEVEL: a.pre_lo = p.pre_lo; break;
            case NTT_TAB_FULL:
                GL355_TRY(ctx->full_pow_table(p.pre_lo, p.pre_hi, p.n_cosets, p.log_n, &a.pre_full));
                a.pre_full_stride = n;
                break;
            case NTT_TAB_ONE_LEVEL_AS_FULL: a.pre_full = p.pre_lo; a.pre_full_stride = 4096; break;
            default: break;
        }
        switch (st.step_tab) {
            case NTT_TAB_TWO_LEVEL: a.step_lo = step_lo; a.step_hi = step_hi; break;
            case NTT_TAB_FULL: GL355_TRY(ctx->full_step_table(step_lo, step_hi, st.log_t, st.log_rows, p.inverse, &a.step_full)); break;
            case NTT_TAB_NAT: GL355_TRY(ctx->nat_step_table(step_lo, step_hi, st.log_t, st.log_rows, &a.step_full)); break;
            default: break;
        }
        if (st.ratio_tab) {
            const uint64_t *rlo, *rhi;
            GL355_TRY(ctx->pow_tables(p.coset_ratio, &rlo, &rhi));
            GL355_TRY(ctx->full_pow_table(rlo, rhi, 1, p.log_n, &a.ratio_full));
        }
        if (st.mid_tab) GL355_TRY(ctx->l24_mid_table(&a.mid));
        if (st.post_tab != NTT_TAB_NONE) { a.post_lo = p.post_lo; a.post_hi = st.post_tab == NTT_TAB_TWO_LEVEL ? p.post_hi : nullptr; }
        ProfScope ps(ctx, st.scope, ((uint64_t)p.batch << p.log_n) * st.bytes_per_point);
        GL355_HIP(ctx, launch_step(st, a, ctx->stream));
    }
    return GL355_OK;
}


int32_t bitrev_permute(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, uint32_t width,
                       uint64_t in_col_stride, uint64_t out_col_stride, uint32_t batch) {
    const uint64_t total = ((uint64_t)batch) << log_n;
    if (total == 0) return GL355_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256 * 16);
    ProfScope ps(ctx, "bitrev_permute", total * 16);
    if (width == 1 && log_n >= 10 && batch <= 65535) {
        hipLaunchKernelGGL(bitrev_tiled_kernel, dim3(1u << (log_n - 10), batch), dim3(256), 0, ctx->stream, in, out, log_n, in_col_stride, out_col_stride);
        GL355_HIP(ctx, hipGetLastError());
        return GL355_OK;
    }
    hipLaunchKernelGGL(bitrev_permute_kernel, dim3(blocks), dim3(256), 0, ctx->stream, in, out, log_n, width,
                       in_col_stride, out_col_stride, batch);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

int32_t transpose_cols_to_rows(Ctx* ctx, const uint64_t* in, uint64_t* out, uint64_t rows, uint32_t cols,
                               uint64_t in_col_stride, uint32_t out_row_stride, uint32_t log_rows_brev) {
    if (rows == 0 || cols == 0) return GL355_OK;
    dim3 grid((uint32_t)((rows + 31) / 32), (cols + 31) / 32);
    ProfScope ps(ctx, "transpose", rows * cols * 16);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, ctx->stream, in, out, rows, cols, in_col_stride,
                       out_row_stride, log_rows_brev);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

int32_t Ctx::full_pow_table(const uint64_t* lo, const uint64_t* hi, uint32_t n_cosets, uint32_t log_n, const uint64_t** out) {
    const uint64_t total = (uint64_t)n_cosets << log_n;
    return cached_table({1, (uint64_t)(uintptr_t)lo, n_cosets, log_n}, total, out, [&](uint64_t* d) {
        hipLaunchKernelGGL(build_pow_table_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, lo, hi, n_cosets, 1ull << log_n, d);
    });
}
int32_t Ctx::full_step_table(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, bool inv, const uint64_t** out) {
    const uint64_t total = 1ull << (l1 + l2);
    return cached_table({2, l1, l2, inv ? 1ull : 0ull}, total, out, [&](uint64_t* d) {
        hipLaunchKernelGGL(build_step_table_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, lo, hi, l1, l2, d);
    });
}
int32_t Ctx::nat_step_table(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, const uint64_t** out) {
    const uint64_t total = 1ull << (l1 + l2);
    return cached_table({5, l1, l2}, total, out, [&](uint64_t* d) {
        hipLaunchKernelGGL(build_nat_step_table_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, lo, hi, l1, l2, d);
    });
}

}  // namespace gl355
