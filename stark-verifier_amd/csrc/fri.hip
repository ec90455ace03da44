// Openings, DEEP quotient, FRI fold / layer commit, query openings and the FRI tail for gfx950 (a1, a11, a12, a14 of SURVEY.md 8).
// Every stage exists once, with a unit dimension B: the lock-step prover (prover_batch.hip) calls the *_units_dev routines and
// fri_tail_units, and the staged surface of the C ABI (interleaved F_p^2 data, any list of (oracle, column)) is their B = 1 call.
// The two kernels that read polynomials take where to find them as a template parameter (PolySet / PolyTable, gl355_internal.h).
//
// Replaces PolynomialBatch::prove_openings (ReducingFactor::reduce_polys_base,
// PolynomialCoeffs::divide_by_linear, shift_poly), OpeningSet::new's polynomial evaluations,
// and fri_committed_trees' reduce_with_powers fold,
// all reached from the reference through CircuitData::prove (src/plonky2_semaphore/access_set.rs:94,
// recursion.rs:168, wrapper.rs:55).  Formulas pinned by the reference's verifier:
// chip/fri_chip.rs:112-149 (batch combine), :168-226 (arity-2 fold), types/fri.rs:50-73 (batches).
//
// These are streaming kernels: every polynomial coefficient is read exactly once, lane k handles
// coefficient k so each wave reads 512 contiguous bytes per column.
#include "gl355_internal.h"

namespace gl355 {

// ---- a1: element-wise field ops (test / utility surface) -------------------------------------
__global__ void field_batch_kernel(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (op) {
        case GL355_OP_ADD: out[i] = gl_canon(gl_add(a[i], b[i])); break;
        case GL355_OP_SUB: out[i] = gl_canon(gl_sub(a[i], b[i])); break;
        case GL355_OP_MUL: out[i] = gl_canon(gl_mul(a[i], b[i])); break;
        case GL355_OP_INV: out[i] = gl_canon(gl_inv(a[i])); break;
        case GL355_OP_EXT_MUL: {
            gl2 r = gl2_canon(gl2_mul(gl2_make(a[2 * i], a[2 * i + 1]), gl2_make(b[2 * i], b[2 * i + 1])));
            out[2 * i] = r.c0; out[2 * i + 1] = r.c1;
        } break;
        case GL355_OP_EXT_INV: {
            gl2 r = gl2_canon(gl2_inv(gl2_make(a[2 * i], a[2 * i + 1])));
            out[2 * i] = r.c0; out[2 * i + 1] = r.c1;
        } break;
    }
}
int32_t field_batch_dev(Ctx* ctx, int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    if (n == 0) return GL355_OK;
    hipLaunchKernelGGL(field_batch_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, a, b, out, n);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

__global__ void canon_kernel(uint64_t* a, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i < n) a[i] = gl_canon(a[i]);
}
int32_t canon_dev(Ctx* ctx, uint64_t* a, uint64_t n) {
    if (n == 0) return GL355_OK;
    hipLaunchKernelGGL(canon_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, a, n);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

// ---- ext <-> two base columns (the F_p^2 LDE is two base-field LDEs; the unit kernels below work on columns) ---------------
__global__ void ext_split_kernel(const uint64_t* ext, uint64_t n, uint64_t* c0, uint64_t* c1) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(ext + 2 * k);
    c0[k] = v.x; c1[k] = v.y;
}
__global__ void ext_join_kernel(const uint64_t* c0, const uint64_t* c1, uint64_t n, uint64_t* ext) {
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (k >= n) return;
    *reinterpret_cast<ulonglong2*>(ext + 2 * k) = make_ulonglong2(c0[k], c1[k]);
}
int32_t ext_split_dev(Ctx* ctx, const uint64_t* ext, uint64_t n, uint64_t* c0, uint64_t* c1) {
    ProfScope ps(ctx, "ext_split_join", n * 32);
    hipLaunchKernelGGL(ext_split_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, ext, n, c0, c1);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}
int32_t ext_join_dev(Ctx* ctx, const uint64_t* c0, const uint64_t* c1, uint64_t n, uint64_t* ext) {
    ProfScope ps(ctx, "ext_split_join", n * 32);
    hipLaunchKernelGGL(ext_join_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, c0, c1, n, ext);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}
int32_t lde_ext_dev(Ctx* ctx, const uint64_t* coeffs, uint32_t log_n, uint32_t rate_bits, uint64_t shift, uint64_t* out,
                    bool out_bitrev) {
    const uint64_t n = 1ull << log_n, N = n << rate_bits;
    Scratch sc(ctx);
    GL355_TRY(sc.get((2 * n + 2 * N) * 8));
    uint64_t* cols = sc.as<uint64_t>();
    uint64_t* res = cols + 2 * n;
    GL355_TRY(ext_split_dev(ctx, coeffs, n, cols, cols + n));
    GL355_TRY(lde_dev(ctx, cols, n, log_n, rate_bits, shift, 2, res, N, out_bitrev));
    return ext_join_dev(ctx, res, res + N, N, out);
}

// ---- openings: p_i(z) for base-field coefficient columns, z in F_p^2 ---------------------------------------------------------
// OpeningSet::new: block (i, u) evaluates polynomial i of unit u at zeta_u (i < n_all) or Z polynomial i - n_all at g * zeta_u;
// lane t Horner-evaluates the coefficients k = t (mod 256) in z^256 (coalesced loads) and scales by z^t; the partials are summed in LDS.  out[u][i] (extension)
template <class Polys>
__global__ void __launch_bounds__(256) eval_polys_units_kernel(EvalArgs<Polys> a) {
    __shared__ uint64_t sh[512];
    const int tid = threadIdx.x;
    const uint32_t u = blockIdx.y, i = blockIdx.x;
    const bool at_next = i >= a.n_all;
    const uint64_t* p = at_next ? a.zs.ptr(u, i - a.n_all) : a.all.ptr(u, i);
    const gl2 zz = at_next ? gl2_make(a.zeta.v[u * 4 + 2], a.zeta.v[u * 4 + 3]) : gl2_make(a.zeta.v[u * 4], a.zeta.v[u * 4 + 1]);
    const uint64_t n = 1ull << a.all.log_n;
    const gl2 acc = gl2_horner_strided256(p, n, zz, (uint32_t)tid);
    sh[2 * tid] = acc.c0; sh[2 * tid + 1] = acc.c1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sh[2 * tid] = gl_add(sh[2 * tid], sh[2 * (tid + s)]);
            sh[2 * tid + 1] = gl_add(sh[2 * tid + 1], sh[2 * (tid + s) + 1]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint64_t* o = a.out + (uint64_t)u * a.out_us + 2ull * i;
        o[0] = gl_canon(sh[0]); o[1] = gl_canon(sh[1]);
    }
}
template <class Polys>
int32_t eval_polys_units_dev(Ctx* ctx, uint32_t B, uint32_t n_zs, const EvalArgs<Polys>& a) {
    ProfScope ps(ctx, "eval_polys", (uint64_t)B * ((uint64_t)(a.n_all + n_zs) << a.all.log_n) * 8);
    hipLaunchKernelGGL(eval_polys_units_kernel<Polys>, dim3(a.n_all + n_zs, B), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}
template int32_t eval_polys_units_dev<PolySet>(Ctx*, uint32_t, uint32_t, const EvalArgs<PolySet>&);

// ---- a11: DEEP quotient --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) deep_tables_kernel(DeepTabArgs a) {
    const uint32_t u = blockIdx.x;
    uint64_t* t = a.tab + (uint64_t)u * deep_tab_len(a.n_alpha) * 2;
    const gl2 al = gl2_make(a.alpha.v[u * 4], a.alpha.v[u * 4 + 1]);
    for (uint32_t i = threadIdx.x; i <= a.n_alpha; i += blockDim.x) {
        const gl2 c = gl2_canon(gl2_pow(al, i));
        t[2 * i] = c.c0; t[2 * i + 1] = c.c1;
    }
    for (int pt = 0; pt < 2; pt++) {
        const gl2 z = gl2_make(a.zeta.v[u * 4 + 2 * pt], a.zeta.v[u * 4 + 2 * pt + 1]);
        uint64_t* tz = t + 2 * ((uint64_t)(a.n_alpha + 1) + (uint64_t)pt * (8 + DEEP_BLK + 1));
        for (uint32_t i = threadIdx.x; i < 8 + DEEP_BLK + 1; i += blockDim.x) {
            const gl2 c = gl2_canon(i < 8 ? gl2_pow(z, 1ull << i) : gl2_pow(z, i - 8));
            tz[2 * i] = c.c0; tz[2 * i + 1] = c.c1;
        }
    }
}
int32_t deep_tables_dev(Ctx* ctx, uint32_t B, const DeepTabArgs& a) {
    hipLaunchKernelGGL(deep_tables_kernel, dim3(B), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}
GL_DEV const uint64_t* deep_tab_u(const DeepArgs& a, uint32_t u) { return a.tab + (uint64_t)u * deep_tab_len(a.n_alpha) * 2; }
// phase 1: comp[k] = sum_i alpha^i p_i[k]; in-block suffix Horner sums v[k] = sum_{j>=k, j in block} comp[j] z^(j-k) by a log-step
// scan with multipliers z^(2^s); block totals to `totals`
template <class Polys>
__global__ void __launch_bounds__(DEEP_BLK) deep_reduce_scan_units_kernel(DeepScanArgs<Polys> sa) {
    const DeepArgs& a = sa.a;
    __shared__ uint64_t sh[2 * DEEP_BLK];
    const int tid = threadIdx.x;
    const uint32_t u = blockIdx.y;
    const uint64_t k = blockIdx.x * (uint64_t)DEEP_BLK + tid;
    const uint64_t* tab = deep_tab_u(a, u);
    const uint64_t* z_pow2 = tab + 2 * ((uint64_t)(a.n_alpha + 1) + (uint64_t)a.point * (8 + DEEP_BLK + 1));
    gl2 c = gl2_make(0, 0);
    if (k < a.n) {
        for (uint32_t i = 0; i < a.n_polys; i++) {
            const uint64_t coef = sa.polys.ptr(u, i)[k];
            c.c0 = gl_add(c.c0, gl_mul(tab[2 * i], coef));
            c.c1 = gl_add(c.c1, gl_mul(tab[2 * i + 1], coef));
        }
    }
    sh[2 * tid] = c.c0; sh[2 * tid + 1] = c.c1;
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 8; s++) {
        const int other = tid + (1 << s);
        gl2 add = gl2_make(0, 0);
        if (other < DEEP_BLK) add = gl2_mul(gl2_make(sh[2 * other], sh[2 * other + 1]), gl2_make(z_pow2[2 * s], z_pow2[2 * s + 1]));
        __syncthreads();
        c = gl2_add(c, add);
        sh[2 * tid] = c.c0; sh[2 * tid + 1] = c.c1;
        __syncthreads();
    }
    uint64_t* v = a.v + (uint64_t)u * a.n * 2;
    if (k < a.n) { v[2 * k] = c.c0; v[2 * k + 1] = c.c1; }
    if (tid == 0) { uint64_t* t = a.totals + ((uint64_t)u * a.n_blocks + blockIdx.x) * 2; t[0] = c.c0; t[1] = c.c1; }
}
// phase 2 (one lane per unit): carry[blk] = T_{blk+1} + z^B carry[blk+1]
__global__ void deep_carry_units_kernel(DeepArgs a) {
    const uint32_t u = blockIdx.x;
    if (threadIdx.x != 0) return;
    const uint64_t* tab = deep_tab_u(a, u);
    const uint64_t* z_pows = tab + 2 * ((uint64_t)(a.n_alpha + 1) + (uint64_t)a.point * (8 + DEEP_BLK + 1) + 8);
    const gl2 zb = gl2_make(z_pows[2 * DEEP_BLK], z_pows[2 * DEEP_BLK + 1]);
    const uint64_t* totals = a.totals + (uint64_t)u * a.n_blocks * 2;
    uint64_t* carry = a.carry + (uint64_t)u * a.n_blocks * 2;
    gl2 c = gl2_make(0, 0);
    for (uint64_t blk = a.n_blocks; blk-- > 0;) {
        carry[2 * blk] = c.c0; carry[2 * blk + 1] = c.c1;
        c = gl2_add(gl2_make(totals[2 * blk], totals[2 * blk + 1]), gl2_mul(zb, c));
    }
}
// phase 3: quotient q_k = b_{k+1}, b_j = v[j] + z^(B - j%B) carry[blk(j)]; acc = acc * alpha^n_polys + q
__global__ void __launch_bounds__(DEEP_BLK) deep_finish_units_kernel(DeepArgs a) {
    const uint64_t k = blockIdx.x * (uint64_t)DEEP_BLK + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t u = blockIdx.y;
    const uint64_t* tab = deep_tab_u(a, u);
    const uint64_t* z_pows = tab + 2 * ((uint64_t)(a.n_alpha + 1) + (uint64_t)a.point * (8 + DEEP_BLK + 1) + 8);
    const uint64_t* v = a.v + (uint64_t)u * a.n * 2;
    const uint64_t* carry = a.carry + (uint64_t)u * a.n_blocks * 2;
    gl2 q = gl2_make(0, 0);
    const uint64_t j = k + 1;
    if (j < a.n) {
        const uint64_t blk = j / DEEP_BLK, off = j % DEEP_BLK;
        const gl2 cr = gl2_make(carry[2 * blk], carry[2 * blk + 1]);
        const uint64_t e = DEEP_BLK - off;
        q = gl2_add(gl2_make(v[2 * j], v[2 * j + 1]), gl2_mul(gl2_make(z_pows[2 * e], z_pows[2 * e + 1]), cr));
    }
    uint64_t* acc0 = a.acc + (uint64_t)u * 2 * a.n;
    uint64_t* acc1 = acc0 + a.n;
    const gl2 shift = gl2_make(tab[2 * a.n_polys], tab[2 * a.n_polys + 1]);
    const gl2 r = gl2_canon(gl2_add(gl2_mul(gl2_make(acc0[k], acc1[k]), shift), q));
    acc0[k] = r.c0; acc1[k] = r.c1;
}
template <class Polys>
int32_t deep_units_dev(Ctx* ctx, uint32_t B, const Polys& polys, const DeepArgs& a) {
    ProfScope ps(ctx, "deep_batch", (uint64_t)B * ((uint64_t)a.n_polys * a.n * 8 + a.n * 32));   // every coefficient once + acc in/out
    hipLaunchKernelGGL(deep_reduce_scan_units_kernel<Polys>, dim3((uint32_t)a.n_blocks, B), dim3(DEEP_BLK), 0, ctx->stream, DeepScanArgs<Polys>{polys, a});
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(deep_carry_units_kernel, dim3(B), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(deep_finish_units_kernel, dim3((uint32_t)a.n_blocks, B), dim3(DEEP_BLK), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}
template int32_t deep_units_dev<PolySet>(Ctx*, uint32_t, const PolySet&, const DeepArgs&);

// ---- a12: FRI commit phase -----------------------------------------------------------------------------------------------------
// layer leaves from the bit-reversed F_p^2 evaluations held as two base columns per unit: the interleaved sequence (c0[e], c1[e]),
// written a pair of values at a time.  A layer that folds by A takes A consecutive values as one leaf (fri_chip.rs:275-316 for
// A = 2: leaf i = (c0[2i], c1[2i], c0[2i+1], c1[2i+1])), so this one buffer is the row-major leaf array [len / A][2A] of every arity
__global__ void fri_leaves_units_kernel(const uint64_t* cols /* [B][2][len] */, uint64_t len, uint64_t* leaves /* [B][len/2][4] */) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= len / 2) return;
    const uint32_t u = blockIdx.y;
    const uint64_t* c0 = cols + (uint64_t)u * 2 * len;
    const uint64_t* c1 = c0 + len;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(c0 + 2 * i);
    const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(c1 + 2 * i);
    uint64_t* dst = leaves + ((uint64_t)u * (len / 2) + i) * 4;
    *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(a.x, b.x);
    *reinterpret_cast<ulonglong2*>(dst + 2) = make_ulonglong2(a.y, b.y);
}
// fold of the coefficient columns by A = 2^AB: out[k] = sum_{j<A} beta_u^j c[A k + j], one lane per output.  The lane's A coefficients
// of each base column are 8 A contiguous bytes (16-byte loads); Horner from the top in the lazy gl2 forms, canonical on the way out.
// <1> is c[2k] + beta_u * c[2k+1]
template <int AB>
__global__ void fri_fold_units_kernel(const uint64_t* cols /* [B][2][len] */, uint64_t len, UnitVals beta, uint64_t* out /* [B][2][len >> AB] */) {
    constexpr int H = 1 << (AB - 1);      // pairs of coefficients per column
    const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t n_out = len >> AB;
    if (k >= n_out) return;
    const uint32_t u = blockIdx.y;
    const uint64_t* c0 = cols + (uint64_t)u * 2 * len;
    const uint64_t* c1 = c0 + len;
    ulonglong2 a[H], b[H];
#pragma unroll
    for (int j = 0; j < H; j++) {
        a[j] = *reinterpret_cast<const ulonglong2*>(c0 + 2 * (H * k + j));
        b[j] = *reinterpret_cast<const ulonglong2*>(c1 + 2 * (H * k + j));
    }
    const gl2 bt = gl2_make(beta.v[u * 4], beta.v[u * 4 + 1]);
    gl2 acc = gl2_make(a[H - 1].y, b[H - 1].y);
    acc = gl2_add(gl2_make(a[H - 1].x, b[H - 1].x), gl2_mul(acc, bt));
#pragma unroll
    for (int j = H - 2; j >= 0; j--) {
        acc = gl2_add(gl2_make(a[j].y, b[j].y), gl2_mul(acc, bt));
        acc = gl2_add(gl2_make(a[j].x, b[j].x), gl2_mul(acc, bt));
    }
    const gl2 r = gl2_canon(acc);
    uint64_t* o0 = out + (uint64_t)u * 2 * n_out;
    o0[k] = r.c0; o0[n_out + k] = r.c1;
}
int32_t fri_fold_units_dev(Ctx* ctx, uint32_t arity_bits, uint32_t B, const uint64_t* cols, uint64_t len, const UnitVals& betas, uint64_t* out) {
    const uint64_t n_out = len >> arity_bits;
    ProfScope ps(ctx, "fri_fold", (uint64_t)B * (len * 16 + n_out * 16));
    const dim3 grid((uint32_t)((n_out + 255) / 256), B), block(256);
    switch (arity_bits) {
        case 1: hipLaunchKernelGGL(fri_fold_units_kernel<1>, grid, block, 0, ctx->stream, cols, len, betas, out); break;
        case 2: hipLaunchKernelGGL(fri_fold_units_kernel<2>, grid, block, 0, ctx->stream, cols, len, betas, out); break;
        case 3: hipLaunchKernelGGL(fri_fold_units_kernel<3>, grid, block, 0, ctx->stream, cols, len, betas, out); break;
        case 4: hipLaunchKernelGGL(fri_fold_units_kernel<4>, grid, block, 0, ctx->stream, cols, len, betas, out); break;
        default: return ctx->fail(GL355_E_UNSUPPORTED, "fri_fold: 1..4 arity bits");
    }
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}

// ---- a14: query openings ---------------------------------------------------------------------------------------------------------
// block (q, u): row idx[u][q] of unit u's column-major LDE (+ salt segment) and its Merkle path (siblings leaf -> cap, MerkleTree::prove's
// index walk), dense per-unit outputs: one launch and one copy back per oracle for all queries instead of (1 + depth) tiny copies per query
__global__ void open_units_kernel(OpenArgs a) {
    const uint32_t q = blockIdx.x, u = blockIdx.y;
    const uint64_t index = a.idx[(uint64_t)u * a.n_idx + q];
    const uint32_t layers = a.lde_bits - a.cap_height;
    const uint64_t* lde = a.o.lde + (uint64_t)u * a.o.lde_us;
    const uint64_t* salt = a.o.salt ? a.o.salt + (uint64_t)u * a.o.salt_us : nullptr;
    uint64_t* lo = a.leaves + ((uint64_t)u * a.n_idx + q) * a.o.leaf_len;
    for (uint32_t c = threadIdx.x; c < a.o.leaf_len; c += blockDim.x)
        lo[c] = c < a.o.batch ? lde[(uint64_t)c * a.N + index] : salt[(uint64_t)(c - a.o.batch) * a.N + index];
    const uint64_t sub_leaves = 1ull << layers;
    const uint64_t* tree = a.o.digests + (uint64_t)u * a.o.dig_us + (index >> layers) * 2 * (sub_leaves - 1) * 4;
    const uint64_t k0 = index & (sub_leaves - 1);
    uint64_t* so = a.sibs + ((uint64_t)u * a.n_idx + q) * layers * 4;
    for (uint32_t e = threadIdx.x; e < layers * 4; e += blockDim.x) {
        const uint32_t layer = e >> 2;
        const uint64_t k = (k0 >> layer) ^ 1;
        so[e] = tree[digest_slot(layer, k) * 4 + (e & 3)];
    }
}
int32_t open_units_dev(Ctx* ctx, uint32_t B, const OpenArgs& a) {
    ProfScope ps(ctx, "open_batch", (uint64_t)B * a.n_idx * (a.o.leaf_len * 16 + (a.lde_bits - a.cap_height) * 64));
    hipLaunchKernelGGL(open_units_kernel, dim3(a.n_idx, B), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}
// block (q, u, l): the leaf of layer l at index idx[u][q] >> s_l (its 2^a_l evaluations) and its path
struct OpenFriArgs {
    const uint64_t* trees; uint64_t leaf_off[32], dig_off[32];     // layer l: leaves [B][nl][2 A_l] at leaf_off, digests [B][2(nl - cap)][4] at dig_off
    FriLayers lay;
    uint32_t lde_bits, cap_height, n_idx;
    const uint64_t* idx; uint64_t* evals /* [B][n_idx][lay.ev_total] */; uint64_t* sibs /* [B][n_idx][lay.sib_total] */;
};
__global__ void open_fri_units_kernel(OpenFriArgs a) {
    const uint32_t q = blockIdx.x, u = blockIdx.y, l = blockIdx.z;
    const uint64_t index = a.idx[(uint64_t)u * a.n_idx + q] >> a.lay.s[l];
    const uint32_t log_nl = a.lde_bits - a.lay.s[l], layers = a.lay.depth[l], lw = 2u << a.lay.a[l];
    const uint64_t nl = 1ull << log_nl, n_cap = 1ull << a.cap_height;
    const uint64_t* leaves = a.trees + a.leaf_off[l] + (uint64_t)u * nl * lw;
    const uint64_t* digs = a.trees + a.dig_off[l] + (uint64_t)u * 2 * (nl - n_cap) * 4;
    uint64_t* ev = a.evals + ((uint64_t)u * a.n_idx + q) * a.lay.ev_total + a.lay.ev_off[l];
    if (threadIdx.x < lw) ev[threadIdx.x] = leaves[index * lw + threadIdx.x];      // lw <= 32 < blockDim.x
    const uint64_t sub_leaves = 1ull << layers;
    const uint64_t* tree = digs + (index >> layers) * 2 * (sub_leaves - 1) * 4;
    const uint64_t k0 = index & (sub_leaves - 1);
    uint64_t* so = a.sibs + ((uint64_t)u * a.n_idx + q) * a.lay.sib_total + a.lay.sib_off[l];
    for (uint32_t e = threadIdx.x; e < layers * 4; e += blockDim.x) {
        const uint32_t layer = e >> 2;
        const uint64_t k = (k0 >> layer) ^ 1;
        so[e] = tree[digest_slot(layer, k) * 4 + (e & 3)];
    }
}

// ---- the FRI tail (fri_committed_trees, final polynomial, fri_proof_of_work, query indices, layer openings): gl355_internal.h ----------
int32_t fri_tail_units(Ctx* ctx, const FriShape& s, uint32_t B, uint64_t* cols, uint64_t* cols2, uint64_t* vals, uint64_t* stage,
                       gl355_challenger* ch, const FriUnitOut* out, uint64_t* q_idx, uint64_t* d_idx, uint64_t* d_evals, uint64_t* d_sibs) {
    const FriLayers& fl = s.layers;
    const uint32_t L = fl.n, lde_bits = s.log_n + s.rate_bits;
    const uint64_t N = 1ull << lde_bits, n_cap = 1ull << s.cap_height;
    if (fl.total_bits > s.log_n) return ctx->fail(GL355_E_INVALID_ARG, "fri: the layers fold more than the polynomial has coefficients");
    OpenFriArgs fa;         // the layer trees: leaves [B][nl][2 A_l] and digests [B][2(nl - n_cap)][4] of layer l, one after the other
    memset(&fa, 0, sizeof fa);
    uint64_t tree_words = 0;
    for (uint32_t l = 0; l < L; l++) {
        const uint64_t nl = N >> fl.s[l];
        if (nl < n_cap) return ctx->fail(GL355_E_INVALID_ARG, "fri: layer smaller than the cap");
        fa.leaf_off[l] = tree_words; tree_words += (uint64_t)B * (N >> (fl.s[l] - fl.a[l])) * 2;
        fa.dig_off[l] = tree_words; tree_words += (uint64_t)B * 2 * (nl - n_cap) * 4;
    }
    Scratch trees(ctx);
    GL355_TRY(trees.get((tree_words + (uint64_t)B * n_cap * 4 + 16) * 8));
    uint64_t* tree_buf = trees.as<uint64_t>();
    uint64_t* d_cap = tree_buf + tree_words;
    uint64_t shift = GL355_COSET_SHIFT, len_c = 1ull << s.log_n;
    for (uint32_t l = 0; l < L; l++) {
        const uint32_t ab = fl.a[l];
        const uint64_t len_v = len_c << s.rate_bits, nl = len_v >> ab;
        GL355_TRY(lde_dev(ctx, cols, len_c, log2_u64(len_c), s.rate_bits, gl_canon(shift), 2 * B, vals, len_v, true));
        uint64_t* lv = tree_buf + fa.leaf_off[l];
        // leaves of 8, 16 or 32 words, few enough to leave the chip short of waves at one lane per leaf (1, 2 or 4 dependent permutations per
        // lane): 16 lanes per leaf, read from the value columns, the leaf array written on the way (merkle.hip); GL355_OPT_LEAF_LANES_LOG
        if (ab >= 2 && s.hasher == GL355_HASH_POSEIDON && ctx->leaf_lanes_log && (uint64_t)B * nl < (1ull << ctx->leaf_lanes_log)) {
            GL355_TRY(fri_wide_leaves_tree_dev(ctx, ab, B, vals, len_v, lv, log2_u64(nl) - s.cap_height, tree_buf + fa.dig_off[l], d_cap));
        } else {
            {
                ProfScope ps(ctx, "fri_layer_leaves", (uint64_t)B * len_v * 32);
                hipLaunchKernelGGL(fri_leaves_units_kernel, dim3((uint32_t)((len_v / 2 + 255) / 256), B), dim3(256), 0, ctx->stream, vals, len_v, lv);
                LAUNCH_CHECK(ctx);
            }
            LeafArgs la;
            memset(&la, 0, sizeof la);
            la.leaves = lv; la.n_leaves = (uint64_t)B * nl; la.leaf_len = 2u << ab; la.col_major = 0; la.stride = 2u << ab;
            GL355_TRY(merkle_build_args(ctx, s.hasher, la, log2_u64(nl) - s.cap_height, tree_buf + fa.dig_off[l], d_cap));
        }
        uint64_t* cap_dst[MAXB];
        for (uint32_t u = 0; u < B; u++) cap_dst[u] = out[u].caps + (uint64_t)l * n_cap * 4;
        GL355_TRY(observe_caps_units(ctx, B, n_cap, d_cap, stage, ch, cap_dst));
        UnitVals beta;
        memset(&beta, 0, sizeof beta);
        for (uint32_t u = 0; u < B; u++) squeeze_ext(&ch[u], &beta.v[u * 4]);
        GL355_TRY(fri_fold_units_dev(ctx, ab, B, cols, len_c, beta, cols2));
        std::swap(cols, cols2);
        len_c >>= ab;
        for (uint32_t j = 0; j < ab; j++) shift = gl_mul(shift, shift);
    }
    // final polynomial: len_c = n >> total_bits extension coefficients per unit, two columns each
    GL355_HIP(ctx, ctx->d2h(stage, cols, (uint64_t)B * 2 * len_c * 8));
    GL355_HIP(ctx, ctx->wait());
    uint64_t pow_state[MAXB * 12];
    uint32_t pow_pos[MAXB];
    uint64_t* p_pow[MAXB];
    for (uint32_t u = 0; u < B; u++) {
        const uint64_t* c0 = stage + (uint64_t)u * 2 * len_c;
        uint64_t* fp = out[u].final_poly;
        for (uint64_t k = 0; k < len_c; k++) { fp[2 * k] = c0[k]; fp[2 * k + 1] = c0[len_c + k]; }
        gl355_challenger_observe(&ch[u], fp, 2 * len_c);
        if (gl355_challenger_pow_state(&ch[u], &pow_state[u * 12], &pow_pos[u]) != GL355_OK) return ctx->fail(GL355_E_INVALID_ARG, "fri: challenger state");
        for (int k = 0; k < 12; k++) pow_state[u * 12 + k] = gl_canon(pow_state[u * 12 + k]);
        p_pow[u] = out[u].pow_witness;
    }
    // proof of work: the smallest witness of every unit
    GL355_TRY(pow_grind_units_dev(ctx, s.hasher, B, pow_state, pow_pos, s.pow_bits, 0, stage, p_pow));
    // queries: x_index = challenge mod N; layer l opens the leaf at x_index >> s_l and its path
    for (uint32_t u = 0; u < B; u++) {
        gl355_challenger_observe(&ch[u], p_pow[u], 1);
        uint64_t resp;
        gl355_challenger_squeeze(&ch[u], &resp, 1);
        if (s.pow_bits && (resp >> (64 - s.pow_bits)) != 0) return ctx->fail(GL355_E_HIP, "fri: proof-of-work response check failed");
        uint64_t* qi = q_idx + (uint64_t)u * s.n_queries;
        gl355_challenger_squeeze(&ch[u], qi, s.n_queries);
        for (uint32_t q = 0; q < s.n_queries; q++) qi[q] &= (N - 1);
    }
    GL355_HIP(ctx, hipMemcpyAsync(d_idx, q_idx, (uint64_t)B * s.n_queries * 8, hipMemcpyHostToDevice, ctx->stream));
    if (L) {
        fa.trees = tree_buf;
        fa.lay = fl;
        fa.lde_bits = lde_bits; fa.cap_height = s.cap_height; fa.n_idx = s.n_queries; fa.idx = d_idx;
        fa.evals = d_evals; fa.sibs = d_sibs;
        ProfScope ps(ctx, "open_batch", (uint64_t)B * s.n_queries * (fl.ev_total * 16 + fl.sib_total * 16));
        hipLaunchKernelGGL(open_fri_units_kernel, dim3(s.n_queries, B, L), dim3(64), 0, ctx->stream, fa);
        LAUNCH_CHECK(ctx);
    }
    return GL355_OK;
}

// ---- the staged forms: one unit, interleaved F_p^2, challenges in any representation -----------------------------------------------
// two canonical words of an extension element in words [0, 1] of unit 0, everything else zero
static UnitVals unit0_ext(const uint64_t x[2]) {
    UnitVals v;
    memset(&v, 0, sizeof v);
    v.v[0] = gl_canon(x[0]); v.v[1] = gl_canon(x[1]);
    return v;
}
// the polynomials' addresses as a PolyTable in `sc`, `extra_bytes` of work space behind it (*extra).  Waits: the host table must outlive the copy
static int32_t upload_poly_table(Ctx* ctx, Scratch& sc, const uint64_t* const* poly_ptrs_host, uint32_t n_polys, uint32_t log_n, size_t extra_bytes,
                                 PolyTable* table, uint64_t** extra) {
    const size_t ptr_bytes = (sizeof(uint64_t*) * n_polys + 15) & ~(size_t)15;
    GL355_TRY(sc.get(ptr_bytes + extra_bytes));
    GL355_HIP(ctx, hipMemcpyAsync(sc.p, poly_ptrs_host, sizeof(uint64_t*) * n_polys, hipMemcpyHostToDevice, ctx->stream));
    GL355_HIP(ctx, ctx->wait());
    *table = PolyTable{sc.as<const uint64_t*>(), log_n};
    *extra = reinterpret_cast<uint64_t*>(sc.as<char>() + ptr_bytes);
    return GL355_OK;
}

int32_t eval_polys_ext_dev(Ctx* ctx, const uint64_t* const* poly_ptrs_host, uint32_t n_polys, uint32_t log_n,
                           const uint64_t z[2], uint64_t* out_dev) {
    if (n_polys == 0) return GL355_OK;      // a grid of no blocks is a launch error
    Scratch sc(ctx);
    EvalArgs<PolyTable> ea;
    uint64_t* unused;
    GL355_TRY(upload_poly_table(ctx, sc, poly_ptrs_host, n_polys, log_n, 0, &ea.all, &unused));
    ea.zs = PolyTable{nullptr, log_n};      // no polynomial is evaluated at the second point
    ea.n_all = n_polys; ea.zeta = unit0_ext(z); ea.out = out_dev; ea.out_us = 0;
    return eval_polys_units_dev(ctx, 1, 0, ea);
}

int32_t deep_batch_dev(Ctx* ctx, const uint64_t* const* poly_ptrs_host, uint32_t n_polys, uint32_t log_n,
                       const uint64_t alpha[2], const uint64_t z[2], uint64_t* acc) {
    const uint64_t n = 1ull << log_n;
    const uint64_t n_blocks = (n + DEEP_BLK - 1) / DEEP_BLK;
    const uint64_t tab_words = (uint64_t)deep_tab_len(n_polys) * 2;
    Scratch sc(ctx);
    PolyTable polys;
    uint64_t* work;      // tables | acc as two columns | v, totals, carry
    GL355_TRY(upload_poly_table(ctx, sc, poly_ptrs_host, n_polys, log_n, (tab_words + 2 * n + 2 * n + 4 * n_blocks + 8) * 8, &polys, &work));
    DeepTabArgs ta;
    ta.tab = work; ta.n_alpha = n_polys; ta.alpha = unit0_ext(alpha); ta.zeta = unit0_ext(z);      // one point: the tables of point 0
    GL355_TRY(deep_tables_dev(ctx, 1, ta));
    DeepArgs da;
    memset(&da, 0, sizeof da);
    da.n_polys = n_polys; da.n_alpha = n_polys; da.point = 0; da.tab = work; da.n = n; da.n_blocks = n_blocks;
    da.acc = work + tab_words; da.v = da.acc + 2 * n; da.totals = da.v + 2 * n; da.carry = da.totals + 2 * n_blocks;
    GL355_TRY(ext_split_dev(ctx, acc, n, da.acc, da.acc + n));
    GL355_TRY(deep_units_dev(ctx, 1, polys, da));
    return ext_join_dev(ctx, da.acc, da.acc + n, n, acc);
}

int32_t fri_fold_dev(Ctx* ctx, const uint64_t* coeffs, uint64_t n, uint32_t arity_bits, const uint64_t beta[2], uint64_t* out) {
    const uint64_t n_out = n >> arity_bits;
    if (n_out == 0) return GL355_OK;
    Scratch sc(ctx);
    GL355_TRY(sc.get((2 * n + 2 * n_out) * 8));
    uint64_t* cols = sc.as<uint64_t>();
    uint64_t* folded = cols + 2 * n;
    GL355_TRY(ext_split_dev(ctx, coeffs, n, cols, cols + n));
    GL355_TRY(fri_fold_units_dev(ctx, arity_bits, 1, cols, n, unit0_ext(beta), folded));
    return ext_join_dev(ctx, folded, folded + n_out, n_out, out);
}

// leaves[i] = (v[br(2i)], v[br(2i+1)]) -- i.e. ext element j of the bit-reversed sequence, from natural-order interleaved values
__global__ void fri_layer_leaves_kernel(const uint64_t* values, uint32_t log_n, uint64_t* leaves) {
    const uint64_t n = 1ull << log_n;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = log_n ? (__brevll(i) >> (64 - log_n)) : 0;
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(values + 2 * j);
    *reinterpret_cast<ulonglong2*>(leaves + 2 * i) = make_ulonglong2(gl_canon(v.x), gl_canon(v.y));
}
int32_t fri_layer_leaves_dev(Ctx* ctx, const uint64_t* values, uint64_t n, uint64_t* leaves) {
    if (n == 0) return GL355_OK;
    ProfScope ps(ctx, "fri_layer_leaves", n * 32);
    hipLaunchKernelGGL(fri_layer_leaves_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, values,
                       log2_u64(n), leaves);
    GL355_HIP(ctx, hipGetLastError());
    return GL355_OK;
}

}  // namespace gl355
