// The multi-scalar multiplication of the reference's SNARK finalisation: halo2_proofs' `best_multiexp` over halo2curves'
// bn256 G1 (y^2 = x^3 + 3 over Fq), sum_i scalars[i] * bases[i], as ParamsKZG::commit / commit_lagrange and create_proof reach it through
// `verify_inside_snark` (src/plonky2_verifier/verifier_api.rs:77-92)                                              -> gl355_bn254_g1_msm
// Checked against oracle/bn254_curve_oracle.c (itself pinned by the EIP-196 2*G vector).
//
// Pippenger's bucket method, bucket-parallel, on signed digits: per window a counting sort of the point indices by digit (in two levels with
// LDS atomics from 2^11 buckets on), one lane per bucket -- taken by decreasing size -- adding its points in XYZZ coordinates on nine 29-bit
// limbs (bn254_msm_acc.cuh), lane and workgroup items for the buckets that skewed scalars overfill, a recursion of running sums over groups of
// eight for the buckets of a window, and a Horner combination of the windows on the host.  Prepared bases (gl355_bn254_g1_msm_prepare, bn254_kzg.hip) hold
// every window's multiple of every point, so that all windows of a scalar set share one set of buckets.
#include "bn254_msm_acc.cuh"
#include <vector>

namespace gl355 {

// host_bn254_curve.cpp: sum_w 2^(c w) (S_w + Wt_w) as an affine point (canonical integers; zeros = the identity)
void bn254_g1_horner_host(const uint32_t* s, const uint32_t* wt, uint32_t n_windows, uint32_t c, uint64_t result[8]);

struct MsmArgs {
    const uint64_t* points;     // [n][8] affine x | y, canonical integers; (0, 0) = identity
    const uint64_t* scalars;    // [n][4]
    uint64_t n;
    uint32_t c, n_windows;      // window bits, windows (signed digits: |digit| <= 2^(c-1), one more window takes the last carry)
    uint32_t wps, n_sets;       // windows per scalar set, scalar sets sharing the bases (n_windows = wps * n_sets: a set's windows are just more windows)
    uint32_t cb;                // c - 1: a window has 2^cb buckets, bucket j collects the points whose digit is +-(j + 1)
    uint32_t* pm;               // [n][16] points in Montgomery form
    uint32_t* hist;             // [W][2^cb]     counts, then exclusive offsets
    uint32_t* cursor;           // [W][2^cb]     scatter cursors
    uint32_t* idx;              // [W][n]        point indices sorted by bucket, bit 31 = the digit is negative
    uint32_t* buckets;          // [W][2^cb][24] Jacobian bucket sums
    uint32_t* order;            // [W * 2^cb]    bucket ids (w << cb | j) by decreasing size
    uint32_t* size_hist;        // [MSM_SIZE_BINS] buckets per size, then the write cursor of each size class
    uint32_t* wsum;             // [W][24]       window sums
    uint64_t* result;           // [8]
    // buckets of more than MSM_BIG points (skewed scalars: selector columns of 0 / 1, constants, the sparse top window) are summed by
    // whole workgroups instead of one lane
    uint32_t* big_counters;     // [5]           work items, big buckets; of those, the items / buckets of more than MSM_MID points (workgroup path);
                                //               [4] != 0: some scalar does not fit the plan's wps signed digits of c bits (msm_digits_overflow)
    uint32_t* big_items;        // [max_items][2] bucket id, first point of the item (relative to the bucket)
    uint32_t* big_buckets;      // [max_big][3]  bucket id, first item, items
    uint32_t* big_partial;      // [max_items][24]
    uint32_t max_items, max_big;
    // two-level sort (msm_digits_kernel ... msm_fine_sort_kernel): signed digits, (index | sign, low digit bits) pairs grouped by the
    // digit's high bits, and the per-window counters of those coarse bins
    uint32_t* dig;              // [W][n]     magnitude | sign << 31; 0 = nothing to add
    uint32_t* pairs;            // [W][n][2]
    uint32_t* coarse_cnt;       // [W][2^cbits] points per coarse bin
    uint32_t* coarse_start;     // [W][2^cbits] exclusive scan of the counts
    uint32_t* coarse_fill;      // [W][2^cbits] reservation cursors of the scatter
    uint32_t cbits, chunk;      // coarse bits (cb - MSM_FINE_BITS), points per block of the coarse kernels
    uint32_t have_table;        // pm is a prepared table (gl355_bn254_g1_msm_prepare): msm_digits_kernel converts nothing
    // regions of the fine sort with more than MSM_FINE_BIG pairs (skewed scalars: runs of equal values put a window's points into one coarse bin) are
    // cut into slices of MSM_FINE_SLICE pairs, one workgroup each (msm_fine_big_* kernels)
    uint32_t* fb_counters;      // [2]            big regions, slices
    uint32_t* fb_regions;       // [max_reg][2]   region (w << cbits | bin), slices
    uint32_t* fb_items;         // [max_items][2] region, slice
    uint32_t fb_max_reg, fb_max_items;
};
#define MSM_FINE_BITS 10u
#define MSM_FINE_BIG (1u << 17)   // pairs in a (window, coarse bin) region above which it is sorted by several workgroups
#define MSM_FINE_SLICE (1u << 15)
#define MSM_UNROLL 8
#define MSM_SIZE_BINS 128
#define MSM_BIG 256u            // a lane sums at most this many points; a normal bucket holds 8-64
#define MSM_BIG_WG_POINTS 4096u // points per workgroup item of a big bucket (16 per lane), more when a bucket would need over 256 items
GL_DEV uint32_t msm_digit(const uint64_t* k, uint32_t w, uint32_t c) {
    const uint32_t bit = w * c;
    if (bit >= 256) return 0;
    const uint32_t limb = bit >> 6, off = bit & 63;
    uint64_t v = k[limb] >> off;
    if (off + c > 64 && limb + 1 < 4) v |= k[limb + 1] << (64 - off);
    return (uint32_t)(v & ((1ull << c) - 1));
}
// signed digit of window w given the carry out of the windows below: magnitude (0 = nothing to add) and sign; raw digits of
// 2^(c-1) and more become negative and carry one into the next window, which halves the buckets of a window
GL_DEV uint32_t msm_signed_digit(const uint64_t* k, uint32_t w, uint32_t c, uint32_t& carry, bool& neg) {
    const uint32_t raw = msm_digit(k, w, c) + carry;
    neg = raw >= (1u << (c - 1));
    carry = neg ? 1u : 0u;
    return neg ? (1u << c) - raw : raw;
}
// counter[key] += 1 for every lane with `active`, returning the value before the lane's increment.  Lanes of a wave that share one of
// up to three sampled keys are combined into one atomic: with skewed scalars (all equal, 0 / 1, the sparse top window) half a million
// points hit ONE counter, and one-by-one atomics on it took 6 ms per pass; uniformly random keys cost three ballots more.
GL_DEV uint32_t msm_wave_inc(uint32_t* counter, uint32_t key, bool active) {
    uint32_t slot = 0;
    bool done = !active;
    uint64_t tried = 0;
    const uint32_t lane = __lane_id();
#pragma unroll
    for (int it = 0; it < 3; it++) {
        const uint64_t cand = __ballot(!done) & ~tried;
        if (!cand) break;                                          // wave-uniform
        const int leader = __ffsll((unsigned long long)cand) - 1;
        tried |= 1ull << leader;
        const uint32_t lk = __shfl(key, leader);
        const uint64_t same = __ballot(!done && key == lk);
        const uint32_t cnt = (uint32_t)__popcll(same);
        if (cnt < 4) continue;                                     // not worth a round trip: leave them to the plain atomics
        uint32_t b = 0;
        if (lane == (uint32_t)leader) b = atomicAdd(counter + lk, cnt);
        b = __shfl(b, leader);
        if (!done && key == lk) { slot = b + (uint32_t)__popcll(same & ((1ull << lane) - 1)); done = true; }
    }
    if (!done) slot = atomicAdd(counter + key, 1u);
    return slot;
}
// what wps signed digits of c bits cannot hold: the carry out of the last window, or scalar bits at and above wps * c.  A plan cut to the caller's
// max_bits (msm_plan) silently dropped both; with max_bits = 256 neither exists (wps * c > 256, and the top window's 256 mod c < c - 1 bits never carry)
GL_DEV bool msm_digits_overflow(const uint64_t* k, uint32_t bit, uint32_t carry) {
    if (bit >= 256) return carry != 0;
    const uint32_t limb = bit >> 6;
    uint64_t v = k[limb] >> (bit & 63);
    for (uint32_t l = limb + 1; l < 4; l++) v |= k[l];
    return (v | carry) != 0;
}
__global__ void msm_prepare_kernel(MsmArgs a) {          // points to Montgomery form + digit histograms
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    bool live = i < a.n;                                  // every lane stays for the wave-level combining below
    const uint64_t ii = live ? i : 0;
    const u256 x = load256(a.points + 8 * ii), y = load256(a.points + 8 * ii + 4);
    const bool ident = u_is_zero(x) && u_is_zero(y);
    if (live) {
        const u256 xm = ident ? u_zero() : msm_table_form(m_from_int<F_Q>(x)), ym = ident ? u_zero() : msm_table_form(m_from_int<F_Q>(y));
        uint32_t* d = a.pm + 16 * i;
#pragma unroll
        for (int j = 0; j < 8; j++) { d[j] = xm.l[j]; d[8 + j] = ym.l[j]; }
    }
    live = live && !ident;
    for (uint32_t set = 0; set < a.n_sets; set++) {
        const uint64_t* k = a.scalars + 4 * ((uint64_t)set * a.n + ii);
        uint32_t carry = 0;
        for (uint32_t w = 0; w < a.wps; w++) {
            bool neg;
            const uint32_t mag = msm_signed_digit(k, w, a.c, carry, neg);
            (void)msm_wave_inc(a.hist + ((uint64_t)(set * a.wps + w) << a.cb), mag ? mag - 1 : 0, live && mag != 0);
        }
        if (live && msm_digits_overflow(k, a.wps * a.c, carry)) atomicOr(a.big_counters + 4, 1u);      // (the identity's scalar does not count)
    }
}
// per window: exclusive scan of the 2^cb counts (one workgroup), offsets copied to the cursors
__global__ void __launch_bounds__(1024) msm_scan_kernel(MsmArgs a) {
    __shared__ uint32_t sh[1024];
    const uint32_t w = blockIdx.x, nb = 1u << a.cb, tid = threadIdx.x;
    uint32_t* h = a.hist + ((uint64_t)w << a.cb);
    uint32_t* cur = a.cursor + ((uint64_t)w << a.cb);
    const uint32_t per = (nb + 1023) / 1024, lo = tid * per, hi = min(nb, lo + per);
    uint32_t s = 0;
    for (uint32_t b = lo; b < hi; b++) s += h[b];
    sh[tid] = s;
    __syncthreads();
    for (int st = 1; st < 1024; st <<= 1) {
        const uint32_t o = tid >= (uint32_t)st ? sh[tid - st] : 0;
        __syncthreads();
        sh[tid] += o;
        __syncthreads();
    }
    uint32_t run = tid ? sh[tid - 1] : 0;
    for (uint32_t b = lo; b < hi; b++) {
        const uint32_t cnt = h[b];
        h[b] = run; cur[b] = run;
        run += cnt;
    }
}
__global__ void msm_scatter_kernel(MsmArgs a) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    bool live = i < a.n;
    const uint64_t ii = live ? i : 0;
    const uint32_t* d = a.pm + 16 * ii;
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) o |= d[j];
    live = live && o != 0;                                // the identity contributes nothing
    for (uint32_t set = 0; set < a.n_sets; set++) {
        const uint64_t* k = a.scalars + 4 * ((uint64_t)set * a.n + ii);
        uint32_t carry = 0;
        for (uint32_t ww = 0; ww < a.wps; ww++) {
            bool neg;
            const uint32_t mag = msm_signed_digit(k, ww, a.c, carry, neg), w = set * a.wps + ww;
            const bool act = live && mag != 0;
            const uint32_t pos = msm_wave_inc(a.cursor + ((uint64_t)w << a.cb), mag ? mag - 1 : 0, act);
            if (act) a.idx[(uint64_t)w * a.n + pos] = (uint32_t)i | (neg ? 0x80000000u : 0u);
        }
    }
}
// ---- the sort in two levels (round 3).  The histogram and the scatter above pay one DEVICE-scope atomic per point and window each
// (2 x 109 M at 2^23 points: 4.0 + 6.0 of 36.6 ms -- the L2s of the eight XCDs are not coherent, so those atomics execute at the memory
// side).  Here the digits are written once (msm_digits_kernel), blocks of `chunk` points count and scatter them by part of the digit's bits
// with LDS atomics and one global atomic per (block, coarse bin), and one workgroup per (window, coarse bin) sorts its region by the other
// MSM_FINE_BITS bits in LDS, writing the bucket offsets (hist / cursor) and the final index array.  The coarse bin is the digit's LOW bits:
// the top window of a 254-bit scalar has only a few significant bits, and binned by the high bits its 2^23 points fell into 8 regions of
// a million points each, one workgroup per region (5 ms).  Same outputs as msm_prepare /
// msm_scan / msm_scatter up to the order of the points inside a bucket, which does not matter.  Skewed scalars only make regions large
// (a workgroup then loops over its region); nothing overflows.
__global__ void msm_digits_kernel(MsmArgs a) {            // points to Montgomery form + the signed digits of every window
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    bool ident;
    if (a.have_table) {                                       // the table's first slice IS pm; the identity is all zeros there too
        const uint4* t = reinterpret_cast<const uint4*>(a.pm + 16 * i);
        const uint4 t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
        ident = (t0.x | t0.y | t0.z | t0.w | t1.x | t1.y | t1.z | t1.w | t2.x | t2.y | t2.z | t2.w | t3.x | t3.y | t3.z | t3.w) == 0;
    } else {
        const u256 x = load256(a.points + 8 * i), y = load256(a.points + 8 * i + 4);
        ident = u_is_zero(x) && u_is_zero(y);
        const u256 xm = ident ? u_zero() : msm_table_form(m_from_int<F_Q>(x)), ym = ident ? u_zero() : msm_table_form(m_from_int<F_Q>(y));
        uint32_t* d = a.pm + 16 * i;
#pragma unroll
        for (int j = 0; j < 8; j++) { d[j] = xm.l[j]; d[8 + j] = ym.l[j]; }
    }
    for (uint32_t set = 0; set < a.n_sets; set++) {
        const uint64_t* k = a.scalars + 4 * ((uint64_t)set * a.n + i);
        uint32_t carry = 0;
        for (uint32_t w = 0; w < a.wps; w++) {
            bool neg;
            const uint32_t mag = msm_signed_digit(k, w, a.c, carry, neg);
            a.dig[(uint64_t)(set * a.wps + w) * a.n + i] = ident ? 0u : (mag | (neg && mag ? 0x80000000u : 0u));
        }
        if (!ident && msm_digits_overflow(k, a.wps * a.c, carry)) atomicOr(a.big_counters + 4, 1u);
    }
}
__global__ void __launch_bounds__(256) msm_coarse_count_kernel(MsmArgs a) {
    extern __shared__ uint32_t lh[];
    const uint32_t w = blockIdx.y, nbin = 1u << a.cbits;
    const uint64_t lo = (uint64_t)blockIdx.x * a.chunk, hi = min(a.n, lo + a.chunk);
    for (uint32_t b = threadIdx.x; b < nbin; b += 256) lh[b] = 0;
    __syncthreads();
    const uint32_t* dg = a.dig + (uint64_t)w * a.n;
    // (MSM_UNROLL loads in flight per thread: with one load per iteration these loops were chains of 64 dependent memory round trips)
    for (uint64_t i0 = lo + threadIdx.x; i0 < hi; i0 += 256 * MSM_UNROLL) {
        uint32_t d[MSM_UNROLL];
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) { const uint64_t i = i0 + 256ull * k; d[k] = i < hi ? dg[i] : 0u; }
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) {
            const uint32_t mag = d[k] & 0x7fffffffu;
            if (mag) atomicAdd(&lh[(mag - 1) & (nbin - 1)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbin; b += 256)
        if (lh[b]) atomicAdd(a.coarse_cnt + (uint64_t)w * nbin + b, lh[b]);
}
__global__ void __launch_bounds__(1024) msm_coarse_scan_kernel(MsmArgs a) {     // per window: exclusive scan of the coarse counts
    __shared__ uint32_t sh[1024];
    const uint32_t w = blockIdx.x, nbin = 1u << a.cbits, tid = threadIdx.x;
    const uint32_t* c = a.coarse_cnt + (uint64_t)w * nbin;
    uint32_t* st = a.coarse_start + (uint64_t)w * nbin;
    const uint32_t per = (nbin + 1023) / 1024, lo = min(nbin, tid * per), hi = min(nbin, lo + per);
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += c[b];
    sh[tid] = sum;
    __syncthreads();
    for (int stp = 1; stp < 1024; stp <<= 1) {
        const uint32_t o = tid >= (uint32_t)stp ? sh[tid - stp] : 0;
        __syncthreads();
        sh[tid] += o;
        __syncthreads();
    }
    uint32_t run = tid ? sh[tid - 1] : 0;
    for (uint32_t b = lo; b < hi; b++) { st[b] = run; run += c[b]; }
}
__global__ void __launch_bounds__(256) msm_coarse_scatter_kernel(MsmArgs a) {
    extern __shared__ uint32_t lh[];                       // [2^cbits] counts, then running cursors; [2^cbits] bases
    const uint32_t w = blockIdx.y, nbin = 1u << a.cbits;
    uint32_t* lbase = lh + nbin;
    const uint64_t lo = (uint64_t)blockIdx.x * a.chunk, hi = min(a.n, lo + a.chunk);
    for (uint32_t b = threadIdx.x; b < nbin; b += 256) lh[b] = 0;
    __syncthreads();
    const uint32_t* dg = a.dig + (uint64_t)w * a.n;
    for (uint64_t i0 = lo + threadIdx.x; i0 < hi; i0 += 256 * MSM_UNROLL) {
        uint32_t d[MSM_UNROLL];
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) { const uint64_t i = i0 + 256ull * k; d[k] = i < hi ? dg[i] : 0u; }
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) {
            const uint32_t mag = d[k] & 0x7fffffffu;
            if (mag) atomicAdd(&lh[(mag - 1) & (nbin - 1)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbin; b += 256) {
        const uint32_t cnt = lh[b];
        lbase[b] = cnt ? a.coarse_start[(uint64_t)w * nbin + b] + atomicAdd(a.coarse_fill + (uint64_t)w * nbin + b, cnt) : 0;
        lh[b] = 0;
    }
    __syncthreads();
    uint32_t* pr = a.pairs + 2ull * (uint64_t)w * a.n;
    for (uint64_t i0 = lo + threadIdx.x; i0 < hi; i0 += 256 * MSM_UNROLL) {
        uint32_t dd[MSM_UNROLL];
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) { const uint64_t i = i0 + 256ull * k; dd[k] = i < hi ? dg[i] : 0u; }
#pragma unroll
        for (int k = 0; k < MSM_UNROLL; k++) {
            const uint32_t d = dd[k], mag = d & 0x7fffffffu;
            if (!mag) continue;
            const uint32_t bin = (mag - 1) & (nbin - 1);
            const uint32_t pos = lbase[bin] + atomicAdd(&lh[bin], 1u);
            *reinterpret_cast<uint2*>(pr + 2ull * pos) = make_uint2((uint32_t)(i0 + 256ull * k) | (d & 0x80000000u), (mag - 1) >> a.cbits);
        }
    }
}
__global__ void __launch_bounds__(256) msm_fine_sort_kernel(MsmArgs a) {
    __shared__ uint32_t fh[1u << MSM_FINE_BITS], fbase[1u << MSM_FINE_BITS], part[256];
    const uint32_t bin = blockIdx.x, w = blockIdx.y, nbin = 1u << a.cbits, tid = threadIdx.x;
    const uint32_t start = a.coarse_start[(uint64_t)w * nbin + bin], cnt = a.coarse_cnt[(uint64_t)w * nbin + bin];
    constexpr uint32_t NF = 1u << MSM_FINE_BITS, PER = NF / 256;
    if (cnt > MSM_FINE_BIG) return;                                   // msm_fine_big_* (one workgroup would walk the whole region alone)
    for (uint32_t f = tid; f < NF; f += 256) fh[f] = 0;
    __syncthreads();
    const uint32_t* pr = a.pairs + 2ull * ((uint64_t)w * a.n + start);
    for (uint32_t k0 = tid; k0 < cnt; k0 += 256 * MSM_UNROLL) {
        uint32_t f[MSM_UNROLL];
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) { const uint32_t k = k0 + 256u * j; f[j] = k < cnt ? pr[2ull * k + 1] : 0xFFFFFFFFu; }
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) if (f[j] != 0xFFFFFFFFu) atomicAdd(&fh[f[j]], 1u);
    }
    __syncthreads();
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) { c[j] = fh[tid * PER + j]; sum += c[j]; }
    part[tid] = sum;
    __syncthreads();
    for (int stp = 1; stp < 256; stp <<= 1) {
        const uint32_t o = tid >= (uint32_t)stp ? part[tid - stp] : 0;
        __syncthreads();
        part[tid] += o;
        __syncthreads();
    }
    uint32_t run = start + (tid ? part[tid - 1] : 0);
    const uint64_t bucket0 = ((uint64_t)w << a.cb) + bin;            // bucket = digit - 1 = fine << cbits | bin
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t f = tid * PER + j;
        a.hist[bucket0 + ((uint64_t)f << a.cbits)] = run; a.cursor[bucket0 + ((uint64_t)f << a.cbits)] = run + c[j];
        fbase[f] = run; fh[f] = 0;
        run += c[j];
    }
    __syncthreads();
    uint32_t* out = a.idx + (uint64_t)w * a.n;
    for (uint32_t k0 = tid; k0 < cnt; k0 += 256 * MSM_UNROLL) {
        uint2 pp[MSM_UNROLL];
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) { const uint32_t k = k0 + 256u * j; pp[j] = k < cnt ? *reinterpret_cast<const uint2*>(pr + 2ull * k) : make_uint2(0u, 0xFFFFFFFFu); }
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) if (pp[j].y != 0xFFFFFFFFu) out[fbase[pp[j].y] + atomicAdd(&fh[pp[j].y], 1u)] = pp[j].x;
    }
}
// ---- big regions of the fine sort.  A column whose values come in long runs (a grand product that stands still where its constraint is switched off, a
// constant, 0 / 1 flags) puts millions of pairs into ONE (window, coarse bin) region, and the single workgroup of msm_fine_sort_kernel walked it alone:
// 15 - 28 ms per call in a k = 23 proof against 1 - 7 for uniform columns.  Such regions are listed and cut into slices; a slice's workgroup counts its fine
// bins in LDS and adds them to the bucket counts (a.hist, zeroed by the caller), one workgroup per region turns counts into offsets, and the slices reserve
// their ranges per fine bin with one atomic each and scatter.  Same outputs as msm_fine_sort_kernel (hist = start, cursor = end of every bucket, idx).
__global__ void __launch_bounds__(256) msm_fine_big_list_kernel(MsmArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (a.n_windows << a.cbits)) return;
    const uint32_t cnt = a.coarse_cnt[r];
    if (cnt <= MSM_FINE_BIG) return;
    const uint32_t slices = (cnt + MSM_FINE_SLICE - 1) / MSM_FINE_SLICE;
    const uint32_t slot = atomicAdd(a.fb_counters, 1u), first = atomicAdd(a.fb_counters + 1, slices);
    if (slot >= a.fb_max_reg || first + slices > a.fb_max_items) return;      // cannot happen: the bounds are sums over all pairs (host side)
    a.fb_regions[2 * slot] = r; a.fb_regions[2 * slot + 1] = slices;
    for (uint32_t k = 0; k < slices; k++) { a.fb_items[2 * (first + k)] = r; a.fb_items[2 * (first + k) + 1] = k; }
}
// the fine-bin histogram of pairs [lo, hi) of a region in LDS (fh zeroed by the caller)
GL_DEV void msm_fine_slice_hist(const uint32_t* pr, uint32_t lo, uint32_t hi, uint32_t* fh) {
    for (uint32_t k0 = lo + threadIdx.x; k0 < hi; k0 += 256 * MSM_UNROLL) {
        uint32_t f[MSM_UNROLL];
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) { const uint32_t k = k0 + 256u * j; f[j] = k < hi ? pr[2ull * k + 1] : 0xFFFFFFFFu; }
#pragma unroll
        for (int j = 0; j < MSM_UNROLL; j++) if (f[j] != 0xFFFFFFFFu) atomicAdd(&fh[f[j]], 1u);
    }
}
__global__ void __launch_bounds__(256) msm_fine_big_count_kernel(MsmArgs a) {
    __shared__ uint32_t fh[1u << MSM_FINE_BITS];
    constexpr uint32_t NF = 1u << MSM_FINE_BITS;
    const uint32_t n_items = min(a.fb_counters[1], a.fb_max_items), nbin = 1u << a.cbits;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t r = a.fb_items[2 * it], sl = a.fb_items[2 * it + 1], w = r >> a.cbits, bin = r & (nbin - 1);
        const uint32_t start = a.coarse_start[r], cnt = a.coarse_cnt[r];
        const uint32_t lo = sl * MSM_FINE_SLICE, hi = min(cnt, lo + MSM_FINE_SLICE);
        for (uint32_t f = threadIdx.x; f < NF; f += 256) fh[f] = 0;
        __syncthreads();
        msm_fine_slice_hist(a.pairs + 2ull * ((uint64_t)w * a.n + start), lo, hi, fh);
        __syncthreads();
        const uint64_t bucket0 = ((uint64_t)w << a.cb) + bin;
        for (uint32_t f = threadIdx.x; f < NF; f += 256) if (fh[f]) atomicAdd(a.hist + bucket0 + ((uint64_t)f << a.cbits), fh[f]);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) msm_fine_big_scan_kernel(MsmArgs a) {      // counts -> offsets, one workgroup per big region
    __shared__ uint32_t part[256];
    constexpr uint32_t NF = 1u << MSM_FINE_BITS, PER = NF / 256;
    const uint32_t n_reg = min(a.fb_counters[0], a.fb_max_reg), nbin = 1u << a.cbits, tid = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < n_reg; q += gridDim.x) {
        const uint32_t r = a.fb_regions[2 * q], w = r >> a.cbits, bin = r & (nbin - 1);
        const uint64_t bucket0 = ((uint64_t)w << a.cb) + bin;
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) { c[j] = a.hist[bucket0 + ((uint64_t)(tid * PER + j) << a.cbits)]; sum += c[j]; }
        part[tid] = sum;
        __syncthreads();
        for (int stp = 1; stp < 256; stp <<= 1) {
            const uint32_t o = tid >= (uint32_t)stp ? part[tid - stp] : 0;
            __syncthreads();
            part[tid] += o;
            __syncthreads();
        }
        uint32_t run = a.coarse_start[r] + (tid ? part[tid - 1] : 0);
#pragma unroll
        for (uint32_t j = 0; j < PER; j++) {
            const uint64_t b = bucket0 + ((uint64_t)(tid * PER + j) << a.cbits);
            a.hist[b] = run; a.cursor[b] = run;                       // the scatter's reservations move the cursor to the bucket's end
            run += c[j];
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) msm_fine_big_scatter_kernel(MsmArgs a) {
    __shared__ uint32_t fh[1u << MSM_FINE_BITS], fbase[1u << MSM_FINE_BITS];
    constexpr uint32_t NF = 1u << MSM_FINE_BITS;
    const uint32_t n_items = min(a.fb_counters[1], a.fb_max_items), nbin = 1u << a.cbits;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t r = a.fb_items[2 * it], sl = a.fb_items[2 * it + 1], w = r >> a.cbits, bin = r & (nbin - 1);
        const uint32_t start = a.coarse_start[r], cnt = a.coarse_cnt[r];
        const uint32_t lo = sl * MSM_FINE_SLICE, hi = min(cnt, lo + MSM_FINE_SLICE);
        const uint32_t* pr = a.pairs + 2ull * ((uint64_t)w * a.n + start);
        for (uint32_t f = threadIdx.x; f < NF; f += 256) fh[f] = 0;
        __syncthreads();
        msm_fine_slice_hist(pr, lo, hi, fh);
        __syncthreads();
        const uint64_t bucket0 = ((uint64_t)w << a.cb) + bin;
        for (uint32_t f = threadIdx.x; f < NF; f += 256) {
            fbase[f] = fh[f] ? atomicAdd(a.cursor + bucket0 + ((uint64_t)f << a.cbits), fh[f]) : 0;
            fh[f] = 0;
        }
        __syncthreads();
        uint32_t* out = a.idx + (uint64_t)w * a.n;
        for (uint32_t k0 = lo + threadIdx.x; k0 < hi; k0 += 256 * MSM_UNROLL) {
            uint2 pp[MSM_UNROLL];
#pragma unroll
            for (int j = 0; j < MSM_UNROLL; j++) { const uint32_t k = k0 + 256u * j; pp[j] = k < hi ? *reinterpret_cast<const uint2*>(pr + 2ull * k) : make_uint2(0u, 0xFFFFFFFFu); }
#pragma unroll
            for (int j = 0; j < MSM_UNROLL; j++) if (pp[j].y != 0xFFFFFFFFu) out[fbase[pp[j].y] + atomicAdd(&fh[pp[j].y], 1u)] = pp[j].x;
        }
        __syncthreads();
    }
}
// Buckets by decreasing size.  A lane sums one bucket, so a wave takes as long as its largest bucket: with 2^20 points in 2^16
// buckets per window the sizes are Poisson(16) and the largest of 64 is ~27 -- 40 % of the lanes' time idle.  Sizes are small
// integers, so a counting sort (per-workgroup LDS histogram, one global atomic per class and workgroup) puts equal sizes side by side.
GL_DEV uint32_t msm_bucket_size(const MsmArgs& a, uint32_t id) {
    const uint32_t sz = a.cursor[id] - a.hist[id];                 // cursor = end of the bucket's range after the scatter
    return sz < MSM_SIZE_BINS ? sz : MSM_SIZE_BINS - 1;
}
__global__ void __launch_bounds__(256) msm_size_hist_kernel(MsmArgs a) {
    __shared__ uint32_t h[MSM_SIZE_BINS];
    if (threadIdx.x < MSM_SIZE_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x, total = a.n_windows << a.cb;
    if (id < total) atomicAdd(&h[msm_bucket_size(a, id)], 1u);
    __syncthreads();
    if (threadIdx.x < MSM_SIZE_BINS && h[threadIdx.x]) atomicAdd(a.size_hist + threadIdx.x, h[threadIdx.x]);
}
__global__ void msm_size_scan_kernel(MsmArgs a) {                   // counts -> start of each size class, largest size first
    if (threadIdx.x || blockIdx.x) return;
    uint32_t run = 0;
    for (int sz = MSM_SIZE_BINS - 1; sz >= 0; sz--) { const uint32_t cnt = a.size_hist[sz]; a.size_hist[sz] = run; run += cnt; }
}
__global__ void __launch_bounds__(256) msm_order_kernel(MsmArgs a) {
    __shared__ uint32_t h[MSM_SIZE_BINS], base[MSM_SIZE_BINS];
    if (threadIdx.x < MSM_SIZE_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x, total = a.n_windows << a.cb;
    uint32_t sz = 0, slot = 0;
    if (id < total) { sz = msm_bucket_size(a, id); slot = atomicAdd(&h[sz], 1u); }
    __syncthreads();
    if (threadIdx.x < MSM_SIZE_BINS && h[threadIdx.x]) base[threadIdx.x] = atomicAdd(a.size_hist + threadIdx.x, h[threadIdx.x]);
    __syncthreads();
    if (id < total) a.order[base[sz] + slot] = id;
}
// one lane per (window, bucket), taken in the order above: sum of the bucket's points (big buckets: the kernels below)
__global__ void __launch_bounds__(256) msm_bucket_kernel(MsmArgs a) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (a.n_windows << a.cb)) return;
    const uint32_t id = a.order[g], w = id >> a.cb;
    const uint32_t lo = a.hist[id], hi = a.cursor[id];
    if (hi - lo > MSM_BIG) return;
    xyzz29 acc; acc.ident = true;
    for (uint32_t k = lo; k < hi; k++) msm_add_point_xyzz(a.pm, acc, a.idx[(uint64_t)w * a.n + k]);
    j_store(a.buckets + (uint64_t)id * 24, msm_xyzz_lower(acc));
}
// ---- big buckets: a work list (bucket, slice) built on the device, one workgroup per slice (lanes stride through the slice, then a
// tree over the 256 lane sums in LDS), one workgroup per big bucket for the slices' sums.  One lane per bucket made a 2^20-point MSM
// whose scalars were all equal -- or whose top window held one digit -- a matter of seconds (2^19 dependent additions).
// Buckets of MSM_BIG < sz <= MSM_MID points (the top window of a uniform 2^23-point MSM: 2^13 buckets of ~1024) are cut into items of
// MSM_MID_SLICE points summed by ONE LANE each, like ordinary buckets, and their <= 32 partial sums are added by one lane per bucket: a
// workgroup per 1024-point bucket spent its time in the 8-level tree over 256 lane sums of 4 points each (4.0 of 38.5 ms at 2^23).
#define MSM_MID 8192u
#define MSM_MID_SLICE 64u
GL_DEV uint32_t msm_big_slice(uint32_t sz) {                       // points per item: at most 256 items per bucket
    // (mid-size buckets: at most 32 lane items of 64 .. 256 points -- with prepared bases and 22-bit windows the 12 significant bits of the top window make
    // 2^11 buckets of 2^12 points each, which took the workgroup path at 2.4 times the lane path's cost per addition while MSM_MID was 2048)
    if (sz <= MSM_MID) return max(MSM_MID_SLICE, (sz + 31) / 32);
    const uint32_t need = (sz + 255) / 256;
    return need > MSM_BIG_WG_POINTS ? ((need + 255) & ~255u) : MSM_BIG_WG_POINTS;
}
__global__ void __launch_bounds__(256) msm_big_list_kernel(MsmArgs a) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (a.n_windows << a.cb)) return;
    const uint32_t sz = a.cursor[id] - a.hist[id];
    if (sz <= MSM_BIG) return;
    const uint32_t slice = msm_big_slice(sz), cnt = (sz + slice - 1) / slice;
    const uint32_t first = atomicAdd(a.big_counters, cnt), slot = atomicAdd(a.big_counters + 1, 1u);
    if (sz > MSM_MID) { atomicAdd(a.big_counters + 2, cnt); atomicAdd(a.big_counters + 3, 1u); }
    if (first + cnt > a.max_items || slot >= a.max_big) return;   // cannot happen: the bounds are sums over all points (host side)
    for (uint32_t c = 0; c < cnt; c++) { a.big_items[2 * (first + c)] = id; a.big_items[2 * (first + c) + 1] = c * slice; }
    a.big_buckets[3 * slot] = id; a.big_buckets[3 * slot + 1] = first; a.big_buckets[3 * slot + 2] = cnt;
}
GL_DEV jac msm_wg_tree(jac acc, uint32_t* sh /* 256 x 24 */) {     // sum of the 256 lanes' points, valid on lane 0
    const uint32_t t = threadIdx.x;
    j_store(sh + 24 * t, acc);
    __syncthreads();
    for (uint32_t st = 128; st >= 1; st >>= 1) {
        if (t < st) { acc = j_add(acc, j_load(sh + 24 * (t + st))); j_store(sh + 24 * t, acc); }
        __syncthreads();
    }
    return acc;
}
// items of mid-size buckets: one lane per item (a fixed grid strides over the work list)
__global__ void __launch_bounds__(256) msm_mid_partial_kernel(MsmArgs a) {
    const uint32_t n_items = *a.big_counters;
    for (uint32_t it = blockIdx.x * blockDim.x + threadIdx.x; it < n_items; it += gridDim.x * blockDim.x) {
        const uint32_t id = a.big_items[2 * it], off = a.big_items[2 * it + 1], w = id >> a.cb;
        const uint32_t base = a.hist[id], end = a.cursor[id];
        if (end - base > MSM_MID) continue;                        // a workgroup item (below)
        const uint32_t lo = base + off, hi = min(end, lo + msm_big_slice(end - base));
        xyzz29 acc; acc.ident = true;
        for (uint32_t k = lo; k < hi; k++) msm_add_point_xyzz(a.pm, acc, a.idx[(uint64_t)w * a.n + k]);
        j_store(a.big_partial + 24ull * it, msm_xyzz_lower(acc));
    }
}
// ... and one lane per mid-size bucket for its partial sums
__global__ void __launch_bounds__(64) msm_mid_final_kernel(MsmArgs a) {
    const uint32_t n_big = a.big_counters[1];
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_big; b += gridDim.x * blockDim.x) {
        const uint32_t id = a.big_buckets[3 * b], first = a.big_buckets[3 * b + 1], cnt = a.big_buckets[3 * b + 2];
        if (a.cursor[id] - a.hist[id] > MSM_MID) continue;
        jac acc = j_load(a.big_partial + 24ull * first);
        for (uint32_t k = 1; k < cnt; k++) acc = j_add(acc, j_load(a.big_partial + 24ull * (first + k)));
        j_store(a.buckets + (uint64_t)id * 24, acc);
    }
}
__global__ void __launch_bounds__(256) msm_big_partial_kernel(MsmArgs a) {      // a fixed grid walks the work list (usually empty)
    __shared__ uint32_t sh[256 * 24];
    // (the list holds the lane items of the mid-size buckets too -- 2^17 of them for the top window of a uniform 2^23-point MSM -- and walking
    // it just to skip them was 2 ms per call: nothing to do unless some bucket takes the workgroup path)
    if (a.big_counters[2] == 0) return;
    const uint32_t n_items = *a.big_counters;
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t id = a.big_items[2 * it], off = a.big_items[2 * it + 1], w = id >> a.cb;
        if (a.cursor[id] - a.hist[id] <= MSM_MID) continue;        // a lane item (above); block-uniform
        const uint32_t lo = a.hist[id] + off, end = a.cursor[id];
        const uint32_t hi = min(end, lo + msm_big_slice(end - a.hist[id]));
        xyzz29 acc29; acc29.ident = true;
        for (uint32_t k = lo + threadIdx.x; k < hi; k += 256) msm_add_point_xyzz(a.pm, acc29, a.idx[(uint64_t)w * a.n + k]);
        jac acc = msm_xyzz_lower(acc29);
        acc = msm_wg_tree(acc, sh);
        if (threadIdx.x == 0) j_store(a.big_partial + 24ull * it, acc);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) msm_big_final_kernel(MsmArgs a) {
    __shared__ uint32_t sh[256 * 24];
    if (a.big_counters[3] == 0) return;
    const uint32_t n_big = a.big_counters[1];
    for (uint32_t b = blockIdx.x; b < n_big; b += gridDim.x) {
        const uint32_t id = a.big_buckets[3 * b], first = a.big_buckets[3 * b + 1], cnt = a.big_buckets[3 * b + 2];
        if (a.cursor[id] - a.hist[id] <= MSM_MID) continue;        // msm_mid_final_kernel's; block-uniform
        jac acc = threadIdx.x < cnt ? j_load(a.big_partial + 24ull * (first + threadIdx.x)) : j_identity();
        acc = msm_wg_tree(acc, sh);
        if (threadIdx.x == 0) j_store(a.buckets + (uint64_t)id * 24, acc);
        __syncthreads();
    }
}

// Window sum  sum_j (j + 1) * B_j = Wt + S  by a recursion on pairs (S, Wt) = (sum of the items, sum of local index * item) over groups of 2^kbits
// items: a group of buckets gives S = sum B_b and Wt = sum (b - b0) B_b by the running-sum trick (S_run += B_b from the top,
// L += S_run); a group of pairs at the next level gives  S' = sum S_u,  Wt' = sum Wt_u + width * sum (u - u0) S_u  with
// width = the number of buckets one item spans (a power of two: `shift` doublings).  Every level is one launch of (windows x groups)
// lanes whose dependent chain is ~3 * 2^kbits additions; the single-lane tails of the first version (256 + 48 and then 256 dependent
// additions per window: 19 of 34 ms at 2^20 points) are gone.  The last level's single group gives the window sum Wt + S.
struct MsmLevel {
    const uint32_t* in_s;       // [W][t_in][24]
    const uint32_t* in_w;       // [W][t_in][24] or null (level 0: the items are the buckets themselves)
    uint32_t* out_s;            // [W][t_in >> kbits][24]
    uint32_t* out_w;
    uint32_t t_in, kbits, shift, n_windows;
};
__global__ void __launch_bounds__(64) msm_level_kernel(MsmLevel l) {
    const uint32_t groups = l.t_in >> l.kbits;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups * l.n_windows) return;
    const uint32_t w = g / groups, v = g % groups, k = 1u << l.kbits;
    const uint32_t* s_in = l.in_s + ((uint64_t)w * l.t_in + (uint64_t)v * k) * 24;
    jac29 run, acc;
    run.ident = acc.ident = true;
    for (uint32_t u = k; u-- > 0;) {
        jac29_add(run, jac29_lift(j_load(s_in + u * 24)));
        if (u) jac29_add(acc, run);                                   // acc = sum_u u * S_u: item u is counted in the u sums taken at u' = u .. 1
    }
    for (uint32_t d = 0; d < l.shift; d++) jac29_double(acc);
    if (l.in_w) {
        const uint32_t* w_in = l.in_w + ((uint64_t)w * l.t_in + (uint64_t)v * k) * 24;
        for (uint32_t u = 0; u < k; u++) jac29_add(acc, jac29_lift(j_load(w_in + u * 24)));
    }
    j_store(l.out_s + ((uint64_t)w * groups + v) * 24, jac29_lower(run));
    j_store(l.out_w + ((uint64_t)w * groups + v) * 24, jac29_lower(acc));
}

// The same level with EIGHT LANES PER GROUP (kbits == 3).  A level is pure latency -- one lane's chain of ~26 dependent additions of ~30 us
// each, whatever the level's size: 7 levels were 5.7 of 38.5 ms at 2^23 points -- so the chain is cut instead: suffix sums of the eight S_u
// by a three-step scan across the lanes, sum_{u >= 1} run_u and sum_u Wt_u by three-step trees: 10 dependent additions + the doublings.
GL_DEV jac29 jac29_shfl_down(const jac29& p, uint32_t d) {
    jac29 r;
#pragma unroll
    for (int j = 0; j < 9; j++) { r.x.l[j] = __shfl_down(p.x.l[j], d, 8); r.y.l[j] = __shfl_down(p.y.l[j], d, 8); r.z.l[j] = __shfl_down(p.z.l[j], d, 8); }
    r.ident = __shfl_down((int)p.ident, d, 8) != 0;
    return r;
}
__global__ void __launch_bounds__(64) msm_level_coop_kernel(MsmLevel l) {
    const uint32_t groups = l.t_in >> 3, total = groups * l.n_windows;
    const uint32_t gq = blockIdx.x * 8 + (threadIdx.x >> 3), u = threadIdx.x & 7;
    const bool live = gq < total;
    const uint32_t g = live ? gq : total - 1;                        // idle groups of the last block redo the last one (lanes stay for the shuffles)
    const uint32_t w = g / groups, v = g % groups;
    const uint64_t item = (uint64_t)w * l.t_in + (uint64_t)v * 8 + u;
    jac29 x = jac29_lift(j_load(l.in_s + item * 24));
#pragma unroll 1
    for (uint32_t d = 1; d < 8; d <<= 1) {                           // x_u = S_u + ... + S_7
        const jac29 y = jac29_shfl_down(x, d);
        if (u + d < 8) jac29_add(x, y);
    }
    jac29 acc = x;                                                    // sum_{u >= 1} run_u = sum_u u S_u
    if (!u) acc.ident = true;
#pragma unroll 1
    for (uint32_t d = 4; d >= 1; d >>= 1) {
        const jac29 y = jac29_shfl_down(acc, d);
        if (u < d) jac29_add(acc, y);
    }
    if (u == 0) for (uint32_t d = 0; d < l.shift; d++) jac29_double(acc);
    if (l.in_w) {
        jac29 wt = jac29_lift(j_load(l.in_w + item * 24));
#pragma unroll 1
        for (uint32_t d = 4; d >= 1; d >>= 1) {
            const jac29 y = jac29_shfl_down(wt, d);
            if (u < d) jac29_add(wt, y);
        }
        if (u == 0) jac29_add(acc, wt);
    }
    if (u == 0 && live) {
        j_store(l.out_s + ((uint64_t)w * groups + v) * 24, jac29_lower(x));
        j_store(l.out_w + ((uint64_t)w * groups + v) * 24, jac29_lower(acc));
    }
}

}  // namespace gl355

using namespace gl355;

// ---- one MSM call, host side: plan the sizes, carve one scratch block, launch the sort, the accumulation and the reduction on the context's
// stream, read the window sums back
struct MsmLv { uint32_t t_in, kbits, shift; };
struct MsmPlan {
    MsmArgs a;                  // what the kernels get.  n, n_windows and wps are the REAL sizes until msm_digits_kernel has run (msm_launch_sort)
    bool virt;                  // prepared bases: the kernels past msm_digits_kernel see ONE window of wps n points per scalar set
    uint64_t rn;                // the real number of points
    uint64_t n, W;              // points per window and windows as those kernels see them
    uint64_t nb, nbin;          // buckets per window, coarse bins of the two-level sort
    bool two_level, one_window;
    std::vector<MsmLv> levels;  // reduction levels: groups of 8 items, the last level takes what is left
    uint64_t lvl_words;
    uint64_t fb_max_reg, fb_max_items;
    uint64_t words32;           // the scratch block, in 32-bit words
    uint32_t* lvl;              // [lvl_words] the levels' outputs
    const uint32_t *fin_s, *fin_w;      // per window S and Wt (null without levels): the last level's outputs
};

static int32_t msm_plan(Ctx* ctx, uint64_t n, uint32_t m, uint32_t max_bits, const gl355_msm_bases* bases, MsmPlan& pl) {
    MsmArgs& a = pl.a;
    memset(&a, 0, sizeof a);
    uint32_t lg = 0;
    while ((1ull << lg) < n) lg++;
    a.n = n;
    // window bits.  Fewer, larger windows mean fewer additions in the bucket phase (n per window) and more buckets to reduce; and the
    // TOP window should not be nearly empty: scalars are < r < 2^254, so a top window of only a few bits puts everything into a handful
    // of buckets (workgroup path below, contended counters).  254 = 14 * 17 + 16 = 12 * 20 + 14.  Measured (uniform scalars, ms):
    //   2^18: c = 15 / 16 / 17 -> 3.7 / 3.9 / 4.1;   2^20: 16 / 17 / 18 -> 7.3 / 7.1 / 8.3;   2^22: 16 / 17 / 18 / 19 -> 23.6 / 19.1 / 20.7 / 32.9
    //   2^23-point calls, k = 23 proof: c = 18 / 19 / 20 / 21 -> 1.155 / 1.115 / 1.118 / 1.235 s
    a.c = bases ? bases->c : (lg <= 6 ? 4 : (lg <= 18 ? lg - 2 : (lg <= 22 ? 17 : 20)));
    // scalars shorter than a window (range-check limbs): ONE window just wide enough that no digit reaches 2^(c-1), so nothing is negative, nothing carries
    // and the carry window does not exist -- 2^16 buckets for a 16-bit column instead of two windows of 2^19 (two-level sort from 12 bits on)
    const bool one_window = !bases && max_bits + 1 < a.c && max_bits + 1 >= 12;
    pl.one_window = one_window;
    if (one_window) a.c = max_bits + 1;
    a.cb = a.c - 1;
    a.wps = 256 / a.c + 1;                                       // signed digits: the carry out of bit 255 needs a window of its own
    if (max_bits < 256) a.wps = std::min(a.wps, (std::max(1u, max_bits) + a.c - 1) / a.c + 1);
    if (one_window) a.wps = 1;
    if (bases && a.wps > bases->wps) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm: prepared bases hold too few windows");
    a.n_sets = m;
    a.n_windows = a.wps * m;
    // SHARED BUCKETS (prepared bases): point i of window w is the table entry w n + i, whose own digit is the scalar's w-th -- an MSM of wps n
    // points with ONE window per scalar set.  The digit array [set][w][i] is already that MSM's [set][w n + i], so past msm_digits_kernel every
    // kernel runs unchanged on the virtual sizes: 2^cb buckets per SET to size-sort, accumulate and reduce instead of per window, and the set's
    // sum comes out of the last level (no doublings between windows on the host).
    pl.virt = bases != nullptr;
    pl.rn = n;
    pl.n = n;
    pl.W = a.n_windows;
    if (bases) {
        if (n * a.wps >= (1ull << 31)) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_msm: prepared bases x windows beyond 2^31 entries");
        a.have_table = 1;
        pl.n = n * a.wps; pl.W = m;
    }
    const uint64_t W = pl.W, nb = pl.nb = 1ull << a.cb;
    n = pl.n;                                                    // from here on the sizes are the virtual ones when the bases are prepared
    pl.levels.clear();
    pl.lvl_words = 0;
    for (uint32_t t = (uint32_t)nb, shift = 0; t > 1;) {
        uint32_t kb = 3;
        while ((1u << kb) > t) kb--;
        pl.levels.push_back({t, kb, shift});
        t >>= kb; shift += kb;
        pl.lvl_words += 2ull * W * t * 24;
    }
    // the two-level sort: from 2^11 buckets per window on (below that the histograms are small and the point count with them)
    pl.two_level = a.cb > MSM_FINE_BITS;      // (below: one-level sort with device-scope atomics per point and window)
    a.cbits = pl.two_level ? a.cb - MSM_FINE_BITS : 0;
    const uint64_t nbin = pl.nbin = 1ull << a.cbits;
    a.chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096, 32 * nbin), 1ull << 20);
    // big-bucket work list: a bucket of sz > MSM_BIG points makes ceil(sz / slice) items with slice >= MSM_BIG_WG_POINTS, so over all
    // buckets at most W n / MSM_BIG_WG_POINTS + (number of big buckets) items, and at most W n / MSM_BIG big buckets
    a.max_big = (uint32_t)(W * n / MSM_BIG + 1);
    a.max_items = (uint32_t)(W * n / MSM_MID_SLICE + a.max_big + 1);      // (mid-size buckets: items of MSM_MID_SLICE points)
    pl.fb_max_reg = W * n / MSM_FINE_BIG + 1; pl.fb_max_items = W * n / MSM_FINE_SLICE + pl.fb_max_reg + 1;      // (sums over all pairs)
    const uint64_t sort_words = pl.two_level ? 3 * W * n + 3 * W * nbin + 2 + 2 + 2 * pl.fb_max_reg + 2 * pl.fb_max_items : 0;
    pl.words32 = (bases ? 0 : n * 16) + 3 * W * nb + W * n + W * nb * 24 + (MSM_SIZE_BINS + 5) + pl.lvl_words + 64 +
                 2ull * a.max_items + 3ull * a.max_big + 24ull * a.max_items + sort_words;
    return GL355_OK;
}
// the MsmArgs pointers out of the scratch block `p` (pl.words32 words; `tab`: the prepared bases' table or null), counters and histograms cleared
static int32_t msm_carve(Ctx* ctx, MsmPlan& pl, uint32_t* p, uint32_t* tab) {
    MsmArgs& a = pl.a;
    const uint64_t n = pl.n, W = pl.W, nb = pl.nb, nbin = pl.nbin;
    if (tab) a.pm = tab; else { a.pm = p; p += n * 16; }
    a.hist = p; p += W * nb;
    a.size_hist = p; a.big_counters = p + MSM_SIZE_BINS; p += MSM_SIZE_BINS + 5;      // behind the histograms: cleared with them
    a.cursor = p; p += W * nb;
    a.order = p; p += W * nb;
    a.idx = p; p += W * n;
    a.buckets = p; p += W * nb * 24;
    a.big_items = p; p += 2ull * a.max_items;
    a.big_buckets = p; p += 3ull * a.max_big;
    a.big_partial = p; p += 24ull * a.max_items;
    pl.lvl = p; p += pl.lvl_words;
    if (pl.two_level) {
        p += (2 - ((uintptr_t)p / 4) % 2) % 2;                      // 8-byte alignment of the pairs
        a.pairs = p; p += 2 * W * n;
        a.dig = p; p += W * n;
        a.coarse_cnt = p; p += W * nbin;
        a.coarse_fill = p; p += W * nbin;
        a.coarse_start = p; p += W * nbin;
        a.fb_counters = p; p += 2;
        a.fb_regions = p; p += 2 * pl.fb_max_reg;
        a.fb_items = p; p += 2 * pl.fb_max_items;
        a.fb_max_reg = (uint32_t)pl.fb_max_reg; a.fb_max_items = (uint32_t)pl.fb_max_items;
        GL355_HIP(ctx, hipMemsetAsync(a.coarse_cnt, 0, 2 * W * nbin * 4, ctx->stream));
        GL355_HIP(ctx, hipMemsetAsync(a.fb_counters, 0, 8, ctx->stream));
    }
    GL355_HIP(ctx, hipMemsetAsync(a.hist, 0, (W * nb + (MSM_SIZE_BINS + 5)) * 4, ctx->stream));
    return GL355_OK;
}
// hist / cursor (start and end of every bucket's range) and idx (the point indices by bucket)
static void msm_launch_sort(Ctx* ctx, MsmPlan& pl) {
    MsmArgs& a = pl.a;
    hipStream_t s_ = ctx->stream;
    const uint32_t blk = (uint32_t)((pl.rn + 255) / 256), W = (uint32_t)pl.W, nbin = (uint32_t)pl.nbin;
    if (pl.two_level) hipLaunchKernelGGL(msm_digits_kernel, dim3(blk), dim3(256), 0, s_, a);
    if (pl.virt) { a.n = pl.n; a.n_windows = W; a.wps = 1; }      // the virtual MSM: every kernel below sees one window per set
    if (!pl.two_level) {
        hipLaunchKernelGGL(msm_prepare_kernel, dim3(blk), dim3(256), 0, s_, a);
        hipLaunchKernelGGL(msm_scan_kernel, dim3(W), dim3(1024), 0, s_, a);
        hipLaunchKernelGGL(msm_scatter_kernel, dim3(blk), dim3(256), 0, s_, a);
        return;
    }
    const dim3 cgrid((uint32_t)((pl.n + a.chunk - 1) / a.chunk), W);
    hipLaunchKernelGGL(msm_coarse_count_kernel, cgrid, dim3(256), nbin * 4, s_, a);
    hipLaunchKernelGGL(msm_coarse_scan_kernel, dim3(W), dim3(1024), 0, s_, a);
    hipLaunchKernelGGL(msm_coarse_scatter_kernel, cgrid, dim3(256), nbin * 8, s_, a);
    hipLaunchKernelGGL(msm_fine_sort_kernel, dim3(nbin, W), dim3(256), 0, s_, a);
    // regions too large for one workgroup (usually none: the three kernels behind the list then find empty work lists)
    hipLaunchKernelGGL(msm_fine_big_list_kernel, dim3((uint32_t)((pl.W * pl.nbin + 255) / 256)), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_fine_big_count_kernel, dim3(2048), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_fine_big_scan_kernel, dim3(256), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_fine_big_scatter_kernel, dim3(2048), dim3(256), 0, s_, a);
}
// the bucket sums: buckets by decreasing size, one lane per bucket, lane and workgroup items for the overfull ones
static void msm_launch_accumulate(Ctx* ctx, const MsmPlan& pl) {
    const MsmArgs& a = pl.a;
    hipStream_t s_ = ctx->stream;
    const uint32_t bblk = (uint32_t)((pl.W * pl.nb + 255) / 256);
    hipLaunchKernelGGL(msm_size_hist_kernel, dim3(bblk), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_size_scan_kernel, dim3(1), dim3(64), 0, s_, a);
    hipLaunchKernelGGL(msm_order_kernel, dim3(bblk), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_big_list_kernel, dim3(bblk), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_bucket_kernel, dim3(bblk), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_mid_partial_kernel, dim3(std::min<uint32_t>((a.max_items + 255) / 256, 2048)), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_big_partial_kernel, dim3(std::min<uint32_t>(a.max_items, 1536)), dim3(256), 0, s_, a);
    hipLaunchKernelGGL(msm_mid_final_kernel, dim3(std::min<uint32_t>((a.max_big + 63) / 64, 1024)), dim3(64), 0, s_, a);
    hipLaunchKernelGGL(msm_big_final_kernel, dim3(std::min<uint32_t>(a.max_big, 512)), dim3(256), 0, s_, a);
}
// the window sums (S, Wt) out of the buckets, level by level
static void msm_launch_reduce(Ctx* ctx, MsmPlan& pl) {
    hipStream_t s_ = ctx->stream;
    const uint64_t W = pl.W;
    const uint32_t *cs = pl.a.buckets, *cw = nullptr;
    uint32_t* lv_p = pl.lvl;
    for (const MsmLv& lv : pl.levels) {
        MsmLevel l;
        l.in_s = cs; l.in_w = cw; l.t_in = lv.t_in; l.kbits = lv.kbits; l.shift = lv.shift; l.n_windows = (uint32_t)W;
        const uint64_t groups = lv.t_in >> lv.kbits;
        l.out_s = lv_p; lv_p += W * groups * 24;
        l.out_w = lv_p; lv_p += W * groups * 24;
        // eight lanes per group where a level is latency-bound (few groups); the large first levels are throughput-bound and the scan
        // costs them twice the wave-level additions.  coop_max: the largest W x groups that runs the cooperative form
        constexpr uint64_t coop_max = 16384;
        if (lv.kbits == 3 && W * groups <= coop_max) hipLaunchKernelGGL(msm_level_coop_kernel, dim3((uint32_t)((W * groups + 7) / 8)), dim3(64), 0, s_, l);
        else hipLaunchKernelGGL(msm_level_kernel, dim3((uint32_t)((W * groups + 63) / 64)), dim3(64), 0, s_, l);
        cs = l.out_s; cw = l.out_w;
    }
    pl.fin_s = cs; pl.fin_w = cw;
}

int32_t gl355::bn254_msm_bits(gl355_ctx* h, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint32_t m, uint32_t max_bits, uint64_t* result,
                              const gl355_msm_bases* bases, uint32_t* plan_out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (bases && (bases->ctx != ctx || bases->n != n)) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm: prepared bases of another context or size");
    if (!result || ((!(points || bases) || !scalars) && n)) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm: null argument");
    if (n > (1ull << 26)) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_msm: more than 2^26 points");
    if (m == 0) return GL355_OK;
    if (m > 64 || (uint64_t)m * n > (1ull << 27)) return ctx->fail(GL355_E_UNSUPPORTED, "bn254_g1_msm_batch: more than 64 scalar sets or 2^27 scalars in all");
    const bool dev_result = ptr_is_device(result);
    if (n == 0) {
        if (dev_result) { GL355_HIP(ctx, hipMemsetAsync(result, 0, 64ull * m, ctx->stream)); GL355_HIP(ctx, ctx->wait()); }
        else memset(result, 0, 64ull * m);
        return GL355_OK;
    }
    MsmPlan pl;
    GL355_TRY(msm_plan(ctx, n, m, max_bits, bases, pl));
    if (plan_out) { plan_out[0] = pl.a.c; plan_out[1] = pl.a.wps; plan_out[2] = pl.one_window; plan_out[3] = pl.two_level; }
    Staged sp(ctx), ss(ctx);
    if (!bases) GL355_TRY(sp.open(points, n * 64, 1));
    GL355_TRY(ss.open(scalars, (uint64_t)m * n * 32, 1));
    pl.a.points = bases ? nullptr : sp.as<uint64_t>(); pl.a.scalars = ss.as<uint64_t>();
    Scratch buf(ctx);
    GL355_TRY(buf.get(pl.words32 * 4 + 64));
    GL355_TRY(msm_carve(ctx, pl, buf.as<uint32_t>(), bases ? bases->tab : nullptr));
    {
        ProfScope ps(ctx, "bn254_g1_msm", pl.n * (64 + 32ull * m));
        msm_launch_sort(ctx, pl);
        msm_launch_accumulate(ctx, pl);
        msm_launch_reduce(ctx, pl);
        GL355_HIP(ctx, hipGetLastError());
    }
    // per window S (and Wt when there was at least one level): 2 x W Jacobian points to the host, which combines the windows
    const MsmArgs& a = pl.a;
    const uint64_t W = pl.W;
    std::vector<uint32_t> hs(W * 24), hw(W * 24, 0);
    uint32_t big_used[5] = {0, 0, 0, 0, 0};
    GL355_HIP(ctx, ctx->d2h(big_used, a.big_counters, sizeof big_used));
    GL355_HIP(ctx, ctx->d2h(hs.data(), pl.fin_s, W * 96));
    if (pl.fin_w) GL355_HIP(ctx, ctx->d2h(hw.data(), pl.fin_w, W * 96));
    GL355_HIP(ctx, ctx->wait());
    if (big_used[0] > a.max_items || big_used[1] > a.max_big) return ctx->fail(GL355_E_HIP, "bn254_g1_msm: big-bucket work list overflow (internal bound)");
    if (big_used[4]) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm: a scalar has more bits than max_bits promised (the plan's signed digits cannot hold it)");
    const bool have_w = !pl.levels.empty();
    std::vector<uint64_t> res(8ull * m);
    for (uint32_t set = 0; set < m; set++)
        bn254_g1_horner_host(hs.data() + 24ull * set * a.wps, have_w ? hw.data() + 24ull * set * a.wps : nullptr, a.wps, a.c, res.data() + 8 * set);
    if (dev_result) { GL355_HIP(ctx, hipMemcpyAsync(result, res.data(), 64ull * m, hipMemcpyHostToDevice, ctx->stream)); GL355_HIP(ctx, ctx->wait()); }
    else memcpy(result, res.data(), 64ull * m);
    return GL355_OK;
}

extern "C" {
int32_t gl355_bn254_g1_msm(gl355_ctx* h, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint64_t result[8]) {
    return bn254_msm_bits(h, points, scalars, n, 1, 256, result);
}
int32_t gl355_bn254_g1_msm_batch(gl355_ctx* h, const uint64_t* points, const uint64_t* scalars, uint64_t n, uint32_t n_sets, uint64_t* results) {
    return bn254_msm_bits(h, points, scalars, n, n_sets, 256, results);
}

int32_t gl355_bn254_g1_msm_prepared(gl355_ctx* h, const gl355_msm_bases* bases, const uint64_t* scalars, uint32_t n_sets, uint64_t* results) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!bases) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm_prepared: null bases");
    return bn254_msm_bits(h, nullptr, scalars, bases->n, n_sets, 256, results, bases);
}
// test hook (tests/test_gpu_msm_bits.py): bn254_msm_bits under a caller's max_bits, and the plan it ran
int32_t gl355_bn254_g1_msm_bits(gl355_ctx* h, const uint64_t* points, const gl355_msm_bases* bases, const uint64_t* scalars, uint64_t n, uint32_t n_sets,
                                uint32_t max_bits, uint64_t* results, uint32_t plan_out[4]) {
    return bn254_msm_bits(h, bases ? nullptr : points, scalars, n, n_sets, max_bits, results, bases, plan_out);
}
int32_t gl355_bn254_g1_msm_bases_free(gl355_ctx* h, gl355_msm_bases* bases) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!bases) return GL355_OK;
    if (bases->ctx != ctx) return ctx->fail(GL355_E_INVALID_ARG, "bn254_g1_msm_bases_free: bases of another context");
    (void)ctx->wait();
    ctx->release(bases->tab);
    delete bases;
    return GL355_OK;
}
}  // extern "C"
