// CircuitData::prove for B independent units of ONE circuit in lock-step on one prover context
// (src/plonky2_semaphore/access_set.rs:94, recursion.rs:168, wrapper.rs:55; the reference proves its units from a rayon
// par_iter, recursion.rs:214-227,300-308).
//
// Why lock-step batches: a single proof of n = 2^13..2^14 is ~430 kernel launches of which ~350 are shorter than 30 us (Merkle
// levels of a few thousand nodes, FRI layers, scans) and ~20 host round trips for the Fiat-Shamir transcript -- the device idles
// between them and the small levels run the 16-lanes-per-node permutation (3x the instructions) only to cut latency.  Giving
// every stage a unit dimension makes each launch B times larger (Merkle levels reach the one-lane-per-node kernel B levels
// earlier, small kernels fill the chip), divides launches and host round trips per unit by B, and keeps every unit's bytes
// exactly what a one-by-one proof produces: the units never interact, each has its own transcript (host, ~50 permutations),
// challenges, blinding key and proof buffer.  B = 1 is the single-proof entry (gl355_prove, gl355_prove_sparse).
//
// Stage order and transcript: chip/plonk/plonk_verifier_chip.rs:55-154; oracle and opening order: types/common_data.rs:100-222,
// types/assigned.rs:26-44; permutation argument: chip/plonk/vanishing_poly.rs:54-108,183-218; DEEP / FRI:
// chip/fri_chip.rs:112-149,168-226,275-327,364-376.
//
// Layout in HBM (all unit-major, uniform strides): coefficients [B * batch][n], LDE [B * batch][N] column-major in bit-reversed
// row order (what the DIF transform writes), salt columns [B * 4][N] apart from the LDE (so the NTT sees one uniform batch of
// B * batch columns; the leaf hash and the query openings read the salt segment for the last four leaf elements), digests
// [B][..] in plonky2's layout, caps [B][2^cap_height][4].  B trees of 2^cap_height cap subtrees are, to the Merkle kernels,
// one forest of B * 2^cap_height subtrees.
//
// This file: witness, salt and permutation-argument kernels, the commitment of a batch of units, and prove_units as eight stage
// routines over one ProveRun.  The kernels of the opening, DEEP, FRI and query stages and fri_tail_units are in fri.hip (shared
// with the staged C entry points, which call them with B = 1), the quotient in quotient.hip, Merkle trees and the grinder in merkle.hip.
#include "gl355_internal.h"
#include "blinding.cuh"

using namespace gl355;

namespace gl355 {

// ---- committed batches of B units ------------------------------------------------------------------------------------------
struct BOracle {
    Ctx* ctx = nullptr;
    uint32_t B = 0, log_n = 0, rate_bits = 0, batch = 0, leaf_len = 0, cap_height = 0;
    uint64_t* base = nullptr;
    uint64_t *coeffs = nullptr, *lde = nullptr, *salt = nullptr, *digests = nullptr, *cap = nullptr;
    uint64_t n_dig = 0;      // digests per unit
    ~BOracle() { if (base && ctx) ctx->release(base); }
    int32_t alloc(Ctx* c, uint32_t b, uint32_t lg, uint32_t rb, uint32_t bat, bool salted, uint32_t cap_h) {
        ctx = c; B = b; log_n = lg; rate_bits = rb; batch = bat; leaf_len = bat + (salted ? GL355_SALT_SIZE : 0); cap_height = cap_h;
        const uint64_t n = 1ull << lg, N = n << rb, n_cap = 1ull << cap_h;
        n_dig = 2 * (N - n_cap);
        const uint64_t total = (uint64_t)B * ((uint64_t)bat * n + (uint64_t)leaf_len * N + n_dig * 4 + n_cap * 4);
        void* p = nullptr;
        GL355_TRY(c->alloc(total * 8, &p));
        base = reinterpret_cast<uint64_t*>(p);
        coeffs = base;
        lde = coeffs + (uint64_t)B * bat * n;
        salt = salted ? lde + (uint64_t)B * bat * N : nullptr;
        digests = lde + (uint64_t)B * leaf_len * N;
        cap = digests + (uint64_t)B * n_dig * 4;
        return GL355_OK;
    }
};

static OView view_of(const BOracle& o) {
    const uint64_t n = 1ull << o.log_n, N = n << o.rate_bits;
    return OView{o.coeffs, (uint64_t)o.batch * n, o.lde, (uint64_t)o.batch * N, o.salt, (uint64_t)GL355_SALT_SIZE * N, o.digests, o.n_dig * 4, o.batch, o.leaf_len};
}
// constants_sigmas, shared by all units.  Only for a batch committed without salt (prove_units checks batch == leaf_len): a salted
// gl355_oracle keeps its salt columns inside lde, which is the view oracle_open_batch_on builds (capi.hip)
static OView view_of(const gl355_oracle* o) {
    return OView{o->coeffs, 0, o->lde, 0, nullptr, 0, o->digests, 0, o->batch, o->leaf_len};
}

struct UnitKeys { BlindKey k[MAXB]; };

// ---- witness ---------------------------------------------------------------------------------------------------------------
// scatter the sparse witness rows of every unit into its column-major wire matrix (rows: [B][n_rows][num_wires])
__global__ void witness_rows_units_kernel(uint64_t* wires, uint64_t n, uint32_t num_wires, const uint32_t* row_idx, const uint64_t* row_vals,
                                          uint32_t n_rows) {
    const uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t per = (uint64_t)n_rows * num_wires;
    if (g >= per) return;
    const uint32_t u = blockIdx.y, r = g / num_wires, c = g % num_wires;
    wires[((uint64_t)u * num_wires + c) * n + row_idx[r]] = gl_canon(row_vals[(uint64_t)u * per + g]);
}
// element g of unit u's witness-blinding stream: g < n_blind * num_wires fills wire g / n_blind of blinding row g % n_blind; the next
// n_z_pairs * num_routed elements are the Z-blinding pairs: element c * n_z_pairs + k is the value of routed column c on BOTH rows of
// pair k (plonky2 `blind`: every routed wire of a pair is random and copy-constrained between its two rows -- one value per pair on
// column 0 only, as in round 2, left Z_0 and Z_1 at a blinding row functions of the same value)
__global__ void witness_blind_units_kernel(uint64_t* wires, uint64_t n, uint32_t num_wires, uint32_t num_routed, uint32_t blind_start, uint32_t n_blind,
                                           uint32_t z_start, uint32_t n_z_pairs, UnitKeys keys) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t n_a = (uint64_t)n_blind * num_wires, n_z = (uint64_t)n_z_pairs * num_routed;
    if (4 * b >= n_a + n_z) return;
    const uint32_t u = blockIdx.y;
    uint64_t* w = wires + (uint64_t)u * num_wires * n;
    uint64_t e[4];
    blind_block_elements(keys.k[u], GL355_BLIND_STREAM_WITNESS, (uint32_t)b, e);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t g = 4 * b + j;
        if (g < n_a) {
            const uint32_t c = g / n_blind, r = g % n_blind;
            w[(uint64_t)c * n + blind_start + r] = e[j];
        } else if (g < n_a + n_z) {
            const uint64_t h = g - n_a, c = h / n_z_pairs, k = h % n_z_pairs;
            w[c * n + z_start + 2 * k] = e[j];
            w[c * n + z_start + 2 * k + 1] = e[j];
        }
    }
}
// salt columns of a blinded oracle, written straight into leaf (bit-reversed row) order: stream element c * N + i is the salt of
// column c at natural row i (what plonky2 appends to the LDE before its transpose), stored at row bitrev(i)
__global__ void salt_units_kernel(uint64_t* salt, uint32_t lde_bits, UnitKeys keys, uint32_t stream) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t N = 1ull << lde_bits, cnt = (uint64_t)GL355_SALT_SIZE * N;
    if (4 * b >= cnt) return;
    const uint32_t u = blockIdx.y;
    uint64_t e[4];
    blind_block_elements(keys.k[u], stream, (uint32_t)b, e);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t g = 4 * b + j;          // N >= 4 is a multiple of 4: the four elements are in one column
        const uint64_t c = g >> lde_bits, i = g & (N - 1);
        const uint64_t r = __brevll(i) >> (64 - lde_bits);
        salt[((uint64_t)u * GL355_SALT_SIZE + c) * N + r] = e[j];
    }
}

// ---- a9: permutation argument, instance = (unit, challenge) ---------------------------------------------------------------------
struct ZsArgs {
    const uint64_t* wires; uint64_t wires_us;     // [B][num_wires][n]
    const uint64_t* sigmas; const uint64_t* k_is;
    uint32_t log_n, n_routed, max_degree, nch, n_chunks, npp;
    uint64_t g;
    uint64_t* chunk_q;    // [inst][n_chunks][n]
    uint64_t* row_prod;   // [inst][n]
    uint64_t* zbuf; uint64_t z_us;                // unit u: [Z_0..Z_{nch-1} | pp_{0,*} | pp_{1,*} ...][n]
    UnitVals betas, gammas;                       // [u * 4 + k]
};
constexpr int ZS_MAX_CHUNKS = 16;
// per row: the n_chunks chunk quotients prod(num)/prod(den) and their product; ONE field inversion per row (prefix products of
// the chunk denominators, inverse of the total, walked back) instead of one per chunk
__global__ void __launch_bounds__(256) zs_rows_units_kernel(ZsArgs a) {
    const uint64_t n = 1ull << a.log_n;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t inst = blockIdx.y, u = inst / a.nch, k = inst % a.nch;
    const uint64_t beta = a.betas.v[u * 4 + k], gamma = a.gammas.v[u * 4 + k];
    const uint64_t* wires = a.wires + (uint64_t)u * a.wires_us;
    const uint64_t x = gl_pow(a.g, i);
    const uint64_t bx = gl_mul(beta, x);
    uint64_t num[ZS_MAX_CHUNKS], pre[ZS_MAX_CHUNKS], den[ZS_MAX_CHUNKS];
    uint64_t run = 1;
#pragma unroll
    for (int ch = 0; ch < ZS_MAX_CHUNKS; ch++) {
        num[ch] = 1; den[ch] = 1; pre[ch] = run;
        if ((uint32_t)ch < a.n_chunks) {
            uint64_t nm = 1, dn = 1;
            for (uint32_t j = ch * a.max_degree; j < (ch + 1) * a.max_degree && j < a.n_routed; j++) {
                const uint64_t w = wires[(uint64_t)j * n + i];
                nm = gl_mul(nm, gl_add(gl_add(w, gl_mul(bx, a.k_is[j])), gamma));
                dn = gl_mul(dn, gl_add(gl_add(w, gl_mul(beta, a.sigmas[(uint64_t)j * n + i])), gamma));
            }
            num[ch] = nm; den[ch] = dn;
            run = gl_mul(run, dn);
        }
    }
    uint64_t inv = gl_inv(run);          // 1 / prod_ch den[ch]
    uint64_t rp = 1;
    uint64_t* cq = a.chunk_q + (uint64_t)inst * a.n_chunks * n;
#pragma unroll
    for (int ch = ZS_MAX_CHUNKS - 1; ch >= 0; ch--) {
        if ((uint32_t)ch < a.n_chunks) {
            const uint64_t dinv = gl_mul(inv, pre[ch]);      // 1 / den[ch]
            inv = gl_mul(inv, den[ch]);
            const uint64_t q = gl_mul(num[ch], dinv);
            cq[(uint64_t)ch * n + i] = q;
            rp = gl_mul(rp, q);
        }
    }
    a.row_prod[(uint64_t)inst * n + i] = rp;
}
// one workgroup per instance: z[i] = prod_{j<i} row_prod[j], tile-by-tile log-step product scan
__global__ void __launch_bounds__(1024) zs_scan_units_kernel(ZsArgs a) {
    __shared__ uint64_t sh[1024];
    const int tid = threadIdx.x;
    const uint32_t inst = blockIdx.x, u = inst / a.nch, k = inst % a.nch;
    const uint64_t n = 1ull << a.log_n;
    const uint64_t* row_prod = a.row_prod + (uint64_t)inst * n;
    uint64_t* z = a.zbuf + (uint64_t)u * a.z_us + (uint64_t)k * n;
    uint64_t running = 1;
    for (uint64_t base = 0; base < n; base += 1024) {
        const uint64_t i = base + tid;
        uint64_t v = i < n ? row_prod[i] : 1;
        sh[tid] = v;
        __syncthreads();
        for (int s = 1; s < 1024; s <<= 1) {
            uint64_t o = tid >= s ? sh[tid - s] : 1;
            __syncthreads();
            v = gl_mul(v, o);
            sh[tid] = v;
            __syncthreads();
        }
        const uint64_t excl = tid ? sh[tid - 1] : 1;
        if (i < n) z[i] = gl_canon(gl_mul(running, excl));
        const uint64_t tile_total = sh[1023];
        __syncthreads();
        running = gl_mul(running, tile_total);
    }
}
// partial products: acc = z[i]; acc *= q[ch][i]; pp[ch][i] = acc  (ch < n_chunks - 1)
__global__ void zs_partials_units_kernel(ZsArgs a) {
    const uint64_t n = 1ull << a.log_n;
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t inst = blockIdx.y, u = inst / a.nch, k = inst % a.nch;
    uint64_t* zu = a.zbuf + (uint64_t)u * a.z_us;
    const uint64_t* cq = a.chunk_q + (uint64_t)inst * a.n_chunks * n;
    uint64_t* pp = zu + ((uint64_t)a.nch + (uint64_t)k * a.npp) * n;
    uint64_t acc = zu[(uint64_t)k * n + i];
    for (uint32_t ch = 0; ch + 1 < a.n_chunks; ch++) {
        acc = gl_mul(acc, cq[(uint64_t)ch * n + i]);
        pp[(uint64_t)ch * n + i] = gl_canon(acc);
    }
}

// PolynomialBatch::from_values / from_coeffs for B units: o.coeffs already holds the values (or coefficients) [B * batch][n]
static int32_t commit_units(Ctx* ctx, int32_t hasher, BOracle& o, bool is_coeffs, bool canonical, const UnitKeys* keys, uint32_t stream_id) {
    const uint64_t n = 1ull << o.log_n, N = n << o.rate_bits;
    const uint32_t cols = o.B * o.batch, lde_bits = o.log_n + o.rate_bits;
    if (!is_coeffs) GL355_TRY(ntt_dev(ctx, o.coeffs, o.log_n, cols, n, true, 0));
    else if (!canonical) GL355_TRY(canon_dev(ctx, o.coeffs, (uint64_t)cols * n));
    GL355_TRY(lde_dev(ctx, o.coeffs, n, o.log_n, o.rate_bits, GL355_COSET_SHIFT, cols, o.lde, N, true));
    if (o.salt) {
        const uint64_t cnt = (uint64_t)GL355_SALT_SIZE * N;
        ProfScope ps(ctx, "salt", cnt * 8 * o.B);
        hipLaunchKernelGGL(salt_units_kernel, dim3((uint32_t)((cnt / 4 + 255) / 256), o.B), dim3(256), 0, ctx->stream, o.salt, lde_bits, *keys, stream_id);
        LAUNCH_CHECK(ctx);
    }
    LeafArgs a;
    memset(&a, 0, sizeof a);
    a.leaves = o.lde; a.n_leaves = (uint64_t)o.B * N; a.leaf_len = o.leaf_len; a.col_major = 1; a.stride = N;
    a.unit_log = lde_bits; a.n_main = o.batch; a.unit_stride = (uint64_t)o.batch * N; a.salt = o.salt; a.salt_unit_stride = (uint64_t)GL355_SALT_SIZE * N;
    return merkle_build_args(ctx, hasher, a, lde_bits - o.cap_height, o.digests, o.cap);
}

// caps [B][n_cap][4] on the device -> dst[u] on the host, each absorbed by its unit's transcript
int32_t observe_caps_units(Ctx* ctx, uint32_t B, uint64_t n_cap, const uint64_t* d_caps, uint64_t* stage, gl355_challenger* ch, uint64_t* const* dst) {
    GL355_HIP(ctx, ctx->d2h(stage, d_caps, (uint64_t)B * n_cap * 32));
    GL355_HIP(ctx, ctx->wait());
    for (uint32_t u = 0; u < B; u++) {
        memcpy(dst[u], stage + (uint64_t)u * n_cap * 4, n_cap * 32);
        gl355_challenger_observe(&ch[u], dst[u], n_cap * 4);
    }
    return GL355_OK;
}

// the permutation argument of n_inst = B * nch instances: unit u's Z_0..Z_{nch-1} and then its partial products go to zbuf + u * z_us
static int32_t zs_units_dev(Ctx* ctx, uint32_t B, uint32_t nch, const uint64_t* wires, uint64_t wires_us, const uint64_t* sigmas, const uint64_t* k_is,
                            uint32_t log_n, uint32_t routed, uint32_t max_degree, const UnitVals& betas, const UnitVals& gammas, uint64_t* zbuf, uint64_t z_us) {
    const uint64_t n = 1ull << log_n;
    const uint32_t n_inst = B * nch, n_chunks = (routed + max_degree - 1) / max_degree;
    Scratch zs_tmp(ctx);
    GL355_TRY(zs_tmp.get((uint64_t)n_inst * (n_chunks + 1) * n * 8));
    ZsArgs za;
    memset(&za, 0, sizeof za);
    za.wires = wires; za.wires_us = wires_us; za.sigmas = sigmas; za.k_is = k_is;
    za.log_n = log_n; za.n_routed = routed; za.max_degree = max_degree; za.nch = nch; za.n_chunks = n_chunks; za.npp = n_chunks - 1;
    za.g = gl_root_of_unity(log_n);
    za.chunk_q = zs_tmp.as<uint64_t>(); za.row_prod = za.chunk_q + (uint64_t)n_inst * n_chunks * n;
    za.zbuf = zbuf; za.z_us = z_us;
    for (uint32_t i = 0; i < MAXB * 4; i++) { za.betas.v[i] = gl_canon(betas.v[i]); za.gammas.v[i] = gl_canon(gammas.v[i]); }
    ProfScope ps(ctx, "zs_partial_products", (uint64_t)n_inst * ((uint64_t)routed * n * 16 + (uint64_t)n_chunks * n * 8));
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    hipLaunchKernelGGL(zs_rows_units_kernel, dim3(blocks, n_inst), dim3(256), 0, ctx->stream, za);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(zs_scan_units_kernel, dim3(n_inst), dim3(1024), 0, ctx->stream, za);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(zs_partials_units_kernel, dim3(blocks, n_inst), dim3(256), 0, ctx->stream, za);
    LAUNCH_CHECK(ctx);
    return GL355_OK;
}
// gl355_zs_partial_products: one unit, one challenge
int32_t zs_partial_products_dev(Ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, const uint64_t* k_is, uint32_t log_n, uint32_t n_routed,
                                uint32_t max_degree, uint64_t beta, uint64_t gamma, uint64_t* z_out, uint64_t* pp_out) {
    const uint64_t n = 1ull << log_n;
    const uint32_t n_chunks = (n_routed + max_degree - 1) / max_degree;
    if (n_chunks > ZS_MAX_CHUNKS) return ctx->fail(GL355_E_UNSUPPORTED, "zs_partial_products: at most 16 partial-product chunks");
    Scratch zb(ctx);       // [Z | pp_0 .. pp_{n_chunks-2}][n], as a unit of the prover lays them out
    GL355_TRY(zb.get((uint64_t)n_chunks * n * 8));
    UnitVals betas, gammas;
    memset(&betas, 0, sizeof betas); memset(&gammas, 0, sizeof gammas);
    betas.v[0] = beta; gammas.v[0] = gamma;
    GL355_TRY(zs_units_dev(ctx, 1, 1, wires, 0, sigmas, k_is, log_n, n_routed, max_degree, betas, gammas, zb.as<uint64_t>(), (uint64_t)n_chunks * n));
    GL355_HIP(ctx, hipMemcpyAsync(z_out, zb.p, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_chunks > 1) GL355_HIP(ctx, hipMemcpyAsync(pp_out, zb.as<uint64_t>() + n, (uint64_t)(n_chunks - 1) * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return GL355_OK;
}

// ---- one run of the lock-step prover: what its stages share --------------------------------------------------------------------------
struct ProveRun {
    Ctx* ctx; const gl355_prover_data* pd; const gl355_circuit& c; const gl355_oracle* cs; const ProveUnit* io;
    // shape
    const uint32_t B, nch, qdf, npp, routed, nw, z_width, lde_bits, cap_h, L, nq_idx;
    const uint64_t n, N, n_cap;
    const int32_t hasher; const bool zk;
    const ProofLayout lay;
    // per unit: transcript, write cursor into its proof, blinding key, public-input hash, query indices
    std::vector<gl355_challenger> ch;
    std::vector<uint64_t*> out;
    std::vector<uint64_t> q_idx;
    UnitKeys keys;
    UnitVals pi_hashes;
    uint64_t* stage = nullptr;      // pinned staging for everything that crosses PCIe (caps, openings, final polynomials, query openings)
    // wires | Z and partial products | quotient chunks, and the four opened oracles as the kernels see them
    BOracle o_w, o_z, o_q;
    OView views[4];
    PolySet all, zsset;             // every polynomial (opened at zeta); the Z polynomials (also at g * zeta)
    // challenges, [u * 4 + k]; zetas: [u*4+0..1] = zeta, [u*4+2..3] = g * zeta
    UnitVals betas, gammas, alphas, zetas, fri_alpha;
    // device buffers that outlive the stage that fills them
    Scratch wires_keep;             // the wire VALUES, needed again for the permutation argument
    Staged s_sig, s_k;
    Scratch evb, colsA, colsB, fri_vals, ob;
    uint64_t *d_idx = nullptr, *d_open = nullptr;      // ob: query indices [B][nq_idx] | the openings below
    uint64_t off_leaf[4], off_sib[4], off_ev = 0, off_fsib = 0, open_words = 0;   // word offsets in d_open (and in `stage` after the copy)

    ProveRun(Ctx* cx, const gl355_prover_data* p, uint32_t b, const ProveUnit* units)
        : ctx(cx), pd(p), c(*p->circuit), cs(p->constants_sigmas), io(units), B(b), nch(c.num_challenges), qdf(c.max_degree), npp(c.num_partial_products),
          routed(c.num_routed_wires), nw(c.num_wires), z_width(nch * (1 + npp)), lde_bits(c.degree_bits + c.rate_bits), cap_h(p->cap_height),
          L(p->n_fri_layers), nq_idx(p->num_queries), n(1ull << c.degree_bits), N(1ull << lde_bits), n_cap(1ull << cap_h), hasher(p->hasher),
          zk(p->zero_knowledge != 0), lay(*p), ch(b), out(b), q_idx((uint64_t)b * p->num_queries), wires_keep(cx), s_sig(cx), s_k(cx), evb(cx), colsA(cx),
          colsB(cx), fri_vals(cx), ob(cx) {
        memset(&pi_hashes, 0, sizeof pi_hashes);
        for (UnitVals* v : {&betas, &gammas, &alphas, &zetas, &fri_alpha}) memset(v, 0, sizeof *v);
    }
    // a committed batch's caps: into every unit's proof and transcript
    int32_t observe_caps(const BOracle& o) {
        GL355_TRY(observe_caps_units(ctx, B, n_cap, o.cap, stage, ch.data(), out.data()));
        for (uint32_t u = 0; u < B; u++) out[u] += n_cap * 4;
        return GL355_OK;
    }
    int32_t commit(BOracle& o, bool is_coeffs, bool canonical, uint32_t salt_stream) { return commit_units(ctx, hasher, o, is_coeffs, canonical, &keys, salt_stream); }
};

// proof headers, one transcript per unit (host) started with the circuit digest and the public-input hash, the staging buffer
static int32_t begin_units(ProveRun& r) {
    for (uint32_t u = 0; u < r.B; u++) {
        uint64_t* hdr = r.io[u].proof;
        hdr[0] = r.lay.words; hdr[1] = r.c.degree_bits; hdr[2] = r.L; hdr[3] = r.nq_idx; hdr[4] = r.io[u].n_public_inputs; hdr[5] = r.zk; hdr[6] = r.cap_h; hdr[7] = r.nch;
        r.out[u] = hdr + 8;
        gl355_challenger_init_h(&r.ch[u], r.hasher);
        gl355_host_hash_no_pad(r.io[u].public_inputs, r.io[u].n_public_inputs, &r.pi_hashes.v[u * 4]);
        gl355_challenger_observe(&r.ch[u], r.pd->circuit_digest, 4);
        gl355_challenger_observe(&r.ch[u], &r.pi_hashes.v[u * 4], 4);
        memcpy(r.keys.k[u].w, r.io[u].key, 32);
    }
    const uint64_t stage_words = (uint64_t)r.B * std::max<uint64_t>({r.n_cap * 4, 2 * (r.lay.n_open + r.nch), 2 * (r.n >> r.lay.fri.total_bits) + 8,
                                                                     (r.lay.query_words - 1) * r.nq_idx, 16});
    return r.ctx->pinned(stage_words * 8, reinterpret_cast<void**>(&r.stage));
}

// 1. witness: the wire values [B][num_wires][n], dense from the caller or scattered from its sparse rows plus the blinding rows
static int32_t stage_witness(ProveRun& r, const uint64_t* d_wires_dense, const uint32_t* row_idx, const uint64_t* rows_host, uint32_t n_rows,
                             uint32_t blind_start, uint32_t n_blind, uint32_t z_start, uint32_t n_z_pairs) {
    Ctx* ctx = r.ctx;
    const uint32_t B = r.B, nw = r.nw;
    const uint64_t n = r.n;
    GL355_TRY(r.o_w.alloc(ctx, B, r.c.degree_bits, r.c.rate_bits, nw, r.zk, r.cap_h));
    GL355_TRY(r.wires_keep.get((uint64_t)B * nw * n * 8));
    uint64_t* wires = r.wires_keep.as<uint64_t>();
    if (d_wires_dense) {
        GL355_HIP(ctx, hipMemcpyAsync(wires, d_wires_dense, (uint64_t)B * nw * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return GL355_OK;
    }
    GL355_HIP(ctx, hipMemsetAsync(wires, 0, (uint64_t)B * nw * n * 8, ctx->stream));
    Scratch rbuf(ctx);
    if (n_rows) {
        const uint64_t per = (uint64_t)n_rows * nw;
        const bool rows_on_device = ptr_is_device(rows_host);       // the batch runtime uploads the next batch's rows on its copy stream
        GL355_TRY(rbuf.get((rows_on_device ? 0 : (uint64_t)B * per * 8) + (uint64_t)n_rows * 4 + 16));
        const uint64_t* d_vals = rows_on_device ? rows_host : rbuf.as<uint64_t>();
        uint32_t* d_idx = reinterpret_cast<uint32_t*>(rbuf.as<uint64_t>() + (rows_on_device ? 0 : (uint64_t)B * per));
        if (!rows_on_device) GL355_HIP(ctx, hipMemcpyAsync(rbuf.p, rows_host, (uint64_t)B * per * 8, hipMemcpyHostToDevice, ctx->stream));
        GL355_HIP(ctx, hipMemcpyAsync(d_idx, row_idx, (uint64_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
        ProfScope ps(ctx, "witness_scatter", (uint64_t)B * per * 16);
        hipLaunchKernelGGL(witness_rows_units_kernel, dim3((uint32_t)((per + 255) / 256), B), dim3(256), 0, ctx->stream, wires, n, nw, d_idx, d_vals, n_rows);
        LAUNCH_CHECK(ctx);
    }
    const uint64_t cnt_b = (uint64_t)n_blind * nw + (uint64_t)n_z_pairs * r.routed;
    if (cnt_b) {
        ProfScope ps(ctx, "witness_blind", (uint64_t)B * cnt_b * 8);
        hipLaunchKernelGGL(witness_blind_units_kernel, dim3((uint32_t)((cnt_b / 4 + 256) / 256), B), dim3(256), 0, ctx->stream, wires, n, nw, r.routed, blind_start,
                           n_blind, z_start, n_z_pairs, r.keys);
        LAUNCH_CHECK(ctx);
    }
    GL355_HIP(ctx, ctx->wait());      // the caller's host row buffers may be reused; rbuf is released after its last use
    return GL355_OK;
}

// 2. wires commitment; beta and gamma of every challenge
static int32_t stage_wires_commit(ProveRun& r) {
    GL355_HIP(r.ctx, hipMemcpyAsync(r.o_w.coeffs, r.wires_keep.p, (uint64_t)r.B * r.nw * r.n * 8, hipMemcpyDeviceToDevice, r.ctx->stream));
    GL355_TRY(r.commit(r.o_w, false, false, GL355_BLIND_STREAM_WIRES_SALT));
    GL355_TRY(r.observe_caps(r.o_w));
    for (uint32_t u = 0; u < r.B; u++) {
        gl355_challenger_squeeze(&r.ch[u], &r.betas.v[u * 4], r.nch);
        gl355_challenger_squeeze(&r.ch[u], &r.gammas.v[u * 4], r.nch);
    }
    return GL355_OK;
}

// 3. permutation argument: Z and partial products of every (unit, challenge), committed; alpha of every challenge
static int32_t stage_permutation(ProveRun& r) {
    Ctx* ctx = r.ctx;
    GL355_TRY(r.o_z.alloc(ctx, r.B, r.c.degree_bits, r.c.rate_bits, r.z_width, r.zk, r.cap_h));
    GL355_TRY(r.s_sig.open(r.pd->sigmas, (uint64_t)r.routed * r.n * 8, 1));
    GL355_TRY(r.s_k.open(r.pd->k_is, (uint64_t)r.routed * 8, 1));
    GL355_TRY(zs_units_dev(ctx, r.B, r.nch, r.wires_keep.as<uint64_t>(), (uint64_t)r.nw * r.n, r.s_sig.as<uint64_t>(), r.s_k.as<uint64_t>(), r.c.degree_bits, r.routed,
                           r.qdf, r.betas, r.gammas, r.o_z.coeffs, (uint64_t)r.z_width * r.n));
    GL355_TRY(r.commit(r.o_z, false, false, GL355_BLIND_STREAM_ZS_SALT));
    r.wires_keep.reset();      // the wire values are not needed any more
    GL355_TRY(r.observe_caps(r.o_z));
    for (uint32_t u = 0; u < r.B; u++) gl355_challenger_squeeze(&r.ch[u], &r.alphas.v[u * 4], r.nch);
    return GL355_OK;
}

// 4. quotient: its values on the coset of size n * 2^qdb, back to coefficients, committed as max_degree chunks; zeta
static int32_t stage_quotient(ProveRun& r) {
    Ctx* ctx = r.ctx;
    uint32_t qdb = 0;
    while ((1u << qdb) < r.qdf) qdb++;
    const uint64_t nq = r.n << qdb;
    GL355_TRY(r.o_q.alloc(ctx, r.B, r.c.degree_bits, r.c.rate_bits, r.nch * r.qdf, r.zk, r.cap_h));
    {
        Scratch qv(ctx);
        GL355_TRY(qv.get((uint64_t)r.B * r.nch * nq * 8));
        GL355_TRY(quotient_units_dev(ctx, &r.c, r.B, r.cs->lde, r.o_w.lde, (uint64_t)r.nw * r.N, r.o_z.lde, (uint64_t)r.z_width * r.N, r.N, r.s_k.as<uint64_t>(),
                                     r.betas.v, r.gammas.v, r.alphas.v, r.pi_hashes.v, qv.as<uint64_t>()));
        GL355_TRY(intt_from_bitrev_dev(ctx, qv.as<uint64_t>(), nq, r.o_q.coeffs, nq, r.c.degree_bits + qdb, r.B * r.nch, GL355_COSET_SHIFT));
    }
    GL355_TRY(r.commit(r.o_q, true, true, GL355_BLIND_STREAM_QUOTIENT_SALT));
    GL355_TRY(r.observe_caps(r.o_q));
    const uint64_t g = gl_root_of_unity(r.c.degree_bits);
    for (uint32_t u = 0; u < r.B; u++) {
        uint64_t* z = &r.zetas.v[u * 4];
        squeeze_ext(&r.ch[u], z);
        z[2] = gl_canon(gl_mul(z[0], g)); z[3] = gl_canon(gl_mul(z[1], g));
    }
    return GL355_OK;
}

// 5. openings (OpeningSet::new): every polynomial at zeta, the Z polynomials at g * zeta; the FRI batching challenge
static int32_t stage_openings(ProveRun& r) {
    Ctx* ctx = r.ctx;
    const uint32_t B = r.B, nch = r.nch, n_open = (uint32_t)r.lay.n_open;
    r.views[0] = view_of(r.cs); r.views[1] = view_of(r.o_w); r.views[2] = view_of(r.o_z); r.views[3] = view_of(r.o_q);
    memset(&r.all, 0, sizeof r.all); memset(&r.zsset, 0, sizeof r.zsset);
    for (int o = 0; o < 4; o++) { r.all.base[o] = r.views[o].coeffs; r.all.us[o] = r.views[o].coeffs_us; r.all.count[o] = r.views[o].batch; }
    r.all.n_sets = 4; r.all.log_n = r.c.degree_bits;
    r.zsset.base[0] = r.views[2].coeffs; r.zsset.us[0] = r.views[2].coeffs_us; r.zsset.count[0] = nch; r.zsset.n_sets = 1; r.zsset.log_n = r.c.degree_bits;
    GL355_TRY(r.evb.get((uint64_t)B * (n_open + nch) * 16));
    EvalArgs<PolySet> ea;
    ea.all = r.all; ea.zs = r.zsset; ea.n_all = n_open; ea.zeta = r.zetas; ea.out = r.evb.as<uint64_t>(); ea.out_us = 2 * (n_open + nch);
    GL355_TRY(eval_polys_units_dev(ctx, B, nch, ea));
    GL355_HIP(ctx, ctx->d2h(r.stage, r.evb.as<uint64_t>(), (uint64_t)B * (n_open + nch) * 16));
    GL355_HIP(ctx, ctx->wait());
    for (uint32_t u = 0; u < B; u++) {
        const uint64_t w = 2ull * (n_open + nch);
        memcpy(r.out[u], r.stage + (uint64_t)u * w, w * 8);
        gl355_challenger_observe(&r.ch[u], r.out[u], w);
        r.out[u] += w;
        squeeze_ext(&r.ch[u], &r.fri_alpha.v[u * 4]);
    }
    return GL355_OK;
}

// 6. DEEP quotient (prove_openings): acc = Q_zeta * alpha^nch + Q_{g zeta}, two base columns per unit in colsA
static int32_t stage_deep(ProveRun& r) {
    Ctx* ctx = r.ctx;
    const uint32_t B = r.B, n_open = (uint32_t)r.lay.n_open;
    const uint64_t n = r.n;
    GL355_TRY(r.colsA.get((uint64_t)B * 2 * n * 8));
    GL355_TRY(r.colsB.get((uint64_t)B * n * 8 + 64));
    GL355_TRY(r.fri_vals.get((uint64_t)B * 2 * r.N * 8));
    const uint64_t n_blocks = (n + DEEP_BLK - 1) / DEEP_BLK;
    Scratch tab(ctx), vbuf(ctx);
    GL355_TRY(tab.get((uint64_t)B * deep_tab_len(n_open) * 16));
    GL355_TRY(vbuf.get((uint64_t)B * (2 * n + 4 * n_blocks + 8) * 8));
    DeepTabArgs ta;
    ta.tab = tab.as<uint64_t>(); ta.n_alpha = n_open; ta.alpha = r.fri_alpha; ta.zeta = r.zetas;
    GL355_TRY(deep_tables_dev(ctx, B, ta));
    GL355_HIP(ctx, hipMemsetAsync(r.colsA.p, 0, (uint64_t)B * 2 * n * 8, ctx->stream));
    DeepArgs da;
    memset(&da, 0, sizeof da);
    da.tab = tab.as<uint64_t>(); da.n_alpha = n_open; da.n = n; da.n_blocks = n_blocks;
    da.v = vbuf.as<uint64_t>(); da.totals = da.v + (uint64_t)B * 2 * n; da.carry = da.totals + (uint64_t)B * 2 * n_blocks;
    da.acc = r.colsA.as<uint64_t>();
    for (int pass = 0; pass < 2; pass++) {
        da.n_polys = pass ? r.nch : n_open; da.point = pass;
        GL355_TRY(deep_units_dev(ctx, B, pass ? r.zsset : r.all, da));
    }
    return GL355_OK;
}

// 7. FRI: the device buffer of every query opening (the four oracles', then the layers'), and the shared tail, which writes caps, final
// polynomial and PoW witness into the proofs and leaves the layer openings in that buffer
static int32_t stage_fri(ProveRun& r) {
    const uint64_t per_oracle = (uint64_t)r.B * r.nq_idx;
    uint64_t woff = 0;
    for (int o = 0; o < 4; o++) {
        r.off_leaf[o] = woff; woff += per_oracle * r.lay.leaf_len[o];
        r.off_sib[o] = woff; woff += per_oracle * r.lay.depth0 * 4;
    }
    r.off_ev = woff; woff += per_oracle * r.lay.fri.ev_total;
    r.off_fsib = woff; woff += per_oracle * r.lay.fri.sib_total;
    r.open_words = woff;
    GL355_TRY(r.ob.get((per_oracle + r.open_words + 16) * 8));
    r.d_idx = r.ob.as<uint64_t>();
    r.d_open = r.d_idx + per_oracle;
    const uint64_t final_words = 2 * (r.n >> r.lay.fri.total_bits);
    FriUnitOut fo[MAXB];
    for (uint32_t u = 0; u < r.B; u++) {
        fo[u].caps = r.out[u]; r.out[u] += (uint64_t)r.L * r.n_cap * 4;
        fo[u].final_poly = r.out[u]; r.out[u] += final_words;
        fo[u].pow_witness = r.out[u]; r.out[u] += 1;
    }
    const FriShape shape{r.c.degree_bits, r.c.rate_bits, r.cap_h, r.pd->pow_bits, r.nq_idx, r.hasher, r.lay.fri};
    return fri_tail_units(r.ctx, shape, r.B, r.colsA.as<uint64_t>(), r.colsB.as<uint64_t>(), r.fri_vals.as<uint64_t>(), r.stage, r.ch.data(), fo, r.q_idx.data(),
                          r.d_idx, r.d_open + r.off_ev, r.d_open + r.off_fsib);
}

// 8. the four oracles' rows and paths at every query; ONE copy brings all query openings back; the proofs' query rounds
static int32_t stage_queries(ProveRun& r) {
    Ctx* ctx = r.ctx;
    const uint32_t B = r.B, nq_idx = r.nq_idx, depth0 = r.lay.depth0;
    for (int o = 0; o < 4; o++) {
        OpenArgs oa;
        oa.o = r.views[o]; oa.N = r.N; oa.lde_bits = r.lde_bits; oa.cap_height = r.cap_h; oa.n_idx = nq_idx; oa.idx = r.d_idx;
        oa.leaves = r.d_open + r.off_leaf[o]; oa.sibs = r.d_open + r.off_sib[o];
        if (oa.o.leaf_len != r.lay.leaf_len[o]) return ctx->fail(GL355_E_HIP, "prove: internal leaf-length mismatch");
        GL355_TRY(open_units_dev(ctx, B, oa));
    }
    GL355_HIP(ctx, ctx->d2h(r.stage, r.d_open, r.open_words * 8));
    GL355_HIP(ctx, ctx->wait());
    const uint64_t* st = r.stage;
    for (uint32_t u = 0; u < B; u++) {
        uint64_t* o_ = r.out[u];
        for (uint32_t q = 0; q < nq_idx; q++) {
            const uint64_t uq = (uint64_t)u * nq_idx + q;
            *o_++ = r.q_idx[uq];
            for (int o = 0; o < 4; o++) {
                const uint32_t ll = r.lay.leaf_len[o];
                memcpy(o_, st + r.off_leaf[o] + uq * ll, (uint64_t)ll * 8); o_ += ll;
                memcpy(o_, st + r.off_sib[o] + uq * depth0 * 4, (uint64_t)depth0 * 32); o_ += (uint64_t)depth0 * 4;
            }
            const FriLayers& fl = r.lay.fri;
            for (uint32_t l = 0; l < r.L; l++) {
                const uint64_t w = 2ull << fl.a[l], d = (uint64_t)fl.depth[l] * 4;
                memcpy(o_, st + r.off_ev + uq * fl.ev_total + fl.ev_off[l], w * 8); o_ += w;
                memcpy(o_, st + r.off_fsib + uq * fl.sib_total + fl.sib_off[l], d * 8); o_ += d;
            }
        }
        if ((uint64_t)(o_ - r.io[u].proof) != r.lay.words) return ctx->fail(GL355_E_HIP, "prove: internal proof-size mismatch");
    }
    return GL355_OK;
}

int32_t prove_units(Ctx* ctx, const gl355_prover_data* pd, uint32_t B, const uint64_t* d_wires_dense, const uint32_t* row_idx,
                    const uint64_t* rows_host, uint32_t n_rows, uint32_t blind_start, uint32_t n_blind, uint32_t z_start, uint32_t n_z_pairs,
                    const ProveUnit* io) {
    if (!pd || !pd->circuit || !pd->constants_sigmas || !pd->sigmas || !pd->k_is || !io || B == 0 || B > MAXB)
        return ctx->fail(GL355_E_INVALID_ARG, "prove: null argument or more than GL355_MAX_UNITS units");
    struct CpuScope {      // thread CPU time of the whole call, for gl355_profile_read's host:cpu_in_prove
        Ctx* c; uint64_t t0;
        explicit CpuScope(Ctx* cx) : c(cx), t0(cx->prof_on ? thread_cpu_ns() : 0) {}
        ~CpuScope() { if (c->prof_on) { c->prove_cpu_ns += thread_cpu_ns() - t0; c->prove_calls++; } }
    } cpu_scope(ctx);
    const gl355_circuit& c = *pd->circuit;
    const gl355_oracle* cs = pd->constants_sigmas;
    const uint32_t nch = c.num_challenges, lde_bits = c.degree_bits + c.rate_bits, cap_h = pd->cap_height, L = pd->n_fri_layers;
    if (nch == 0 || nch > 4 || L > 32 || lde_bits > 27) return ctx->fail(GL355_E_UNSUPPORTED, "prove: unsupported shape");
    FriLayers fl;
    const int32_t fl_rc = fl.init(lde_bits, cap_h, L, pd->fri_arity_bits);
    if (fl_rc == GL355_E_UNSUPPORTED) return ctx->fail(fl_rc, "prove: a FRI layer folds by 2, 4, 8 or 16");
    if (fl_rc != GL355_OK) return ctx->fail(fl_rc, "prove: a FRI arity of 0 bits, or too many FRI layers for the cap height");
    if (fl.total_bits >= c.degree_bits) return ctx->fail(GL355_E_UNSUPPORTED, "prove: the final polynomial must keep at least two coefficients");
    if (lde_bits - fl.total_bits < cap_h + 1u) return ctx->fail(GL355_E_INVALID_ARG, "prove: too many FRI layers for the cap height");
    const uint32_t n_chunks = (c.num_routed_wires + c.max_degree - 1) / c.max_degree;
    if (n_chunks > ZS_MAX_CHUNKS || c.num_partial_products + 1 != n_chunks) return ctx->fail(GL355_E_UNSUPPORTED, "prove: at most 16 partial-product chunks");
    if (cs->log_n != c.degree_bits || cs->rate_bits != c.rate_bits || cs->cap_height != cap_h)
        return ctx->fail(GL355_E_INVALID_ARG, "prove: constants_sigmas oracle does not match the circuit");
    if (pd->hasher != GL355_HASH_POSEIDON && pd->hasher != GL355_HASH_BN254_POSEIDON) return ctx->fail(GL355_E_INVALID_ARG, "prove: unknown hasher");
    if (cs->hasher != pd->hasher) return ctx->fail(GL355_E_INVALID_ARG, "prove: constants_sigmas was committed with another hasher");
    ProveRun r(ctx, pd, B, io);
    for (uint32_t u = 0; u < B; u++) {
        if (!io[u].proof || (!io[u].public_inputs && io[u].n_public_inputs)) return ctx->fail(GL355_E_INVALID_ARG, "prove: null argument");
        if (io[u].proof_capacity_words < r.lay.words) return ctx->fail(GL355_E_INVALID_ARG, "prove: proof buffer too small (see gl355_proof_words)");
    }
    // a constants_sigmas batch of another width than the circuit's would only show as a size mismatch after the whole proof
    if (cs->batch != r.lay.leaf_len[0] || cs->leaf_len != r.lay.leaf_len[0])
        return ctx->fail(GL355_E_HIP, "prove: internal leaf-length mismatch");
    GL355_TRY(begin_units(r));
    GL355_TRY(stage_witness(r, d_wires_dense, row_idx, rows_host, n_rows, blind_start, n_blind, z_start, n_z_pairs));
    GL355_TRY(stage_wires_commit(r));
    GL355_TRY(stage_permutation(r));
    GL355_TRY(stage_quotient(r));
    GL355_TRY(stage_openings(r));
    GL355_TRY(stage_deep(r));
    GL355_TRY(stage_fri(r));
    return stage_queries(r);
}

}  // namespace gl355
