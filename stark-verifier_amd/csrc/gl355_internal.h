// Internal C++ declarations shared by the HIP translation units of libgl355.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gl355.h"
#include "gl_field.cuh"
#include "merkle_common.cuh"
#include "coset_interp.h"
#include "gate_shape.h"
#include "merkle_update_plan.h"

namespace gl355 { struct Ctx; }

// a committed polynomial batch resident in HBM (PolynomialBatch); one allocation from the context pool
struct gl355_oracle {
    struct gl355::Ctx* ctx;
    uint32_t log_n, rate_bits, batch, leaf_len, cap_height;
    uint64_t* coeffs;   // [batch][n]
    uint64_t* lde;      // [leaf_len][N], rows in bit-reversed order (salt columns last)
    uint64_t* digests;  // plonky2 layout
    uint64_t* cap;
    uint64_t n_digests;
    int32_t hasher;     // GL355_HASH_*: the hash of this batch's Merkle tree
};

// MerkleTree { leaves, digests, cap } resident in HBM, updated in place (merkle.hip, merkle_tree.hip); one allocation from the context pool
struct gl355_merkle_tree {
    struct gl355::Ctx* ctx;
    int32_t hasher;         // GL355_HASH_*
    uint64_t n_leaves;
    uint32_t leaf_len, cap_height, sub_bits;      // sub_bits = log2(n_leaves) - cap_height: the layers of a cap subtree = the digests of a path
    uint64_t* digests;      // plonky2 layout; the allocation starts here
    uint64_t* cap;
    uint64_t* leaves;       // row-major [n_leaves][leaf_len]
    uint64_t n_digests;
};

namespace gl355 {

struct Ctx;

// evaluate a HIP call, record the error on the context and return GL355_E_HIP from the caller
#define GL355_HIP(ctx, expr)                                                          \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) return (ctx)->fail_hip(_e, #expr, __FILE__, __LINE__);  \
    } while (0)
#define GL355_TRY(expr)          \
    do {                         \
        int32_t _rc = (expr);    \
        if (_rc != GL355_OK) return _rc; \
    } while (0)
#define LAUNCH_CHECK(ctx) GL355_HIP(ctx, hipGetLastError())

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool external_stream = false;
    std::string err;
    uint64_t* tw_fwd = nullptr;  // omega_{2^14}^e, e < 2^14
    uint64_t* tw_inv = nullptr;  // omega_{2^14}^-e
    // round-major copy for the LDS rounds of radix 2^rho (rho = 3, 4), stored behind the two tables above
    const uint64_t* twr(uint32_t rho, bool inv) const { return tw_fwd + 32768 + ((rho - 3) * 2 + (inv ? 1 : 0)) * 32768; }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // cached two-level power tables, keyed by the list of bases
    struct PowTab { uint64_t* lo; uint64_t* hi; };
    std::map<std::vector<uint64_t>, PowTab> pow_cache;
    std::map<std::vector<uint64_t>, uint64_t*> full_cache;   // full-size multiplier tables (ntt.hip)
    // the table of `words` words under `key`: built once by build(device pointer), one kernel launch on the stream, and kept as long as the context
    template <class Build>
    int32_t cached_table(const std::vector<uint64_t>& key, uint64_t words, const uint64_t** out, Build build) {
        auto it = full_cache.find(key);
        if (it != full_cache.end()) { *out = it->second; return GL355_OK; }
        uint64_t* d = nullptr;
        GL355_HIP(this, hipMalloc((void**)&d, words * 8));
        build(d);
        GL355_HIP(this, hipGetLastError());
        full_cache[key] = d;
        *out = d;
        return GL355_OK;
    }
    int32_t full_pow_table(const uint64_t* lo, const uint64_t* hi, uint32_t n_cosets, uint32_t log_n, const uint64_t** out);
    int32_t full_step_table(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, bool inv, const uint64_t** out);
    int32_t nat_step_table(const uint64_t* lo, const uint64_t* hi, uint32_t l1, uint32_t l2, const uint64_t** out);   // natural -> natural flow
    // table of the 24-bit-limb row pass (ntt_l24.hip): the twiddles between its two radix-64 super-rounds
    int32_t l24_mid_table(const uint64_t** out);

    // trivial caching device allocator (per context => per stream, so reuse is stream-ordered)
    struct Block { void* p; size_t size; bool used; uint64_t serial; };
    std::vector<Block> blocks;
    uint64_t block_serial = 0;        // blocks are numbered in creation order: trim_since(mark) only touches what a phase created itself

    // optional per-kernel timing (gl355_profile_enable): HIP events around every launch group
    struct ProfRec { const char* name; hipEvent_t e0, e1; uint64_t bytes; };
    // host wait for the stream: spinning hipStreamSynchronize (lowest latency) or, with GL355_OPT_BLOCKING_SYNC, a blocking
    // event wait that leaves the CPU to other prover threads (more host threads than cores)
    uint32_t replay_threads = 1;      // GL355_OPT_REPLAY_THREADS
    uint32_t batch_units = 8;         // GL355_OPT_BATCH_UNITS
    uint32_t ntt_single_pass_max_log = 12;   // GL355_OPT_NTT_SINGLE_PASS_MAX_LOG (12..14); 12: +1.8 % units/s over 14 (profiles/r03b_single_pass_ab.txt)
    int blocking_sync = 0;            // GL355_OPT_BLOCKING_SYNC: 0 runtime wait, 1 blocking event, 2 poll + back-off
    hipEvent_t sync_ev = nullptr;
    hipError_t wait();
    hipError_t wait_impl();
    // device -> host copy on the stream; into pageable memory the call itself waits for the stream, so it is accounted like wait()
    hipError_t d2h(void* dst, const void* src, size_t bytes);
    uint64_t wait_ns = 0, wait_calls = 0;   // accumulated by wait() while prof_on
    uint64_t wait_cpu_ns = 0, prove_cpu_ns = 0, prove_calls = 0;   // thread CPU time inside wait() / inside prove_units (waits included)
    uint32_t merkle_lanes_log = 14;   // Merkle levels with <= 2^this nodes use the 16-lanes-per-node kernel (GL355_OPT_MERKLE_LANES_LOG)
    uint32_t merkle_update_full_log = 4;   // gl355_merkle_tree_update rebuilds every level from n_leaves >> this changed leaves on (GL355_OPT_MERKLE_UPDATE_FULL_LOG)
    uint32_t leaf_lanes_log = 16;     // FRI layers of 8- to 32-word leaves with < 2^this leaves over all units hash them 16 lanes per leaf; 0 = never (GL355_OPT_LEAF_LANES_LOG)
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t prof_event();

    int32_t fail(int32_t code, const char* msg);
    int32_t fail_hip(hipError_t e, const char* expr, const char* file, int line);
    int32_t alloc(size_t bytes, void** out);
    void release(void* p);
    // pinned host staging area of the context (grow-only): device -> host copies into it are truly asynchronous
    void* pinned_buf = nullptr;
    size_t pinned_size = 0;
    int32_t pinned(size_t bytes, void** out);
    // batch runtime (batch.cpp): two witness-row slots (pinned host + device) and a copy stream, kept across calls
    void* rt_rows[2] = {nullptr, nullptr};
    void* rt_drows[2] = {nullptr, nullptr};
    void* rt_aux[2] = {nullptr, nullptr};
    size_t rt_bytes = 0, rt_aux_bytes = 0;
    bool device_replay = true;        // GL355_OPT_DEVICE_REPLAY
    hipStream_t rt_copy_stream = nullptr;
    int32_t runtime_buffers(size_t bytes, size_t aux_bytes, uint64_t* rows[2], uint64_t* drows[2], void* aux[2], hipStream_t* copy_stream);
    void runtime_buffers_free();
    void release_all();
    void trim_since(uint64_t mark);   // hipFree every cached block CREATED at or after `mark` (= block_serial at the start of a one-off phase with large
                                      // temporaries, e.g. a keygen) that is not in use; older blocks -- the warmed cache of proofs this context serves -- stay
    // lo[c*4096 + j] = bases[c]^j, hi[c*4096 + j] = bases[c]^(4096 j)
    int32_t pow_tables_multi(const std::vector<uint64_t>& bases, const uint64_t** lo, const uint64_t** hi);
    int32_t pow_tables(uint64_t base, const uint64_t** lo, const uint64_t** hi) {
        return pow_tables_multi(std::vector<uint64_t>{gl_canon(base)}, lo, hi);
    }
};

// RAII: times everything enqueued on the context stream during its lifetime under `name`
struct ProfScope {
    Ctx* ctx; int idx = -1;
    // alg_bytes: the ALGORITHMIC HBM bytes of the launches in this scope (compulsory reads + writes)
    ProfScope(Ctx* c, const char* name, uint64_t alg_bytes = 0) : ctx(c) {
        if (!c->prof_on) return;
        Ctx::ProfRec r{name, c->prof_event(), c->prof_event(), alg_bytes};
        if (!r.e0 || !r.e1) return;
        (void)hipEventRecord(r.e0, c->stream);
        idx = (int)c->prof.size();
        c->prof.push_back(r);
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(ctx->prof[idx].e1, ctx->stream); }
};

// RAII scratch buffer from the context allocator
struct Scratch {
    Ctx* ctx;
    void* p = nullptr;
    explicit Scratch(Ctx* c) : ctx(c) {}
    ~Scratch() { if (p) ctx->release(p); }
    int32_t get(size_t bytes) { return ctx->alloc(bytes, &p); }
    void reset() { if (p) ctx->release(p); p = nullptr; }      // give the block back early (reuse is stream-ordered)
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
};

// A caller buffer that may live on the host or on the device.  Host buffers are staged through a
// scratch allocation (H2D before, D2H after); device buffers are used in place.
struct Staged {
    Ctx* ctx;
    void* user = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
    bool is_host = false, copy_back = false;
    explicit Staged(Ctx* c) : ctx(c) {}
    ~Staged() { if (is_host && dev) ctx->release(dev); }
    // dir: bit0 = read by the kernels (copy in), bit1 = written (copy out at finish())
    int32_t open(const void* ptr, size_t nbytes, int dir);
    int32_t finish();  // enqueue D2H if needed, then sync
    template <typename T> T* as() const { return reinterpret_cast<T*>(dev); }
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
};
bool ptr_is_device(const void* p);

// ---- ntt.hip -------------------------------------------------------------------------------
struct NttPlan {
    const uint64_t* in = nullptr;
    uint64_t* out = nullptr;
    uint64_t in_col_stride = 0, out_col_stride = 0;
    uint32_t log_n = 0, batch = 1;
    bool inverse = false;      // use omega^-1 (no scaling unless `scale` says so)
    bool in_bitrev = false;    // input is in bit-reversed order
    bool out_bitrev = false;   // leave output in bit-reversed order
    uint32_t n_cosets = 1;     // > 1: LDE-style, coset c reads tables c and writes slot coset_slot[c]
    uint64_t coset_ratio = 0;  // != 0: the cosets' bases are base[0] * coset_ratio^c (lets one block run all cosets of a tile)
    uint8_t coset_slot[16] = {0};
    uint64_t coset_out_stride = 0;
    const uint64_t* pre_lo = nullptr;  // multiplier tables on natural-order input index
    const uint64_t* pre_hi = nullptr;
    const uint64_t* post_lo = nullptr; // multiplier tables on natural-order output index
    const uint64_t* post_hi = nullptr;
    uint64_t scale = 1;
};
int32_t ntt_run(Ctx* ctx, const NttPlan& p);
int32_t bitrev_permute(Ctx* ctx, const uint64_t* in, uint64_t* out, uint32_t log_n, uint32_t width,
                       uint64_t in_col_stride, uint64_t out_col_stride, uint32_t batch);
int32_t transpose_cols_to_rows(Ctx* ctx, const uint64_t* in, uint64_t* out, uint64_t rows, uint32_t cols,
                               uint64_t in_col_stride, uint32_t out_row_stride, uint32_t log_rows_brev);
// device-resident building blocks used by the C ABI layer and the commit pipeline
int32_t ntt_dev(Ctx* ctx, uint64_t* data, uint32_t log_n, uint32_t batch, uint64_t stride, bool inverse,
                uint64_t coset_shift /* 0 = none */);
int32_t lde_dev(Ctx* ctx, const uint64_t* coeffs, uint64_t in_stride, uint32_t log_n, uint32_t rate_bits,
                uint64_t shift, uint32_t batch, uint64_t* out, uint64_t out_stride, bool out_bitrev);

// ---- merkle.hip: the launch code of both hash back-ends (kernels: merkle.hip, merkle_bn254.hip); hasher = GL355_HASH_* ---------------
// What the launch code (merkle.hip) needs to know of a back-end; each of the two files fills its own.
struct HasherLaunch {
    void (*permute)(uint64_t*, uint64_t);
    void (*leaves)(LeafArgs);
    void (*two_to_one)(const uint64_t*, const uint64_t*, uint64_t, uint64_t*);
    void (*grind)(PowArgs);
    const char *permute_scope, *leaves_scope, *two_to_one_scope, *grind_scope;      // profile scopes of those four launches
    uint32_t grind_window_log;      // a grinder launch tries at most 2^this candidates per unit
    // the levels above the leaf digests (digest_slot(0, k) of every cap subtree is written), the hasher's level kernels among them
    int32_t (*above_leaves)(Ctx* ctx, uint64_t n_leaves, uint32_t sub_bits, uint64_t* digests, uint64_t* cap);
    // in-place updates: the leaf kernel, the one-lane kernel over a dirty list, their profile scopes, and whether the dirty path may take the
    // 16-lane kernels (merkle_update_level_lanes_kernel, merkle_update_climb_kernel: Poseidon only)
    void (*update_leaves)(UpdateLeafArgs);
    void (*update_level)(uint64_t*, uint64_t*, uint32_t, uint32_t, const uint64_t*, uint64_t);
    const char *update_leaves_scope, *update_level_scope;
    bool lanes16;
};
const HasherLaunch& bn254_hasher_launch();      // merkle_bn254.hip
int32_t permute_dev(Ctx* ctx, int32_t hasher, uint64_t* states, uint64_t count);
// leaves: row-major [n][leaf_len] (row_stride = leaf_len) when col_major == false, else
// column-major: element (leaf i, column c) at leaves[c * col_stride + i].  always_hash: hash_no_pad (no "at most 4 words are their own digest")
int32_t hash_leaves_dev(Ctx* ctx, int32_t hasher, const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, bool col_major,
                        uint64_t col_stride, uint64_t* digests /* n_leaves * 4, linear order */, bool always_hash);
int32_t two_to_one_dev(Ctx* ctx, int32_t hasher, const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t* out);
int32_t merkle_build_dev(Ctx* ctx, int32_t hasher, const uint64_t* leaves, uint64_t n_leaves, uint32_t leaf_len, bool col_major,
                         uint64_t col_stride, uint32_t cap_height, uint64_t* digests, uint64_t* cap);
int32_t merkle_build_args(Ctx* ctx, int32_t hasher, LeafArgs a, uint32_t sub_bits, uint64_t* digests, uint64_t* cap);
// the levels above the leaf digests of a Poseidon tree, for a caller that has written digest_slot(0, k) of every cap subtree itself
int32_t merkle_build_above_leaves(Ctx* ctx, uint64_t n_leaves, uint32_t sub_bits, uint64_t* digests, uint64_t* cap);
// FRI layer leaves of 2 << ab words (ab = 2..4), hashed 16 lanes per leaf straight from the value columns vals [B][2][len_v]: writes the row-major
// leaf array leaves [B][len_v >> ab][2 << ab] and the leaf digests (or the cap entries when sub_bits == 0), then builds the levels above (Poseidon only)
int32_t fri_wide_leaves_tree_dev(Ctx* ctx, uint32_t ab, uint32_t B, const uint64_t* vals, uint64_t len_v, uint64_t* leaves, uint32_t sub_bits,
                                 uint64_t* digests, uint64_t* cap);
// a resident tree's update (p: the sorted unique leaves, the row of rows_host [n_rows][leaf_len] each one takes and, unless `full`, the dirty lists)
// and its batched reads (what = 0: paths, 1: leaves) into host memory; all three wait for the stream
int32_t merkle_update_dev(Ctx* ctx, const gl355_merkle_tree* t, const MerkleUpdatePlan& p, const uint64_t* rows_host, uint64_t n_rows, bool full);
int32_t merkle_tree_gather_dev(Ctx* ctx, const gl355_merkle_tree* t, int what, const uint64_t* indices_host, uint64_t n_idx, uint64_t* out_host);
// the grinder for B <= GL355_MAX_UNITS sponge states at once (pow_grind_dev is its B = 1 call): the smallest passing
// candidate >= start of every unit; `landing` is a host area of B words for the device's answers (pinned: no hidden wait)
int32_t pow_grind_units_dev(Ctx* ctx, int32_t hasher, uint32_t B, const uint64_t* states /* [B][12] */, const uint32_t* pos /* [B] */, uint32_t bits,
                            uint64_t start, uint64_t* landing, uint64_t* const* witness_host /* [B] */);
int32_t pow_grind_dev(Ctx* ctx, int32_t hasher, const uint64_t state[12], uint32_t pos, uint32_t bits, uint64_t start,
                      uint64_t* witness_host);
// host_bn254.cpp
void host_bn254_permute(uint64_t state[12]);
int32_t oracle_open_batch_on(Ctx* ctx, const gl355_oracle* o, const uint64_t* indices, uint32_t n_idx, uint64_t* leaves,
                             uint64_t* siblings);

// ---- fri.hip -------------------------------------------------------------------------------
// Openings, DEEP quotient, FRI fold and query openings exist once, with a unit dimension B: the lock-step prover's stages call the
// *_units_dev routines below, the staged C entry points are their B = 1 calls.
constexpr uint32_t MAXB = GL355_MAX_UNITS;
struct UnitVals { uint64_t v[MAXB * 4]; };      // up to 4 words per unit (challenges, pi hash, extension elements)

// Where a kernel finds polynomial i of unit u (n = 2^log_n coefficients): the template parameter `Polys` of the kernels that read polynomials.
// PolySet: the lock-step prover's, by index, without a pointer table: block o contributes count[o] columns, unit u's at base[o] + u * us[o].
// It lives in the kernel arguments, so the hot path never waits for a pointer load.
struct PolySet {
    const uint64_t* base[4]; uint64_t us[4]; uint32_t count[4];
    uint32_t n_sets, log_n;
    GL_DEV const uint64_t* ptr(uint32_t u, uint32_t i) const {
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if ((uint32_t)k + 1 < n_sets && i >= count[o]) { i -= count[o]; o++; }
        return base[o] + (uint64_t)u * us[o] + ((uint64_t)i << log_n);
    }
};
// PolyTable: the staged entry points', which take any list of (oracle, column): a pointer table on the device, one unit
struct PolyTable {
    const uint64_t* const* p; uint32_t log_n;
    GL_DEV const uint64_t* ptr(uint32_t, uint32_t i) const { return p[i]; }
};

// OpeningSet::new: polynomial i < n_all of `all` at zeta_u, polynomial i - n_all of `zs` at g * zeta_u; out[u][i] (extension)
template <class Polys>
struct EvalArgs { Polys all, zs; uint32_t n_all; UnitVals zeta /* [u*4+0..1] = zeta, [u*4+2..3] = g * zeta */; uint64_t* out; uint32_t out_us; };
template <class Polys> int32_t eval_polys_units_dev(Ctx* ctx, uint32_t B, uint32_t n_zs, const EvalArgs<Polys>& a);

constexpr int DEEP_BLK = 256;  // coefficients per workgroup in the division scan
// per-unit tables of the two opening batches (point A = zeta, point B = g * zeta), ext elements:
//   [0, n_alpha]            alpha^i, i <= n_alpha (n_alpha = number of polynomials of the larger batch)
//   then for A and for B:   z^(2^s), s < 8 | z^e, e <= DEEP_BLK
GL_HD uint32_t deep_tab_len(uint32_t n_alpha) { return (n_alpha + 1) + 2 * (8 + DEEP_BLK + 1); }
struct DeepTabArgs { uint64_t* tab; uint32_t n_alpha; UnitVals alpha /* [u*4+0..1] */, zeta /* as EvalArgs */; };
int32_t deep_tables_dev(Ctx* ctx, uint32_t B, const DeepTabArgs& a);
struct DeepArgs {
    uint32_t n_polys, n_alpha, point;   // point 0 = zeta tables, 1 = g * zeta tables
    const uint64_t* tab;
    uint64_t n, n_blocks;
    uint64_t* v;        // [B][n] ext scratch
    uint64_t* totals;   // [B][n_blocks] ext
    uint64_t* carry;    // [B][n_blocks] ext
    uint64_t* acc;      // [B][2][n]: the accumulated quotient as two base-field columns (what the F_p^2 LDE takes)
};
template <class Polys> struct DeepScanArgs { Polys polys; DeepArgs a; };      // what the one DEEP kernel that reads polynomials takes
// acc = acc * alpha^n_polys + (sum_i alpha^i polys_i) / (X - z_point), for every unit
template <class Polys> int32_t deep_units_dev(Ctx* ctx, uint32_t B, const Polys& polys, const DeepArgs& a);

// fold of B units' coefficient columns cols [B][2][len] by 2^arity_bits with beta_u = betas[u*4+0..1] (canonical) into out [B][2][len >> arity_bits]
int32_t fri_fold_units_dev(Ctx* ctx, uint32_t arity_bits, uint32_t B, const uint64_t* cols, uint64_t len, const UnitVals& betas, uint64_t* out);

// one oracle as the kernels see it: unit u's data at base + u * stride (stride 0 = shared by all units).  Columns c < batch of a leaf
// are in lde, the other leaf_len - batch in salt
struct OView {
    const uint64_t* coeffs; uint64_t coeffs_us;
    const uint64_t* lde; uint64_t lde_us;
    const uint64_t* salt; uint64_t salt_us;
    const uint64_t* digests; uint64_t dig_us;
    uint32_t batch, leaf_len;
};
// row idx[u][q] of unit u's column-major LDE (+ salt segment) and its Merkle path, dense per-unit outputs
struct OpenArgs { OView o; uint64_t N; uint32_t lde_bits, cap_height, n_idx; const uint64_t* idx /* [B][n_idx] */; uint64_t* leaves; uint64_t* sibs; };
int32_t open_units_dev(Ctx* ctx, uint32_t B, const OpenArgs& a);

// the staged forms: interleaved F_p^2 in and out, any (oracle, column) list, challenges in any representation
int32_t deep_batch_dev(Ctx* ctx, const uint64_t* const* poly_ptrs_host, uint32_t n_polys, uint32_t log_n,
                       const uint64_t alpha[2], const uint64_t z[2], uint64_t* acc /* n ext */);
int32_t eval_polys_ext_dev(Ctx* ctx, const uint64_t* const* poly_ptrs_host, uint32_t n_polys, uint32_t log_n,
                           const uint64_t z[2], uint64_t* out_dev);
int32_t fri_fold_dev(Ctx* ctx, const uint64_t* coeffs, uint64_t n, uint32_t arity_bits, const uint64_t beta[2], uint64_t* out);
int32_t fri_layer_leaves_dev(Ctx* ctx, const uint64_t* values, uint64_t n, uint64_t* leaves);
int32_t lde_ext_dev(Ctx* ctx, const uint64_t* coeffs, uint32_t log_n, uint32_t rate_bits, uint64_t shift, uint64_t* out,
                    bool out_bitrev);
int32_t ext_split_dev(Ctx* ctx, const uint64_t* ext, uint64_t n, uint64_t* c0, uint64_t* c1);
int32_t ext_join_dev(Ctx* ctx, const uint64_t* c0, const uint64_t* c1, uint64_t n, uint64_t* ext);
int32_t field_batch_dev(Ctx* ctx, int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n);
int32_t zs_partial_products_dev(Ctx* ctx, const uint64_t* wires, const uint64_t* sigmas, const uint64_t* k_is,
                                uint32_t log_n, uint32_t n_routed, uint32_t max_degree, uint64_t beta, uint64_t gamma,
                                uint64_t* z_out, uint64_t* pp_out);
int32_t canon_dev(Ctx* ctx, uint64_t* a, uint64_t n);
int32_t intt_from_bitrev_dev(Ctx* ctx, const uint64_t* in, uint64_t in_stride, uint64_t* out, uint64_t out_stride,
                             uint32_t log_n, uint32_t batch, uint64_t coset_shift);
int32_t quotient_dev(Ctx* ctx, const gl355_circuit* c, const uint64_t* cs_lde, const uint64_t* wires_lde,
                     const uint64_t* zs_lde, uint64_t lde_stride, const uint64_t* k_is_dev, const uint64_t* betas,
                     const uint64_t* gammas, const uint64_t* alphas, const uint64_t pi_hash[4], uint64_t* out_values);
Ctx* ctx_of(gl355_ctx* h);
uint64_t thread_cpu_ns();

// ---- prover_batch.hip: CircuitData::prove for B lock-step units of one circuit ---------------------------------------------
struct BlindKey;
struct ProveUnit {
    const uint64_t* public_inputs; uint32_t n_public_inputs;
    uint32_t key[8];                       // the unit's blinding key (blinding.cuh BlindKey words)
    uint64_t* proof; uint64_t proof_capacity_words;
};
// dense witness: d_wires_dense = [B][num_wires][n] on the device; sparse: rows_host = [B][n_rows][num_wires] (host) of circuit rows
// row_idx[r], blinding rows generated on the device from each unit's key
int32_t prove_units(Ctx* ctx, const gl355_prover_data* pd, uint32_t B, const uint64_t* d_wires_dense, const uint32_t* row_idx,
                    const uint64_t* rows_host, uint32_t n_rows, uint32_t blind_start, uint32_t n_blind, uint32_t z_start, uint32_t n_z_pairs,
                    const ProveUnit* io);
uint64_t tape_validate(const uint64_t* tape, uint64_t n_ops, uint64_t n_inputs, uint64_t n_words, uint32_t num_wires);
int32_t tape_replay_dev(hipStream_t stream, const uint64_t* d_tape, const uint64_t* d_seg_start, uint64_t n_seq, uint32_t n_segs, uint32_t n_units,
                        const uint64_t* d_inputs, uint64_t n_inputs, uint64_t* d_rows, uint64_t n_words, const uint64_t* d_pi_pos, uint32_t n_pi,
                        uint64_t* d_status, uint64_t* d_pis);
// witness rows of n_units units generated on the device on `stream` (inputs: host [units][n_inputs]); d_aux: device scratch of
// circuit_replay_aux_bytes(); the call returns after the stream has finished (polling, no spinning)
uint64_t circuit_replay_aux_bytes(const gl355_circuit_handle* ch, uint32_t n_units);
int32_t circuit_replay_units_dev(const gl355_circuit_handle* ch, int device, hipStream_t stream, uint32_t n_units, const uint64_t* inputs, uint64_t* d_rows,
                                 void* d_aux, uint64_t* pis_out, uint64_t* failed_unit, uint64_t* failed_op, void* h_aux = nullptr);
uint64_t circuit_rows_words(const gl355_circuit_handle* ch);
int32_t circuit_replay_units(const gl355_circuit_handle* ch, uint32_t threads, uint32_t n_units, const uint64_t* inputs, uint64_t* rows, uint64_t* pis_out,
                             uint64_t* failed_unit, uint64_t* failed_op);
int32_t resolve_blinding_key_words(Ctx* ctx, const uint8_t* key, uint32_t out[8]);

// The commit-phase layers of one FRI proof as numbers: the ONE description of "which leaf does layer l open and how long is its
// path" that gl355_fri_prove, the lock-step prover's buffers and assembly loop, gl355_proof_words and gl355_verify all read.
// Layer l folds by A_l = 2^a[l]; s[l] = a[0] + .. + a[l]; its tree has N >> s[l] leaves of A_l extension values (2 A_l words), a query
// opens leaf x_index >> s[l] with a path of depth[l] = lde_bits - s[l] - cap_height digests.
struct FriLayers {
    uint32_t n = 0, total_bits = 0;          // layers; s[n - 1] (0 without layers)
    uint32_t a[32], s[32], depth[32];
    uint64_t ev_off[32], ev_total = 0;       // words: where layer l's 2 A_l words start inside one query's layer evaluations; their sum
    uint64_t sib_off[32], sib_total = 0;     // words: the same for the layer paths
    // arity_bits == NULL: every layer folds by 2.  GL355_OK, or the code of the first layer that cannot be built (no message: the caller names itself)
    int32_t init(uint32_t lde_bits, uint32_t cap_height, uint32_t n_layers, const uint32_t* arity_bits) {
        n = 0; total_bits = 0; ev_total = 0; sib_total = 0;
        if (n_layers > 32) return GL355_E_UNSUPPORTED;
        for (uint32_t l = 0; l < n_layers; l++) {
            const uint32_t al = arity_bits ? arity_bits[l] : 1;
            if (al == 0) return GL355_E_INVALID_ARG;
            if (al > GL355_MAX_FRI_ARITY_BITS) return GL355_E_UNSUPPORTED;
            total_bits += al;
            if (total_bits > lde_bits || lde_bits - total_bits < cap_height) return GL355_E_INVALID_ARG;   // a layer narrower than the cap
            a[l] = al; s[l] = total_bits; depth[l] = lde_bits - total_bits - cap_height;
            ev_off[l] = ev_total; ev_total += 2ull << al;
            sib_off[l] = sib_total; sib_total += (uint64_t)depth[l] * 4;
        }
        n = n_layers;
        return GL355_OK;
    }
};

// The flat proof (layout in include/gl355.h) as numbers, computed once from the prover data: gl355_proof_words, the prover's
// staging and device open buffers and its assembly loop all read this.
struct ProofLayout {
    uint32_t leaf_len[4];              // constants_sigmas | wires | Z and partial products | quotient chunks (salt included)
    uint32_t depth0;                   // digests of a path in one of those four trees
    FriLayers fri;                     // the commit-phase layers; fri_rc != GL355_OK: the arities cannot be built (words = 0)
    int32_t fri_rc;
    uint64_t n_open;                   // polynomials opened at zeta (the num_challenges Z polynomials also at g * zeta)
    uint64_t query_words;              // index | 4 x (leaf, path) | n_fri_layers x (2^a_l evaluations, path)
    uint64_t words;                    // the whole proof, header included
    explicit ProofLayout(const gl355_prover_data& pd) {
        const gl355_circuit& c = *pd.circuit;
        const uint32_t nch = c.num_challenges, lde_bits = c.degree_bits + c.rate_bits, L = pd.n_fri_layers;
        const uint64_t n_cap = 1ull << pd.cap_height;
        const uint32_t widths[4] = {c.num_selectors + c.num_constants + c.num_routed_wires, c.num_wires, nch * (1 + c.num_partial_products), nch * c.max_degree};
        depth0 = lde_bits - pd.cap_height;
        fri_rc = fri.init(lde_bits, pd.cap_height, L, pd.fri_arity_bits);
        n_open = 0;
        query_words = 1 + fri.ev_total + fri.sib_total;
        for (int o = 0; o < 4; o++) {
            n_open += widths[o];
            leaf_len[o] = widths[o] + ((pd.zero_knowledge && o > 0) ? GL355_SALT_SIZE : 0);
            query_words += leaf_len[o] + (uint64_t)depth0 * 4;
        }
        words = 8 + 3 * n_cap * 4                              // header; wires / zs / quotient caps
                + 2 * (n_open + nch)                           // openings (ext)
                + (uint64_t)L * n_cap * 4                      // commit-phase caps
                + 2 * ((1ull << c.degree_bits) >> fri.total_bits) + 1   // final polynomial (ext), PoW witness
                + query_words * pd.num_queries;
        if (fri_rc != GL355_OK) words = 0;
    }
};

// ---- the FRI tail of a proof (fri.hip): commit phase, final polynomial, proof of work, query indices, layer openings ----
struct FriShape { uint32_t log_n, rate_bits, cap_height, pow_bits, n_queries; int32_t hasher; FriLayers layers; };
struct FriUnitOut { uint64_t* caps /* [n_layers][2^cap_height][4] */; uint64_t* final_poly /* [n >> total_bits] ext */; uint64_t* pow_witness; };
// words of host staging fri_tail_units needs
static inline uint64_t fri_tail_stage_words(const FriShape& s, uint32_t B) {
    return (uint64_t)B * std::max<uint64_t>({4ull << s.cap_height, 2 * ((1ull << s.log_n) >> s.layers.total_bits), 1});
}
// B units, each a polynomial of n = 2^log_n F_p^2 coefficients held as two base columns: cols [B][2][n] (consumed), cols2 [B][n] and
// vals [B][2][n << rate_bits] are work space.  ch[u] is advanced as the verifier replays it; caps, final polynomial and PoW witness go
// to out[u], the query indices to q_idx [B][n_queries] (host, must outlive the stream's work) and d_idx (device); the layer openings
// stay on the device: d_evals [B][n_queries][layers.ev_total], d_sibs [B][n_queries][layers.sib_total].  `stage`: pinned host.
int32_t fri_tail_units(Ctx* ctx, const FriShape& s, uint32_t B, uint64_t* cols, uint64_t* cols2, uint64_t* vals, uint64_t* stage,
                       gl355_challenger* ch, const FriUnitOut* out, uint64_t* q_idx, uint64_t* d_idx, uint64_t* d_evals, uint64_t* d_sibs);
// caps [B][n_cap][4] on the device -> dst[u] on the host, each absorbed by its unit's transcript (prover_batch.hip)
int32_t observe_caps_units(Ctx* ctx, uint32_t B, uint64_t n_cap, const uint64_t* d_caps, uint64_t* stage, gl355_challenger* ch, uint64_t* const* dst);
// two canonical words of a transcript's next extension challenge
static inline void squeeze_ext(gl355_challenger* ch, uint64_t* v) {
    gl355_challenger_squeeze(ch, v, 2);
    v[0] = gl_canon(v[0]); v[1] = gl_canon(v[1]);
}
int32_t quotient_units_dev(Ctx* ctx, const gl355_circuit* c, uint32_t B, const uint64_t* cs_lde, const uint64_t* wires_lde, uint64_t wires_us,
                           const uint64_t* zs_lde, uint64_t zs_us, uint64_t lde_stride, const uint64_t* k_is_dev, const uint64_t* betas /* [B][4] */,
                           const uint64_t* gammas, const uint64_t* alphas, const uint64_t* pi_hashes /* [B][4] */, uint64_t* out_values /* [B][nch][nq] */);

// verifier.cpp: the constraints of one gate at an opened point, in the extension field; false = the gate does not fit num_wires / num_constants
bool verifier_eval_gate(const gl355_gate& gt, const gl2* consts, const gl2* w, const uint64_t pi_hash[4], uint32_t num_wires, uint32_t num_constants,
                        std::vector<gl2>& c);

static inline uint32_t log2_u64(uint64_t n) { uint32_t l = 0; while ((1ull << l) < n) l++; return l; }
static inline uint32_t host_brev(uint32_t x, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

}  // namespace gl355
