// Does this witness satisfy this circuit, and if not, where?  halo2's MockProver::run(..).assert_satisfied() -- all of the reference's
// verify_inside_snark_mock (src/plonky2_verifier/verifier_api.rs:34-52), the first step of verify_inside_snark (:72-73) and every chip test
// (goldilocks_chip.rs, arithmetic_chip.rs, poseidon_bn254_chip.rs, all_chip.rs, gate_test.rs) -- on the device, from the descriptor blob alone:
// no SRS, no key.  Semantics follow MockProver::verify (include/gl355.h has the contract):
//   gates        the gate program, evaluated exactly at every usable row, one poison bit per register beside the 12-register file; every EMIT
//                is tested for zero and the verdicts of a wave leave as one 64-bit ballot word per polynomial -- no atomics
//   lookups      exact membership of the input tuple among the table's usable rows: an open-addressing hash set of table ROW INDICES in HBM,
//                equality decided on the full tuples, then one probe per input row
//   permutation  one gather per cell through `mapping`
//   output       popcount / scan / ordered extraction over the bitmaps, which lie in (kind, index, row) order: the same records on every run
// All values are canonical Montgomery scalars, so equality of field elements is equality of words.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <type_traits>

#include "gl355_internal.h"
#include "plonk_desc.h"
#include "plonk_regs.cuh"

using namespace gl355;

namespace gl355 {

constexpr uint32_t CHK_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t CHK_WORDS_PER_LANE = 8, CHK_WORDS_PER_BLOCK = 256 * CHK_WORDS_PER_LANE;

// plain integers -> canonical Montgomery
__global__ void chk_to_mont_kernel(const uint64_t* in, uint64_t* out, uint64_t n) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    store256(out + 4 * i, m_canon<F_R>(m_from_int<F_R>(load256(in + 4 * i))));
}

// ---- the row-domain evaluator -------------------------------------------------------------------------------------------------------
// The programs and the register file of plk_eval_kernel (plonk_kernels.cuh), on the value domain (a rotation is an index shift mod n), with
// one poison bit per register: an advice query that lands in a row >= usable is poisoned (the prover overwrites those rows), poison goes
// through ADD / SUB / NEG / MOV, and through MUL unless the other operand is an unpoisoned zero (halo2's Value::Real(0) * Poison = Real(0): a
// switched-off selector silences its gate).
// Gate mode (out == nullptr): EMIT number e of row i sets bit i of fail[e] (non-zero, not poisoned) or of poisoned[e].
// Tuple mode: EMIT number e stores its canonical value to out[e][i]; poisoned (one bitmap) gets the rows with any poisoned element.
// Lanes of rows >= usable stay in the wave for the ballots: they run the program on row 0 (every load in range) with their ballots and stores masked.
struct ChkEvalArgs {
    const uint32_t* code;
    uint32_t n_instr, n_emit;
    const uint64_t* consts;
    const uint64_t* const* cols[3];
    const int32_t* q_col[3];
    const int32_t* q_rot[3];
    uint64_t n, usable, words;       // words: 64-bit words of one bitmap
    unsigned long long *fail, *poisoned;
    uint64_t* out;
};
GL_DEV u256 chk_operand(const ChkEvalArgs& a, const PlkRegs& f, uint32_t pbits, uint32_t operand, uint64_t row, bool& poison) {
    const uint32_t kind = operand >> 24, idx = operand & 0xFFFFFFu;
    if (kind == PLK_K_REG) { poison = (pbits >> idx) & 1u; return plk_reg_read(f, idx); }
    poison = false;
    if (kind == PLK_K_CONST) return load256(a.consts + 4 * idx);
    const uint32_t kd = kind - PLK_K_ADVICE;
    const uint64_t r = plk_rotated(row, a.q_rot[kd][idx], a.n, 0, 0);
    poison = kd == 0 && r >= a.usable;
    return load256(a.cols[kd][a.q_col[kd][idx]] + 4 * r);
}
__global__ void __launch_bounds__(256) chk_eval_kernel(ChkEvalArgs a) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const bool live = i < a.usable;
    const uint64_t row = live ? i : 0;
    const uint64_t word = i >> 6;                            // a wave is 64 consecutive rows
    const bool writer = (threadIdx.x & 63u) == 0 && word < a.words;
    PlkRegs f;
#define PLK_ZERO(K) f.r##K = u_zero();
    PLK_REG_CASES(PLK_ZERO)
#undef PLK_ZERO
    uint32_t pbits = 0, e = 0;
    bool any_poison = false;
#pragma unroll 1
    for (uint32_t pc = 0; pc < a.n_instr; pc++) {
        const uint32_t op = a.code[4 * pc], dst = a.code[4 * pc + 1], oa = a.code[4 * pc + 2], ob = a.code[4 * pc + 3];
        bool px, py = false;
        const u256 x = chk_operand(a, f, pbits, oa, row, px);
        if (op == PLK_OP_EMIT) {
            if (e < a.n_emit) {
                if (a.out) {
                    if (live) store256(a.out + 4 * ((uint64_t)e * a.n + i), m_canon<F_R>(x));
                    any_poison = any_poison || px;
                } else {
                    const unsigned long long bad = __ballot(live && !px && !m_is_zero<F_R>(x)), poi = __ballot(live && px);
                    if (writer) { a.fail[(uint64_t)e * a.words + word] = bad; a.poisoned[(uint64_t)e * a.words + word] = poi; }
                }
            }
            e++;
            continue;
        }
        u256 v;
        bool pv = px;
        if (op == PLK_OP_NEG) v = fr_neg(x);
        else if (op == PLK_OP_MOV) v = x;
        else {
            const u256 y = chk_operand(a, f, pbits, ob, row, py);
            if (op == PLK_OP_MUL) {
                v = m_mul<F_R>(x, y);
                pv = (px || py) && !((!px && m_is_zero<F_R>(x)) || (!py && m_is_zero<F_R>(y)));
            } else {
                v = op == PLK_OP_ADD ? m_add<F_R>(x, y) : m_sub<F_R>(x, y);
                pv = px || py;
            }
        }
        plk_reg_write(f, dst, v);
        pbits = (pbits & ~(1u << dst)) | ((pv ? 1u : 0u) << dst);
    }
    if (a.out) {
        const unsigned long long poi = __ballot(live && any_poison);
        if (writer) a.poisoned[word] = poi;
    }
}

// ---- lookups: exact membership ---------------------------------------------------------------------------------------------------------
// a tuple of `w` scalars: element e of row i at base[4 (e n + i)]
struct ChkTuples { const uint64_t* base; const unsigned long long* poisoned /* or null: no row is */; };
GL_DEV bool chk_bit(const unsigned long long* bm, uint64_t i) { return bm && ((bm[i >> 6] >> (i & 63)) & 1ull); }
GL_DEV uint64_t chk_hash(const uint64_t* base, uint32_t w, uint64_t n, uint64_t row) {
    uint64_t hsh = 0x9E3779B97F4A7C15ull;
    for (uint32_t e = 0; e < w; e++) {
        const uint64_t* p = base + 4 * ((uint64_t)e * n + row);
#pragma unroll
        for (int l = 0; l < 4; l++) { hsh = (hsh ^ p[l]) * 0xFF51AFD7ED558CCDull; hsh ^= hsh >> 32; }
    }
    return hsh;
}
GL_DEV bool chk_tuple_eq(const uint64_t* a, uint64_t ra, const uint64_t* b, uint64_t rb, uint32_t w, uint64_t n) {
    uint64_t diff = 0;
    for (uint32_t e = 0; e < w; e++) {
        const uint64_t *p = a + 4 * ((uint64_t)e * n + ra), *q = b + 4 * ((uint64_t)e * n + rb);
        diff |= (p[0] ^ q[0]) | (p[1] ^ q[1]) | (p[2] ^ q[2]) | (p[3] ^ q[3]);
    }
    return diff == 0;
}
// slots[2^log_slots] hold table row indices.  A row reads its slot BEFORE it tries to claim it: the reference's table is 2^16 values padded
// to 2^23 rows with one value, and millions of compare-and-swaps on one word would serialise; a read of a taken slot costs a cached compare.
// Which of several equal rows holds a slot is of no consequence: only membership is asked.
__global__ void __launch_bounds__(256) chk_table_insert_kernel(ChkTuples t, uint32_t w, uint64_t n, uint64_t usable, uint32_t* slots, uint32_t log_slots) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= usable || chk_bit(t.poisoned, i)) return;       // poisoned table tuples are not part of the table
    const uint64_t mask = (1ull << log_slots) - 1;
    uint64_t s = chk_hash(t.base, w, n, i) & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        uint32_t cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == CHK_EMPTY) {
            cur = atomicCAS(slots + s, CHK_EMPTY, (uint32_t)i);
            if (cur == CHK_EMPTY) return;
        }
        if (cur < usable && chk_tuple_eq(t.base, cur, t.base, i, w, n)) return;
    }
}
__global__ void __launch_bounds__(256) chk_lookup_probe_kernel(ChkTuples in, ChkTuples t, uint32_t w, uint64_t n, uint64_t usable, const uint32_t* slots, uint32_t log_slots,
                                                               uint64_t words, unsigned long long* fail, unsigned long long* aux) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const bool live = i < usable;
    const bool poison = live && chk_bit(in.poisoned, i);
    bool found = false;
    if (live && !poison) {
        const uint64_t mask = (1ull << log_slots) - 1;
        uint64_t s = chk_hash(in.base, w, n, i) & mask;
        for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
            const uint32_t cur = slots[s];
            if (cur == CHK_EMPTY || cur >= usable) break;
            if (chk_tuple_eq(t.base, cur, in.base, i, w, n)) { found = true; break; }
        }
    }
    const unsigned long long bad = __ballot(live && !found), poi = __ballot(poison);
    const uint64_t word = i >> 6;
    if ((threadIdx.x & 63u) == 0 && word < words) { fail[word] = bad; aux[word] = poi; }
}

// ---- copy constraints ------------------------------------------------------------------------------------------------------------------
// blockIdx.y = column position j: cell (j, i) against the cell mapping[j][i] names
__global__ void __launch_bounds__(256) chk_copy_kernel(const uint32_t* mapping /* [n_perm][n][2] */, const uint64_t* const* cols /* [n_perm] */, uint64_t n, uint32_t n_perm,
                                                       uint64_t words, unsigned long long* fail /* [n_perm][words] */, uint32_t* out_of_range) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint32_t j = blockIdx.y;
    bool bad = false;
    if (i < n) {
        const uint32_t cj = mapping[2 * (j * n + i)], ci = mapping[2 * (j * n + i) + 1];
        if (cj >= n_perm || ci >= n) atomicOr(out_of_range, 1u);
        else bad = !u_eq(load256(cols[j] + 4 * i), load256(cols[cj] + 4 * (uint64_t)ci));
    }
    const unsigned long long b = __ballot(bad);
    const uint64_t word = i >> 6;
    if ((threadIdx.x & 63u) == 0 && word < words) fail[(uint64_t)j * words + word] = b;
}

// ---- count and ordered extraction ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) chk_count_kernel(const unsigned long long* bm, uint64_t total_words, uint32_t* block_sums) {
    __shared__ uint32_t sh[256];
    const uint64_t w0 = (uint64_t)blockIdx.x * CHK_WORDS_PER_BLOCK;
    uint32_t c = 0;
    for (uint32_t j = 0; j < CHK_WORDS_PER_LANE; j++) {
        const uint64_t w = w0 + threadIdx.x + 256ull * j;
        if (w < total_words) c += (uint32_t)__popcll(bm[w]);
    }
    sh[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t st = 128; st; st >>= 1) {
        if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sh[0];
}
// one block: offsets[b] = sum of block_sums before b, *total = all
__global__ void __launch_bounds__(256) chk_scan_kernel(const uint32_t* block_sums, uint64_t n_blocks, unsigned long long* offsets, unsigned long long* total) {
    __shared__ unsigned long long sh[256];
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        const unsigned long long mine = b < n_blocks ? block_sums[b] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t st = 1; st < 256; st <<= 1) {
            const unsigned long long add = threadIdx.x >= st ? sh[threadIdx.x - st] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < n_blocks) offsets[b] = carry + sh[threadIdx.x] - mine;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
struct ChkExtractArgs {
    const unsigned long long *bm, *lookup_aux /* [n_lookups][words] */, *offsets;
    uint64_t total_words, words, n, capacity;
    uint32_t n_polys, n_lookups;
    const uint32_t* mapping;
    uint32_t* records;               // [capacity][4]
};
// a lane takes CHK_WORDS_PER_LANE consecutive words, so positions ascend with (segment, row)
__global__ void __launch_bounds__(256) chk_extract_kernel(ChkExtractArgs a) {
    __shared__ uint32_t sh[256];
    const unsigned long long base = a.offsets[blockIdx.x];
    if (base >= a.capacity) return;
    const uint64_t w0 = (uint64_t)blockIdx.x * CHK_WORDS_PER_BLOCK + (uint64_t)threadIdx.x * CHK_WORDS_PER_LANE;
    uint32_t c = 0;
    for (uint32_t j = 0; j < CHK_WORDS_PER_LANE; j++) if (w0 + j < a.total_words) c += (uint32_t)__popcll(a.bm[w0 + j]);
    sh[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t st = 1; st < 256; st <<= 1) {
        const uint32_t add = threadIdx.x >= st ? sh[threadIdx.x - st] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long pos = base + sh[threadIdx.x] - c;
    for (uint32_t j = 0; j < CHK_WORDS_PER_LANE && c; j++) {
        const uint64_t w = w0 + j;
        if (w >= a.total_words) break;
        unsigned long long bits = a.bm[w];
        const uint64_t seg = w / a.words, wi = w % a.words;
        while (bits) {
            if (pos >= a.capacity) return;
            const uint32_t bit = (uint32_t)__ffsll(bits) - 1;
            bits &= bits - 1;
            const uint64_t row = wi * 64 + bit;
            uint32_t kind, index, aux = 0;
            if (seg < a.n_polys) { kind = GL355_PLONK_FAIL_GATE; index = (uint32_t)seg; }
            else if (seg < 2ull * a.n_polys) { kind = GL355_PLONK_FAIL_GATE_POISONED; index = (uint32_t)(seg - a.n_polys); }
            else if (seg < 2ull * a.n_polys + a.n_lookups) {
                kind = GL355_PLONK_FAIL_LOOKUP; index = (uint32_t)(seg - 2ull * a.n_polys);
                aux = (uint32_t)((a.lookup_aux[(uint64_t)index * a.words + wi] >> bit) & 1ull);
            } else {
                kind = GL355_PLONK_FAIL_PERMUTATION; index = (uint32_t)(seg - 2ull * a.n_polys - a.n_lookups);
                aux = a.mapping[2 * ((uint64_t)index * a.n + row)];
            }
            uint32_t* r = a.records + 4 * pos;
            r[0] = kind; r[1] = index; r[2] = (uint32_t)row; r[3] = aux;
            pos++;
        }
    }
}

}  // namespace gl355

namespace {

inline uint32_t blocks(uint64_t n, uint32_t per = 256) { return (uint32_t)((n + per - 1) / per); }
struct StageTimer {
    Ctx* ctx; double* slot; std::chrono::steady_clock::time_point t0;
    StageTimer(Ctx* c, double* s) : ctx(c), slot(s), t0(std::chrono::steady_clock::now()) {}
    ~StageTimer() { if (slot) { (void)ctx->wait(); *slot += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } }
};

}  // namespace

extern "C" int32_t gl355_plonk_check_witness(gl355_ctx* h, const uint64_t* desc, uint64_t desc_words, const uint64_t* fixed_values, const uint32_t* mapping,
                                             const uint64_t* advice, const uint64_t* instances, const uint32_t* instance_lens, uint32_t* failures, uint64_t capacity,
                                             uint64_t* n_failures, double* stage_ms) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    if (!desc || !n_failures || (capacity && !failures)) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: null argument");
    *n_failures = 0;
    PlkDesc d;
    if (const char* what = plk_parse_desc(desc, desc_words, PLK_MAX_K_DEVICE, d)) return ctx->fail(GL355_E_INVALID_ARG, (std::string("plonk_check_witness: ") + what).c_str());
    const uint32_t P = d.n_gate_polys, L = d.n_lookups, M = mapping ? d.n_perm : 0;
    if (d.gate_emits != P) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: the gate program does not emit the header's number of polynomials");
    std::vector<uint32_t> lk_w(L);
    for (uint32_t l = 0; l < L; l++) {
        lk_w[l] = d.lookups[l].in_emits;
        if (!lk_w[l] || lk_w[l] != d.lookups[l].tab_emits) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: a lookup's input and table differ in width");
    }
    if ((d.n_fixed && !fixed_values) || (d.n_advice && !advice) || (d.n_instance && !instance_lens))
        return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: fixed values, advice or instance lengths missing");
    const uint64_t n = d.n, u = d.usable, W = (n + 63) / 64;
    double ms[3] = {0, 0, 0};
    auto slot = [&](int i) { return stage_ms ? &ms[i] : nullptr; };

    Staged sm(ctx);                                           // the mapping; declared before `freer`, whose wait() must come first on every return path
    std::vector<void*> mine;                                  // this call's device buffers
    struct Freer { Ctx* c; std::vector<void*>* v; ~Freer() { (void)c->wait(); for (void* p : *v) c->release(p); } } freer{ctx, &mine};
    auto D = [&](size_t bytes, auto** ptr) -> int32_t { void* p = nullptr; GL355_TRY(ctx->alloc(std::max<size_t>(bytes, 32), &p)); mine.push_back(p); *ptr = static_cast<std::remove_reference_t<decltype(*ptr)>>(p); return GL355_OK; };
    auto h2d = [&](void* dst, const void* src, size_t bytes) -> int32_t {
        if (!bytes) return GL355_OK;
        GL355_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        GL355_HIP(ctx, ctx->wait());                          // pageable source
        return GL355_OK;
    };
    // ---- the columns as canonical Montgomery values: advice | fixed | instance (padded with zeros)
    uint64_t* vals[3] = {nullptr, nullptr, nullptr};
    for (int kd = 0; kd < 3; kd++) GL355_TRY(D((size_t)std::max(1u, d.kind_cols[kd]) * n * 32, &vals[kd]));
    {
        const uint64_t* src[2] = {advice, fixed_values};
        for (int kd = 0; kd < 2; kd++) {
            if (!d.kind_cols[kd]) continue;
            Staged st(ctx);
            GL355_TRY(st.open(src[kd], (size_t)d.kind_cols[kd] * n * 32, 1));
            hipLaunchKernelGGL(chk_to_mont_kernel, dim3(blocks((uint64_t)d.kind_cols[kd] * n)), dim3(256), 0, ctx->stream, st.as<uint64_t>(), vals[kd], (uint64_t)d.kind_cols[kd] * n);
            GL355_HIP(ctx, hipGetLastError());
            GL355_HIP(ctx, ctx->wait());
        }
        GL355_HIP(ctx, hipMemsetAsync(vals[2], 0, (size_t)std::max(1u, d.n_instance) * n * 32, ctx->stream));
        uint64_t off = 0;
        for (uint32_t c = 0; c < d.n_instance; c++) {
            const uint32_t len = instance_lens[c];
            if (len > u) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: more instance values than usable rows");
            if (len && !instances) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: instance values missing");
            if (len) {
                Staged st(ctx);
                GL355_TRY(st.open(instances + 4 * off, 32ull * len, 1));
                hipLaunchKernelGGL(chk_to_mont_kernel, dim3(blocks(len)), dim3(256), 0, ctx->stream, st.as<uint64_t>(), vals[2] + 4ull * c * n, (uint64_t)len);
                GL355_HIP(ctx, hipGetLastError());
                GL355_HIP(ctx, ctx->wait());
            }
            off += len;
        }
    }
    auto col_ptr = [&](uint32_t kind, uint32_t idx) -> const uint64_t* { return vals[kind] + 4ull * idx * n; };
    // ---- programs, constants, query tables, column pointers
    uint64_t* d_consts = nullptr;
    GL355_TRY(D(std::max<size_t>(1, d.consts.size()) * 32, &d_consts));
    GL355_TRY(h2d(d_consts, d.consts.data(), d.consts.size() * 32));
    auto code_to_dev = [&](const std::vector<uint32_t>& code, uint32_t** out) -> int32_t {
        GL355_TRY(D(std::max<size_t>(16, code.size() * 4), out));
        return h2d(*out, code.data(), code.size() * 4);
    };
    int32_t* d_q[3][2];
    for (int kd = 0; kd < 3; kd++) {
        std::vector<int32_t> cols, rots;
        for (auto& q : d.queries[kd]) { cols.push_back(q.first); rots.push_back(q.second); }
        for (int w = 0; w < 2; w++) {
            GL355_TRY(D(std::max<size_t>(16, cols.size() * 4), &d_q[kd][w]));
            GL355_TRY(h2d(d_q[kd][w], (w ? rots : cols).data(), cols.size() * 4));
        }
    }
    const uint64_t** d_ptrs = nullptr;
    const uint32_t n_all = d.n_advice + d.n_fixed + d.n_instance;
    GL355_TRY(D((size_t)(n_all + d.n_perm + 1) * 8, &d_ptrs));
    {
        std::vector<const uint64_t*> v;
        for (uint32_t kd = 0; kd < 3; kd++) for (uint32_t c = 0; c < d.kind_cols[kd]; c++) v.push_back(col_ptr(kd, c));
        for (auto& pc : d.perm_cols) v.push_back(col_ptr(pc.first, pc.second));
        GL355_TRY(h2d((void*)d_ptrs, v.data(), v.size() * 8));
    }
    auto eval_args = [&](const uint32_t* code, uint32_t n_instr, uint32_t n_emit) {
        ChkEvalArgs a;
        memset(&a, 0, sizeof a);
        a.code = code; a.n_instr = n_instr; a.n_emit = n_emit; a.consts = d_consts; a.n = n; a.usable = u; a.words = W;
        a.cols[0] = d_ptrs; a.cols[1] = d_ptrs + d.n_advice; a.cols[2] = d_ptrs + d.n_advice + d.n_fixed;
        for (int kd = 0; kd < 3; kd++) { a.q_col[kd] = d_q[kd][0]; a.q_rot[kd] = d_q[kd][1]; }
        return a;
    };
    // ---- the bitmaps, in the order of the output: GATE [P] | GATE_POISONED [P] | LOOKUP [L] | PERMUTATION [M], W words each
    const uint64_t S = 2ull * P + L + M, T = S * W;
    unsigned long long *bm = nullptr, *lk_aux = nullptr;
    GL355_TRY(D(std::max<uint64_t>(1, T) * 8, &bm));
    GL355_TRY(D(std::max<uint64_t>(1, (uint64_t)L * W) * 8, &lk_aux));
    GL355_HIP(ctx, hipMemsetAsync(bm, 0, std::max<uint64_t>(1, T) * 8, ctx->stream));
    GL355_HIP(ctx, hipMemsetAsync(lk_aux, 0, std::max<uint64_t>(1, (uint64_t)L * W) * 8, ctx->stream));
    GL355_HIP(ctx, ctx->wait());

    // ---- gates
    if (P) {
        StageTimer t(ctx, slot(0));
        uint32_t* d_code = nullptr;
        GL355_TRY(code_to_dev(d.gate_code, &d_code));
        ChkEvalArgs a = eval_args(d_code, (uint32_t)(d.gate_code.size() / 4), P);
        a.fail = bm; a.poisoned = bm + (uint64_t)P * W;
        hipLaunchKernelGGL(chk_eval_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, a);
        GL355_HIP(ctx, hipGetLastError());
    }
    // ---- lookups
    if (L) {
        StageTimer t(ctx, slot(1));
        uint32_t log_slots = d.k + 1;
        uint32_t* slots = nullptr;
        GL355_TRY(D((size_t)4 << log_slots, &slots));
        uint32_t w_max = 0;
        for (uint32_t l = 0; l < L; l++) w_max = std::max(w_max, lk_w[l]);
        bool need_in = false, need_tab = false;
        for (uint32_t l = 0; l < L; l++) {
            need_in = need_in || plk_single_query(d.queries, d.lookups[l].in_code).first >= 3;
            need_tab = need_tab || plk_single_query(d.queries, d.lookups[l].tab_code).first >= 3;
        }
        uint64_t *in_buf = nullptr, *tab_buf = nullptr;
        unsigned long long *in_poi = nullptr, *tab_poi = nullptr;
        if (need_in) { GL355_TRY(D((size_t)w_max * n * 32, &in_buf)); GL355_TRY(D(W * 8, &in_poi)); }
        if (need_tab) { GL355_TRY(D((size_t)w_max * n * 32, &tab_buf)); GL355_TRY(D(W * 8, &tab_poi)); }
        const uint64_t* table_built = nullptr;                // the single column the hash set currently holds (the reference's nine lookups share one)
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t w = lk_w[l];
            ChkTuples tin, ttab;
            const auto qa = plk_single_query(d.queries, d.lookups[l].in_code), qs = plk_single_query(d.queries, d.lookups[l].tab_code);
            auto run = [&](const std::vector<uint32_t>& code, uint64_t* out, unsigned long long* poi) -> int32_t {
                uint32_t* d_code = nullptr;
                GL355_TRY(code_to_dev(code, &d_code));
                ChkEvalArgs a = eval_args(d_code, (uint32_t)(code.size() / 4), w);
                a.out = out; a.poisoned = poi;
                hipLaunchKernelGGL(chk_eval_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, a);
                GL355_HIP(ctx, hipGetLastError());
                return GL355_OK;
            };
            if (qa.first < 3) tin = {col_ptr(qa.first, qa.second), nullptr};
            else { GL355_TRY(run(d.lookups[l].in_code, in_buf, in_poi)); tin = {in_buf, in_poi}; }
            bool build = true;
            if (qs.first < 3) { ttab = {col_ptr(qs.first, qs.second), nullptr}; build = table_built != ttab.base; table_built = ttab.base; }
            else { GL355_TRY(run(d.lookups[l].tab_code, tab_buf, tab_poi)); ttab = {tab_buf, tab_poi}; table_built = nullptr; }
            if (build) {
                GL355_HIP(ctx, hipMemsetAsync(slots, 0xFF, (size_t)4 << log_slots, ctx->stream));
                hipLaunchKernelGGL(chk_table_insert_kernel, dim3(blocks(u)), dim3(256), 0, ctx->stream, ttab, w, n, u, slots, log_slots);
            }
            hipLaunchKernelGGL(chk_lookup_probe_kernel, dim3(blocks(n)), dim3(256), 0, ctx->stream, tin, ttab, w, n, u, (const uint32_t*)slots, log_slots, W,
                               bm + (2ull * P + l) * W, lk_aux + (uint64_t)l * W);
            GL355_HIP(ctx, hipGetLastError());
        }
    }
    // ---- copy constraints
    uint32_t* d_flag = nullptr;
    GL355_TRY(D(32, &d_flag));
    GL355_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    if (M) {
        GL355_TRY(sm.open(mapping, (size_t)M * n * 8, 1));
        GL355_HIP(ctx, ctx->wait());                          // the upload is not part of the stage
        StageTimer t(ctx, slot(2));
        hipLaunchKernelGGL(chk_copy_kernel, dim3(blocks(n), M), dim3(256), 0, ctx->stream, sm.as<uint32_t>(), (const uint64_t* const*)(d_ptrs + n_all), n, M, W,
                           bm + (2ull * P + L) * W, d_flag);
        GL355_HIP(ctx, hipGetLastError());
    }
    // ---- count, then the first `capacity` records in (kind, index, row) order
    unsigned long long total = 0;
    uint32_t flag = 0;
    const uint64_t n_blocks = (T + CHK_WORDS_PER_BLOCK - 1) / CHK_WORDS_PER_BLOCK;
    uint32_t* d_sums = nullptr;
    unsigned long long* d_offsets = nullptr;                  // [n_blocks] + the total
    GL355_TRY(D(std::max<uint64_t>(1, n_blocks) * 4, &d_sums));
    GL355_TRY(D((n_blocks + 1) * 8, &d_offsets));
    if (n_blocks) hipLaunchKernelGGL(chk_count_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, ctx->stream, (const unsigned long long*)bm, T, d_sums);
    hipLaunchKernelGGL(chk_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t*)d_sums, n_blocks, d_offsets, d_offsets + n_blocks);
    GL355_HIP(ctx, hipGetLastError());
    GL355_HIP(ctx, ctx->d2h(&total, d_offsets + n_blocks, 8));
    GL355_HIP(ctx, ctx->d2h(&flag, d_flag, 4));
    GL355_HIP(ctx, ctx->wait());
    if (flag) return ctx->fail(GL355_E_INVALID_ARG, "plonk_check_witness: permutation mapping out of range");
    const uint64_t n_rec = std::min<uint64_t>(capacity, total);
    if (n_rec) {
        const bool dev_out = ptr_is_device(failures);
        uint32_t* d_rec = failures;
        if (!dev_out) GL355_TRY(D(n_rec * 16, &d_rec));
        ChkExtractArgs a;
        memset(&a, 0, sizeof a);
        a.bm = bm; a.lookup_aux = lk_aux; a.offsets = d_offsets; a.total_words = T; a.words = W; a.n = n; a.capacity = n_rec; a.n_polys = P; a.n_lookups = L;
        a.mapping = M ? sm.as<uint32_t>() : nullptr; a.records = d_rec;
        hipLaunchKernelGGL(chk_extract_kernel, dim3((uint32_t)n_blocks), dim3(256), 0, ctx->stream, a);
        GL355_HIP(ctx, hipGetLastError());
        if (!dev_out) GL355_HIP(ctx, ctx->d2h(failures, d_rec, n_rec * 16));
        GL355_HIP(ctx, ctx->wait());
    }
    *n_failures = total;
    if (stage_ms) for (int i = 0; i < 3; i++) stage_ms[i] = ms[i];
    return GL355_OK;
}
