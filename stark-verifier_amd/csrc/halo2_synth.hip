// Witness synthesis of a recorded Halo2 circuit ON THE DEVICE (part 1 of the verifier circuit): the tape of halo2_tape.h --
// what `Verifier::synthesize` assigns through ArithmeticChip / AllChip::permute (verifier_circuit.rs, chip/native_chip/arithmetic_chip.rs:204-500,
// all_chip.rs:52-89) -- interpreted by the GPU, so the [19][2^k][4] advice columns appear where gl355_plonk_prove and gl355_plonk_check_witness read
// them: the host uploads the proof's words instead of 19 x 2^k x 32 bytes of columns.
//
// Schedule: one launch per LEVEL of the tape's DAG, all on the context's stream (no host round trip between levels: the host only enqueues),
// one lane per entry.  The entries of a level are independent and write disjoint cells (validated at load), and a level reads only what earlier
// launches wrote, so stream order is the only synchronisation.  A PERMUTE entry is one lane's whole permutation: the 68 rounds in their dense
// form (the circuit's gates constrain every round's state, so the sparse partial rounds of bn254_permute_fr cannot be used) over bn254.cuh's
// Fr arithmetic, each round's state leaving the Montgomery form once to be stored.  What bounds it is the depth of the DAG times the latency of
// one permutation: a Merkle path is a chain of permutations, however many paths run side by side.
//
// A level with few PERMUTE entries (the transcript: a chain of single permutations everything else waits for; the small Merkle levels) runs
// the SPREAD form of the kernel instead: eight lanes per entry, and a permutation over five of them, one state element per lane.  In a full
// round every lane adds its constant and takes x^5, in a partial round only lane 0 does; for the MDS row lane i forms sum_j M[i][j] s_j from the
// other lanes' limbs, read by cross-lane moves (__shfl: ds_bpermute, no LDS planes), and stores its own state column.  The operations on every
// element are h2_round's, in the same order, so the limbs and the stored columns are the same.  Per round a lane's chain is 3 + 5 + 1 products
// instead of 15 + 25 + 5 (full) or 3 + 25 + 5 (partial).  The rule for choosing the form is halo2_spread_level below.
//
// A RUN of consecutive narrow levels without a PERMUTE (the public-inputs hasher's serial Goldilocks permutations, the gate constrainers' and
// the reduce_extension chains: part 3's many-input circuit has 61 501 levels, 61 283 of them such) is one launch of ONE workgroup that replays
// it level by level behind workgroup barriers: halo2_run_kernel below, where the rule and the guarantees it rests on are.
//
// Offsets are validated once when the tape is loaded (halo2_tape_validate), so the interpreter does not bounds-check; data-dependent
// failures (a VALUE not below p, an ASSERT_EQ on differing cells = an invalid proof) are reported as the smallest failing entry and the number of
// failing entries, exactly like the host replay, and the rows are written all the same.
#include "gl355_internal.h"
#include "halo2_tape.h"
#include "bn254.cuh"

namespace gl355 {

// one dense round (native.rs:45-62): constants, x^5 on every element (full) or on the first, the 5x5 MDS
GL_DEV void h2_round(fr8 (&s)[5], int rnd) {
    const bool full = rnd < 4 || rnd >= 64;
    s[0] = fr_pow5(fr_add(s[0], fr_const(BN254F_RC[5 * rnd])));
    if (full) {
        for (int i = 1; i < 5; i++) s[i] = fr_pow5(fr_add(s[i], fr_const(BN254F_RC[5 * rnd + i])));
    } else {
#pragma unroll
        for (int i = 1; i < 5; i++) s[i] = fr_add(s[i], fr_const(BN254F_RC[5 * rnd + i]));
    }
    fr8 n[5];
    for (int i = 0; i < 5; i++) {
        fr8 acc = fr_mul(s[0], fr_const(BN254F_MDS[5 * i]));
#pragma unroll
        for (int j = 1; j < 5; j++) acc = fr_add(acc, fr_mul(s[j], fr_const(BN254F_MDS[5 * i + j])));
        n[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) s[i] = n[i];
}

GL_DEV void h2_permute_rows(const H2Cols& c, const uint64_t* e) {
    const uint64_t row = e[1];
    fr8 s[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const h2_w4 v = h2_operand(c, e[2 + i]);
        h2_store(c, H2_COL_STATE + i, row, v);
        s[i] = fr_enter(v.w);
    }
#pragma unroll 1
    for (int rnd = 0; rnd < 68; rnd++) {
        h2_round(s, rnd);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            h2_w4 v;
            fr_leave(s[i], v.w);
            h2_store(c, H2_COL_STATE + i, row + rnd + 1, v);
        }
    }
}

// element j of the group's state: every limb from lane j of this lane's group of eight
GL_DEV fr8 h2_from_lane(const fr8& x, int j) {
    fr8 r;
#pragma unroll
    for (int l = 0; l < FR_W; l++) r.l[l] = (uint32_t)__shfl((int)x.l[l], j, H2_SPREAD_LANES);
    return r;
}

// h2_permute_rows over the lanes of a group: lane i < 5 holds state element i (lanes 5 .. 7 shadow element 4 and store nothing).  All eight
// lanes of a group take every branch together except the x^5 of a partial round, which has no cross-lane move inside it
GL_DEV void h2_permute_rows_spread(const H2Cols& c, const uint64_t* e, int lane) {
    const uint64_t row = e[1];
    const int i = lane < 5 ? lane : 4;
    const bool stores = lane < 5;
    h2_w4 v = h2_operand(c, e[2 + i]);
    if (stores) h2_store(c, H2_COL_STATE + i, row, v);
    fr8 s = fr_enter(v.w);
    fr8 m[5];                                          // row i of the MDS matrix
#pragma unroll
    for (int j = 0; j < 5; j++) m[j] = fr_const(BN254F_MDS[5 * i + j]);
    fr8 rc = fr_const(BN254F_RC[i]);
#pragma unroll 1
    for (int rnd = 0; rnd < 68; rnd++) {
        const bool full = rnd < 4 || rnd >= 64;
        fr8 t = fr_add(s, rc);
        rc = fr_const(BN254F_RC[5 * (rnd < 67 ? rnd + 1 : rnd) + i]);      // the next round's constant, loaded under this round's products
        if (full || lane == 0) t = fr_pow5(t);
        fr8 acc = fr_mul(h2_from_lane(t, 0), m[0]);
#pragma unroll
        for (int j = 1; j < 5; j++) acc = fr_add(acc, fr_mul(h2_from_lane(t, j), m[j]));
        s = acc;
        fr_leave(s, v.w);
        if (stores) h2_store(c, H2_COL_STATE + i, row + rnd + 1, v);
    }
}

// SPREAD: eight lanes per entry (a PERMUTE entry over five of them, any other entry on the first); otherwise one lane per entry
template <bool SPREAD>
__global__ void __launch_bounds__(64) halo2_level_kernel(const uint64_t* tape, uint64_t first, uint64_t count, H2Cols c, unsigned long long* status) {
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t i = SPREAD ? t / H2_SPREAD_LANES : t;
    const int lane = SPREAD ? (int)(threadIdx.x % H2_SPREAD_LANES) : 0;
    if (i >= count) return;
    const uint64_t* e = tape + H2_ENTRY_WORDS * (first + i);
    int fail = 0;
    if (((uint32_t)e[0] & 0xFF) == H2_OP_PERMUTE) {
        if (SPREAD) h2_permute_rows_spread(c, e, lane);
        else h2_permute_rows(c, e);
    } else if (lane == 0) fail = h2_exec(c, e);
    if (fail) {
        atomicMin(status, (unsigned long long)(first + i));
        atomicAdd(status + 1, 1ull);
    }
}

// A RUN: consecutive levels, none with a PERMUTE entry and none wider than run_max, replayed by ONE workgroup in one launch instead of one
// launch each.  The tape is level-major, so the run is the entry range level_start[first_level] .. level_start[first_level + n_levels); a
// thread takes the entries of a level H2_RUN_THREADS apart and calls the same h2_exec, so the columns and the status words are the level
// kernel's.  Between two levels stands __syncthreads(): a workgroup-scope release fence, the barrier, a workgroup-scope acquire fence.  What
// makes a level's stores visible to the next level's loads is that fence pair in the AMDGPU memory model, which for gfx950 outside
// threadgroup-split mode rests on this: the waves of a workgroup are on ONE CU and send their vector memory operations through that CU's one L1
// in order, so a load issued after the barrier is served behind every store that a wave of the workgroup issued before it.  No wave has to
// wait for its stores to complete before it arrives, and the compiled kernel does not (no vmcnt wait stands before its barrier).  The
// project does not build with tgsplit.  Nothing here relies on visibility ACROSS workgroups (one workgroup per
// launch, and launches are ordered by the stream).  Hang safety: the level loop's bound is a kernel argument, the entry loop holds no
// barrier, and no thread returns before the last barrier -- a thread without an entry in a level still arrives, a failing entry goes on.
__global__ void __launch_bounds__(H2_RUN_THREADS) halo2_run_kernel(const uint64_t* tape, const uint64_t* level_start, uint32_t first_level, uint32_t n_levels,
                                                                   H2Cols c, unsigned long long* status) {
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint64_t first = level_start[first_level + l], end = level_start[first_level + l + 1];
        for (uint64_t i = first + threadIdx.x; i < end; i += H2_RUN_THREADS)
            if (h2_exec(c, tape + H2_ENTRY_WORDS * i)) {
                atomicMin(status, (unsigned long long)i);
                atomicAdd(status + 1, 1ull);
            }
        __syncthreads();
    }
}

// GL355_HALO2_RUN_MAX (entries of a level) overrides the bound of a run's levels: 0 turns the form off (profiles/halo2_synth_verifier.txt
// has the figures with and without)
uint64_t halo2_run_max() {
    const char* v = getenv("GL355_HALO2_RUN_MAX");
    return v && *v ? strtoull(v, nullptr, 10) : H2_RUN_MAX_DEFAULT;
}

// The launches of one synthesis: a level joins a run when it has no PERMUTE entry and at most run_max entries; a maximal run of at least two
// such levels is one launch of halo2_run_kernel, every other level that holds an entry is one launch of halo2_level_kernel.  Planned once,
// at load: gl355_halo2_synthesize walks this list and gl355_halo2_tape_launches counts it, so what is reported is what is launched.
void halo2_plan_launches(gl355_halo2_tape* t) {
    const size_t n_levels = t->level_start.size() - 1;
    const auto in_run = [&](size_t l) { return l < n_levels && !t->level_permutes[l] && t->level_start[l + 1] - t->level_start[l] <= t->run_max; };
    t->launches.clear();
    for (size_t l = 0; l < n_levels; l++) {
        if (t->level_start[l + 1] == t->level_start[l]) continue;
        size_t end = l + 1;
        if (t->run_max && in_run(l))
            while (in_run(end)) end++;
        t->launches.emplace_back((uint32_t)l, (uint32_t)(end - l));
        l = end - 1;
    }
}

// The form of a level.  SPREAD gives an entry eight lanes, so it is taken while the level still leaves lanes idle that way -- at most one wave
// per SIMD (4 SIMDs a CU) -- and has a PERMUTE entry to gain from it; beyond that the lanes are worth more as entries.  GL355_HALO2_SPREAD_MAX
// (entries of a level) overrides the bound: 0 turns the form off (profiles/halo2_synth_fri.txt has the figures with and without)
uint64_t halo2_spread_max(int compute_units) {
    const char* v = getenv("GL355_HALO2_SPREAD_MAX");
    return v && *v ? strtoull(v, nullptr, 10) : (uint64_t)compute_units * 4 * (64 / H2_SPREAD_LANES);
}

}  // namespace gl355

using namespace gl355;

extern "C" int32_t gl355_halo2_tape_load(gl355_ctx* h, const uint64_t* tape, uint64_t n_words, uint64_t n_inputs, uint32_t k, uint32_t n_advice,
                                         gl355_halo2_tape** out) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!out) return ctx->fail(GL355_E_INVALID_ARG, "halo2_tape_load: null argument");
    *out = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    std::vector<uint64_t> level_start;
    gl355_halo2_tape* t = nullptr;
    try {
        if (const char* what = halo2_tape_validate(tape, n_words, n_inputs, k, n_advice, &level_start))
            return ctx->fail(GL355_E_INVALID_ARG, (std::string("halo2_tape_load: ") + what).c_str());
        t = new gl355_halo2_tape();
        t->host.assign(tape, tape + n_words);
    } catch (const std::bad_alloc&) {      // the validator's table of writers (40 bytes a row) or the host copy of the tape
        delete t;
        return ctx->fail(GL355_E_OOM, "halo2_tape_load: out of host memory");
    }
    t->ctx = ctx; t->k = k; t->n_advice = n_advice; t->n_entries = n_words / H2_ENTRY_WORDS; t->n_inputs = n_inputs;
    t->level_start.swap(level_start);
    t->level_permutes.assign(t->level_start.size() - 1, 0);
    for (size_t l = 0; l + 1 < t->level_start.size(); l++)
        for (uint64_t i = t->level_start[l]; i < t->level_start[l + 1]; i++) t->level_permutes[l] += ((uint32_t)tape[H2_ENTRY_WORDS * i] & 0xFF) == H2_OP_PERMUTE;
    t->dev = nullptr;
    t->dev_level_start = nullptr;
    t->run_max = halo2_run_max();
    try {
        halo2_plan_launches(t);
    } catch (const std::bad_alloc&) {
        delete t;
        return ctx->fail(GL355_E_OOM, "halo2_tape_load: out of host memory");
    }
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) { delete t; return ctx->fail(GL355_E_HIP, "halo2_tape_load: hipDeviceGetAttribute failed"); }
    t->spread_max = halo2_spread_max(n_cu);
    if (hipMalloc(reinterpret_cast<void**>(&t->dev), std::max<size_t>(n_words * 8, 64)) != hipSuccess) { delete t; return ctx->fail(GL355_E_OOM, "halo2_tape_load: hipMalloc failed"); }
    if (n_words && hipMemcpy(t->dev, tape, n_words * 8, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(t->dev);
        delete t;
        return ctx->fail(GL355_E_HIP, "halo2_tape_load: upload failed");
    }
    const size_t ls_bytes = t->level_start.size() * 8;
    if (hipMalloc(reinterpret_cast<void**>(&t->dev_level_start), ls_bytes) != hipSuccess ||
        hipMemcpy(t->dev_level_start, t->level_start.data(), ls_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(t->dev_level_start);
        (void)hipFree(t->dev);
        delete t;
        return ctx->fail(GL355_E_HIP, "halo2_tape_load: upload of the level table failed");
    }
    *out = t;
    return GL355_OK;
}

extern "C" int32_t gl355_halo2_tape_free(gl355_halo2_tape* t) {
    if (!t) return GL355_OK;
    if (t->dev) {
        (void)hipSetDevice(t->ctx->device);
        (void)t->ctx->wait();
        (void)hipFree(t->dev);
        (void)hipFree(t->dev_level_start);
    }
    delete t;
    return GL355_OK;
}

extern "C" int32_t gl355_halo2_tape_launches(const gl355_halo2_tape* t, uint64_t* out) {
    if (!t || !out) return GL355_E_INVALID_ARG;
    out[0] = t->run_max;
    out[1] = out[2] = 0;
    out[3] = t->launches.size();
    for (const auto& launch : t->launches)
        if (launch.second > 1) { out[1] += launch.second; out[2]++; }
    return GL355_OK;
}

extern "C" int32_t gl355_halo2_synthesize(gl355_ctx* h, const gl355_halo2_tape* t, const uint64_t* inputs, uint64_t* advice_out, uint64_t* status) {
    Ctx* ctx = ctx_of(h);
    if (!ctx) return GL355_E_INVALID_ARG;
    if (!t || t->ctx != ctx || !advice_out || !status || (t->n_inputs && !inputs)) return ctx->fail(GL355_E_INVALID_ARG, "halo2_synthesize: null argument or a tape of another context");
    if (hipSetDevice(ctx->device) != hipSuccess) return ctx->fail(GL355_E_HIP, "hipSetDevice failed");
    const uint64_t n = 1ull << t->k;
    const size_t bytes = (size_t)t->n_advice * n * 32;
    Staged in(ctx), adv(ctx);
    GL355_TRY(in.open(inputs, std::max<size_t>(t->n_inputs * 8, 8), 1));
    GL355_TRY(adv.open(advice_out, bytes, 2));
    Scratch st(ctx);
    GL355_TRY(st.get(64));
    unsigned long long* d_status = st.as<unsigned long long>();
    GL355_HIP(ctx, hipMemsetAsync(adv.dev, 0, bytes, ctx->stream));
    GL355_HIP(ctx, hipMemsetAsync(d_status, 0xFF, 8, ctx->stream));
    GL355_HIP(ctx, hipMemsetAsync(d_status + 1, 0, 8, ctx->stream));
    const H2Cols c = {adv.as<uint64_t>(), n, in.as<uint64_t>()};
    {
        ProfScope ps(ctx, "halo2_synthesize", bytes);
        for (const auto& launch : t->launches) {
            const uint32_t l = launch.first;
            const uint64_t first = t->level_start[l], count = t->level_start[l + 1] - first;
            if (launch.second > 1)                                // a run: one launch, one workgroup
                hipLaunchKernelGGL(halo2_run_kernel, dim3(1), dim3(H2_RUN_THREADS), 0, ctx->stream, t->dev, t->dev_level_start, l, launch.second, c, d_status);
            else if (t->level_permutes[l] && count <= t->spread_max)
                hipLaunchKernelGGL(halo2_level_kernel<true>, dim3((uint32_t)((count * H2_SPREAD_LANES + 63) / 64)), dim3(64), 0, ctx->stream, t->dev, first, count, c, d_status);
            else
                hipLaunchKernelGGL(halo2_level_kernel<false>, dim3((uint32_t)((count + 63) / 64)), dim3(64), 0, ctx->stream, t->dev, first, count, c, d_status);
            GL355_HIP(ctx, hipGetLastError());
        }
    }
    GL355_HIP(ctx, ctx->d2h(status, d_status, 16));
    GL355_HIP(ctx, ctx->wait());
    GL355_TRY(adv.finish());
    return GL355_OK;
}
