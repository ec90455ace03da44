// Experiment kernels of the 24-bit-limb LDE passes: the forms that were measured against the shipped kernels of csrc/ntt_l24.cuh and lost, or
// that the shipped ones grew out of.  Moved here verbatim from csrc/ntt_l24.cuh; the library launches none of them.  Included by
// tools/ubench/ubench_ntt_l24.hip and ubench_ntt_l24d.hip only.  The limb primitives (L24, dif8_l24, l24_twiddles_r, l24_value, the row buffer
// helpers) and ntt_rows_l24s_kernel / ntt_cols_l24s_cosets_kernel, which these are compared with, come from the product header.
#pragma once
#include "ntt_l24.cuh"

// 1: a persistent row block keeps its eight mid twiddles in registers for all its rows (128 VGPRs + scratch); 0: re-read per row
#ifndef GL355_L24_TW_REGS
#define GL355_L24_TW_REGS 0
#endif

namespace gl355 {

// a * w for w tabulated as four words W_i = w X^i mod p at w[0..3]: the general twiddle WITHOUT leaving the limb form first (header comment of
// csrc/ntt_l24.cuh).  Result: profiles/r03_ubench_ntt_l24.txt (32 bytes of table per element: bound by the CU's vector-memory path).
GL_DEV uint64_t l24_mul4(const L24& a, const uint64_t* __restrict__ w) {
    const ulonglong2 p0 = *reinterpret_cast<const ulonglong2*>(w), p1 = *reinterpret_cast<const ulonglong2*>(w + 2);
    return l24_mul4(a, p0.x, p0.y, p1.x, p1.y);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Row pass: 4096-point rows, 512-thread blocks = two radix-64 super-rounds on a 64 x 64 view (index = 64 u + v): A over u (stride 64),
// the general twiddle omega_4096^(v kA) (a.mid: one word per cell), B over v.  Wave w is butterfly r = w of every first round, so the
// shift twiddles are compile-time per branch.  The tile lives in LDS as 16-byte limb quads at index + (index >> 6) (row stride 65
// quads: the B rounds walk a lane stride of 65 x 16 bytes, conflict-free per 16-lane group); the two exchanges that carry reduced
// 8-byte values (between the super-rounds, and the transposition to store order) use the low half of a thread's OWN cells, so no
// barrier is needed before writing them.  Blocks are PERSISTENT (grid = 2 per CU): a block's eight mid twiddles per thread stay in
// registers for all its rows -- fetched per row they were 128 KB of L2 reads per 64 KB of data and, through the CU's 64-B/clk vector
// memory path, a fifth of the pass (profiles/r03_ubench_ntt_l24.txt) -- and the next row's elements are fetched while this one is
// transformed.  Output order: plain bit reversal (identical to ntt_rows_r8_kernel<12>), canonical.
// Result: profiles/r03_ubench_ntt_l24.txt, r03_ubench_ntt_l24s.txt (against the split-exchange kernel that replaced it).
// ------------------------------------------------------------------------------------------------------------------------------
GL_DEV uint32_t l24_phys(uint32_t idx) { return idx + (idx >> 6); }
constexpr size_t L24_ROWS_LDS_BYTES = (4096 + 64) * 16;

template <int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE))) ntt_rows_l24_kernel(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_raw[];
    int4* lq = reinterpret_cast<int4*>(lds_raw);
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint64_t total_rows = ((uint64_t)a.batch) << a.log_rows;
    // cell addresses written out as base + compile-time offset (the padding idx + (idx >> 6) is linear inside each access pattern), so the
    // compiler issues ds instructions with immediate offsets from five base registers instead of keeping ~40 precomputed addresses alive
    auto put = [&](uint32_t cell, const L24& v) { lq[cell] = make_int4(v.l[0], v.l[1], v.l[2], v.l[3]); };
    auto get = [&](uint32_t cell) { const int4 q = lq[cell]; L24 v; v.l[0] = q.x; v.l[1] = q.y; v.l[2] = q.z; v.l[3] = q.w; return v; };
    auto put8 = [&](uint32_t cell, uint64_t v) { lds_raw[2 * cell] = v; };      // the low 8 bytes of a quad cell
    auto get8 = [&](uint32_t cell) { return lds_raw[2 * cell]; };
    const uint32_t cA1 = 65 * w + lane;          // idx = 64 (8 q + w) + lane      -> cell cA1 + 520 q
    const uint32_t cA2 = 520 * w + lane;         // idx = 64 (8 w + r) + lane      -> cell cA2 + 65 r
    const uint32_t cB1 = 65 * lane + w;          // idx = 64 lane + 8 q + w        -> cell cB1 + 8 q
    const uint32_t cB2 = 65 * lane + 8 * w;      // idx = 64 lane + 8 w + r        -> cell cB2 + r
    const uint32_t cST = tid + w;                // idx = tid + 512 q              -> cell cST + 520 q
    auto row_ptr = [&](uint64_t row, const uint64_t* base, uint64_t stride) {
        const uint64_t col = row >> a.log_rows, rin = row & ((1ull << a.log_rows) - 1);
        return base + col * stride + (rin << 12);
    };
#if GL355_L24_TW_REGS
    uint64_t tw[8];                                         // cell (8 w + s, lane) of the mid table, s < 8: the same for every row
#pragma unroll
    for (int s = 0; s < 8; s++) tw[s] = a.mid[64 * (8 * w + s) + lane];
#endif
    uint64_t row = blockIdx.x;
    const uint32_t tid8 = tid * 8;
    uint64_t x[8];
    if (row < total_rows) {
        const __amdgpu_buffer_rsrc_t rin = l24_row_rsrc(row_ptr(row, a.in, a.in_col_stride));
#pragma unroll
        for (int q = 0; q < 8; q++) x[q] = l24_row_load(rin, tid8, q);
    }
    while (row < total_rows) {
        L24 y[8];
        // A1: the thread that loaded elements tid + 512 q holds u = 8 q + w, v = lane: its own first-round butterfly (r = w)
#pragma unroll
        for (int q = 0; q < 8; q++) y[q] = l24_split(x[q]);
        const uint64_t next = row + gridDim.x;
        if (next < total_rows) {
            const __amdgpu_buffer_rsrc_t rin = l24_row_rsrc(row_ptr(next, a.in, a.in_col_stride));
#pragma unroll
            for (int q = 0; q < 8; q++) x[q] = l24_row_load(rin, tid8, q);
        }
        dif8_l24<false>(y);
        l24_twiddles_r<6, false>(y, w);
#pragma unroll
        for (int q = 0; q < 8; q++) put(cA1 + 520 * q, y[q]);
#if !GL355_L24_TW_REGS
        uint64_t tw[8];                                     // fetched per row (32 KB per tile, L2-resident), issued before the barrier: held
#pragma unroll                                              // across rows they cost 16 VGPRs and pushed the kernel into scratch
        for (int s = 0; s < 8; s++) tw[s] = a.mid[64 * (8 * w + s) + lane];
#endif
        __syncthreads();
        // A2: u = 8 w + r over r, then the general twiddle of the 64 x 64 split; 8-byte products into the thread's own cells
#pragma unroll
        for (int r = 0; r < 8; r++) y[r] = get(cA2 + 65 * r);
        dif8_l24<false>(y);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            put8(cA2 + 65 * s, gl_mul(l24_value(y[s]), tw[s]));
            if (s & 1) __builtin_amdgcn_sched_barrier(0);   // two elements in flight, not eight: their temporaries would not fit 128 VGPRs
        }
        __syncthreads();
        // B1: u-slot = lane, v = 8 q + w; reads and writes the same eight cells
#pragma unroll
        for (int q = 0; q < 8; q++) y[q] = l24_split(get8(cB1 + 8 * q));
        dif8_l24<false>(y);
        l24_twiddles_r<6, false>(y, w);
#pragma unroll
        for (int q = 0; q < 8; q++) put(cB1 + 8 * q, y[q]);
        __syncthreads();
        // B2: v = 8 w + r over r; results leave the limb form (own cells again), then the transposition to store order
#pragma unroll
        for (int r = 0; r < 8; r++) y[r] = get(cB2 + r);
        dif8_l24<false>(y);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            put8(cB2 + s, gl_canon(l24_value(y[s])));
            if (s & 1) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        const __amdgpu_buffer_rsrc_t rout = l24_row_rsrc(row_ptr(row, a.out, a.out_col_stride));
#pragma unroll
        for (int q = 0; q < 8; q++) l24_row_store(rout, tid8, q, get8(cST + 520 * q));
        __syncthreads();                                    // the tile is free for the next row's quads
        row = next;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Round 6 experiment: the limb-QUAD row pass (16-byte cells, 65-KB tile, 5 barriers per row) as ONE ROW PER BLOCK -- the quad kernel above is
// persistent with a register-staged prefetch (128 VGPRs); this is its arithmetic and exchange pattern with the launch shape of the shipped
// split-exchange kernel (fresh blocks, no prefetch): two blocks per CU either way (LDS here, registers there), 3 barriers fewer per row.
// Result: profiles/r06_ubench_ntt_l24d.txt.
// ------------------------------------------------------------------------------------------------------------------------------
template <int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE))) ntt_rows_l24q_kernel(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_raw[];
    int4* lq = reinterpret_cast<int4*>(lds_raw);
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    auto put = [&](uint32_t cell, const L24& v) { lq[cell] = make_int4(v.l[0], v.l[1], v.l[2], v.l[3]); };
    auto get = [&](uint32_t cell) { const int4 q = lq[cell]; L24 v; v.l[0] = q.x; v.l[1] = q.y; v.l[2] = q.z; v.l[3] = q.w; return v; };
    auto put8 = [&](uint32_t cell, uint64_t v) { lds_raw[2 * cell] = v; };
    auto get8 = [&](uint32_t cell) { return lds_raw[2 * cell]; };
    const uint32_t cA1 = 65 * w + lane, cA2 = 520 * w + lane, cB1 = 65 * lane + w, cB2 = 65 * lane + 8 * w, cST = tid + w;
    const uint64_t row = blockIdx.x;
    const uint64_t col = row >> a.log_rows, rin = row & ((1ull << a.log_rows) - 1);
    const uint32_t tid8 = tid * 8;
    const __amdgpu_buffer_rsrc_t rs_in = l24_row_rsrc(a.in + col * a.in_col_stride + (rin << 12));
    L24 y[8];
#pragma unroll
    for (int q = 0; q < 8; q++) y[q] = l24_split(l24_row_load(rs_in, tid8, q));
    dif8_l24<false>(y);
    l24_twiddles_r<6, false>(y, w);
#pragma unroll
    for (int q = 0; q < 8; q++) put(cA1 + 520 * q, y[q]);
    uint64_t tw[8];
#pragma unroll
    for (int s = 0; s < 8; s++) tw[s] = a.mid[64 * (8 * w + s) + lane];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) y[r] = get(cA2 + 65 * r);
    dif8_l24<false>(y);
#pragma unroll
    for (int s = 0; s < 8; s++) {
        put8(cA2 + 65 * s, gl_mul(l24_value(y[s]), tw[s]));
        if (s & 1) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; q++) y[q] = l24_split(get8(cB1 + 8 * q));
    dif8_l24<false>(y);
    l24_twiddles_r<6, false>(y, w);
#pragma unroll
    for (int q = 0; q < 8; q++) put(cB1 + 8 * q, y[q]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) y[r] = get(cB2 + r);
    dif8_l24<false>(y);
#pragma unroll
    for (int s = 0; s < 8; s++) {
        put8(cB2 + s, gl_canon(l24_value(y[s])));
        if (s & 1) __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_out = l24_row_rsrc(a.out + col * a.out_col_stride + (rin << 12));
#pragma unroll
    for (int q = 0; q < 8; q++) l24_row_store(rs_out, tid8, q, get8(cST + 520 * q));
}

// ------------------------------------------------------------------------------------------------------------------------------
// Round 6 experiment: the split-exchange row pass with the NEXT row fetched by LDS-DMA (global_load_lds_dwordx4: global -> LDS without passing
// through registers) while this row is transformed.  The register-staged prefetch of round 3 / 5 cost 16 VGPRs and with them the kernel's occupancy
// (profiles/r05_ubench_ntt_l24s.txt: 0.66-0.70 ms against 0.56); a DMA costs none, only 32 KB of LDS for the raw row next to the 33-KB tile
// (2 blocks per CU either way).  Persistent blocks walk rows blockIdx, blockIdx + grid, ...  Every barrier is a raw s_barrier behind lgkmcnt(0):
// __syncthreads() would drain the DMA in flight (its fence waits vmcnt(0)).  One vector-memory counter orders everything: at the top of an
// iteration the row's four DMA pieces per wave are older than the previous row's eight stores, so vmcnt(8) retires exactly them; the barrier that
// follows makes the other waves' pieces visible.  The DMA of row r + 1 is issued behind the first barrier of row r, when every thread has read
// its elements of row r out of the raw buffer.  Same cells, same arithmetic, same output as ntt_rows_l24s_kernel.
// Result: profiles/r06_ubench_ntt_l24d.txt (the register-staged prefetch it replaces: r05_ubench_ntt_l24s.txt).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr size_t L24D_ROWS_LDS_BYTES = 0;      // static LDS: (4096 + 64) * 8 + 4096 * 8 = 66 048 B
#define GL355_L24D_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
template <int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE))) ntt_rows_l24d_kernel(PassArgs a) {
    // two DISTINCT LDS objects: the compiler orders a ds access behind an LDS-DMA in flight unless it can prove they do not alias, and inside one
    // dynamic array it cannot (it then waits vmcnt(0) in front of every tile access, i.e. right behind the DMA's issue)
    __shared__ __attribute__((aligned(16))) uint64_t lds_raw[4096 + 64];
    __shared__ __attribute__((aligned(16))) uint64_t raw[4096];
    int2* lp = reinterpret_cast<int2*>(lds_raw);
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint64_t total_rows = ((uint64_t)a.batch) << a.log_rows;
    const uint32_t cA1 = 65 * w + lane, cA2 = 520 * w + lane, cB1 = 65 * lane + w, cB2 = 65 * lane + 8 * w, cST = tid + w;
    auto row_ptr = [&](uint64_t row, const uint64_t* base, uint64_t stride) {
        const uint64_t col = row >> a.log_rows, rin = row & ((1ull << a.log_rows) - 1);
        return base + col * stride + (rin << 12);
    };
    typedef __attribute__((address_space(3))) void* lds_vptr;
    typedef const __attribute__((address_space(1))) void* glb_vptr;
    // wave w fetches elements [512 w, 512 w + 512) of the row as four 1-KB pieces: lane l of piece j brings elements 512 w + 128 j + 2 l, + 1
    auto dma_row = [&](const uint64_t* rowp) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t e0 = 512 * w + 128 * j;
            __builtin_amdgcn_global_load_lds((glb_vptr)(rowp + e0 + 2 * lane), (lds_vptr)(raw + e0), 16, 0, 0);
        }
    };
    uint64_t row = blockIdx.x;
    const uint32_t tid8 = tid * 8;
    const uint32_t raw_addr = (uint32_t)(uintptr_t)(lds_vptr)raw + tid8;      // LDS byte address of this thread's first element
    // the eight mid twiddles of a thread are the same for every row: held in registers by the persistent block (the LDS limit of two blocks per CU
    // leaves 128 VGPRs per lane; a load inside the loop would be waited for with vmcnt(0) and drain the DMA in flight)
    uint64_t tw[8];
#pragma unroll
    for (int s = 0; s < 8; s++) tw[s] = a.mid[64 * (8 * w + s) + lane];
    if (row < total_rows) dma_row(row_ptr(row, a.in, a.in_col_stride));
    bool first = true;
    while (row < total_rows) {
        const uint64_t next = row + gridDim.x;
        // this row's DMA pieces have landed (they are older than the previous row's 8 stores), then everybody's
        if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        first = false;
        GL355_L24D_BARRIER();
        L24 y[8], z[8];
        {
            // the raw row through ds_read_b64 written out: as C loads the compiler orders them behind "the DMA that may still be in flight" with a
            // vmcnt(0) of its own, which would also wait for the previous row's stores
            uint64_t x[8];
            asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %8 offset:4096\n\tds_read_b64 %2, %8 offset:8192\n\tds_read_b64 %3, %8 offset:12288\n\t"
                         "ds_read_b64 %4, %8 offset:16384\n\tds_read_b64 %5, %8 offset:20480\n\tds_read_b64 %6, %8 offset:24576\n\tds_read_b64 %7, %8 offset:28672\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]), "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7]) : "v"(raw_addr) : "memory");
#pragma unroll
            for (int q = 0; q < 8; q++) y[q] = l24_split(x[q]);
        }
        dif8_l24<false>(y);
        l24_twiddles_r<6, false>(y, w);
#pragma unroll
        for (int q = 0; q < 8; q++) lp[cA1 + 520 * q] = make_int2(y[q].l[0], y[q].l[1]);
        GL355_L24D_BARRIER();                                  // the raw row has been consumed by every thread
        if (next < total_rows) dma_row(row_ptr(next, a.in, a.in_col_stride));
#pragma unroll
        for (int r = 0; r < 8; r++) { const int2 t = lp[cA2 + 65 * r]; z[r].l[0] = t.x; z[r].l[1] = t.y; }
        GL355_L24D_BARRIER();
#pragma unroll
        for (int q = 0; q < 8; q++) lp[cA1 + 520 * q] = make_int2(y[q].l[2], y[q].l[3]);
        GL355_L24D_BARRIER();
#pragma unroll
        for (int r = 0; r < 8; r++) { const int2 t = lp[cA2 + 65 * r]; z[r].l[2] = t.x; z[r].l[3] = t.y; }
        dif8_l24<false>(z);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            lds_raw[cA2 + 65 * s] = gl_mul(l24_value(z[s]), tw[s]);
            if (s & 1) __builtin_amdgcn_sched_barrier(0);
        }
        GL355_L24D_BARRIER();
#pragma unroll
        for (int q = 0; q < 8; q++) y[q] = l24_split(lds_raw[cB1 + 8 * q]);
        dif8_l24<false>(y);
        l24_twiddles_r<6, false>(y, w);
#pragma unroll
        for (int q = 0; q < 8; q++) lp[cB1 + 8 * q] = make_int2(y[q].l[0], y[q].l[1]);
        GL355_L24D_BARRIER();
#pragma unroll
        for (int r = 0; r < 8; r++) { const int2 t = lp[cB2 + r]; z[r].l[0] = t.x; z[r].l[1] = t.y; }
        GL355_L24D_BARRIER();
#pragma unroll
        for (int q = 0; q < 8; q++) lp[cB1 + 8 * q] = make_int2(y[q].l[2], y[q].l[3]);
        GL355_L24D_BARRIER();
#pragma unroll
        for (int r = 0; r < 8; r++) { const int2 t = lp[cB2 + r]; z[r].l[2] = t.x; z[r].l[3] = t.y; }
        dif8_l24<false>(z);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            lds_raw[cB2 + s] = gl_canon(l24_value(z[s]));
            if (s & 1) __builtin_amdgcn_sched_barrier(0);
        }
        GL355_L24D_BARRIER();
        const __amdgpu_buffer_rsrc_t rout = l24_row_rsrc(row_ptr(row, a.out, a.out_col_stride));
#pragma unroll
        for (int q = 0; q < 8; q++) l24_row_store(rout, tid8, q, lds_raw[cST + 520 * q]);
        row = next;
        // (the next iteration's first barrier also frees the tile: every thread has read its store-order cells before it gets there)
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Column pass of the LDE over all cosets (the shape of ntt_cols_r8_cosets_kernel<5>): 32 rows x 128 columns per tile, 32 = 8 x 4 with
// omega_32 = 2^78 shift twiddles between the radix-8 and the radix-4 round, the 4-step twiddle (a.step_full) at the store.  Threads
// tid >> 7 = r are wave-uniform.  A thread stores to the same eight places with the same step twiddles for every coset: they are loaded
// once per tile.  blockIdx is mapped so that an XCD
// (blockIdx % 8) only ever touches 4 of the 32 column tiles: its L2 holds those slices of the step / pre / ratio tables.
// Result: profiles/r03_ubench_ntt_l24.txt, r03_ubench_ntt_l24s.txt (against ntt_cols_l24s_cosets_kernel).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr size_t L24_COLS_LDS_BYTES = 4096 * 16;
template <int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE))) ntt_cols_l24_cosets_kernel(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_raw[];
    int4* lq = reinterpret_cast<int4*>(lds_raw);
    constexpr uint32_t LOG_TC = 7, TC = 128;
    const uint32_t tid = threadIdx.x, r = tid >> 7, cc = tid & (TC - 1);
    const uint32_t log_n2 = a.log_rows;                     // 12
    const uint32_t tiles_per_col = (1u << log_n2) >> LOG_TC; // 32
    uint32_t tile, colu;
    if (tiles_per_col == 32) { tile = (blockIdx.x & 7) + 8 * ((blockIdx.x >> 3) & 3); colu = blockIdx.x >> 5; }
    else { tile = blockIdx.x % tiles_per_col; colu = blockIdx.x / tiles_per_col; }
    const uint64_t col = colu, c0 = (uint64_t)tile << LOG_TC;
    const uint64_t* in = a.in + col * a.in_col_stride;
    uint64_t v[8], step[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint64_t gi = ((uint64_t)(r + 4 * q) << log_n2) + c0 + cc;
        v[q] = gl_mul(in[gi], a.pre_full[gi]);
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; t2++)
#pragma unroll
        for (int k = 0; k < 4; k++) step[4 * t2 + k] = a.step_full[((uint64_t)(4 * (r + 4 * t2) + k) << log_n2) + c0 + cc];
    const CosetSlots slots = coset_slots_of(a);
    for (uint32_t c = 0; c < a.n_cosets; c++) {
        if (c) {        // the ratio table is re-read per coset (L2-resident, coalesced) rather than held: 16 VGPRs less, no spills
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = gl_mul(v[q], a.ratio_full[((uint64_t)(r + 4 * q) << log_n2) + c0 + cc]);
        }
        uint64_t* out = a.out + (uint64_t)coset_slot_at(slots, c) * a.coset_out_stride + col * a.out_col_stride;
        L24 y[8];
#pragma unroll
        for (int q = 0; q < 8; q++) y[q] = l24_split(v[q]);
        dif8_l24<false>(y);
        l24_twiddles_r<5, false>(y, r);
#pragma unroll
        for (int q = 0; q < 8; q++) lq[TC * (4 * q + r) + cc] = make_int4(y[q].l[0], y[q].l[1], y[q].l[2], y[q].l[3]);
        __syncthreads();
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {                    // two radix-4 tasks: rows 4 q' + {0..3}, q' = r and r + 4
            const uint32_t qp = r + 4 * t2;
            L24 z[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { const int4 qd = lq[TC * (4 * qp + k) + cc]; z[k].l[0] = qd.x; z[k].l[1] = qd.y; z[k].l[2] = qd.z; z[k].l[3] = qd.w; }
            dif4_l24<false>(z);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t go = ((uint64_t)(4 * qp + k) << log_n2) + c0 + cc;
                out[go] = gl_mul(l24_value(z[k]), step[4 * t2 + k]);
            }
        }
        __syncthreads();
    }
}

}  // namespace gl355
