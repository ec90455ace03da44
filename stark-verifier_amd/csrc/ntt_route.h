// The route of a Goldilocks NTT as data: which pass kernels run for a transform, in which order, with which tables (a2, a3 of SURVEY.md 8).
// Pure host code without a HIP include, so that tests/ntt_route_check.cpp can build it alone under the host sanitizers, like merkle_update_plan.h.
//   NttShape              what the decision reads of an NttPlan and of the context, and nothing else
//   ntt_route             shape -> at most four NttSteps in launch order, or the refusal code and message
//   GL355_NTT_*_INSTANCES the (form, template arguments) that are compiled: the dispatch of ntt.hip / ntt_r8.hip / ntt_l24.hip and
//                         ntt_instance_listed both expand them, so a route cannot name a kernel that does not exist
//   ntt_step_grid         the grid of a step
// ntt_run (ntt.hip) builds the shape, fetches the tables the steps name, fills one PassArgs per step and dispatches.  The sizes at which a form
// was measured against its neighbours are in DESIGN.md 4.1; docs/history/ntt_route.md has the route of every shape the callers can build.
#pragma once
#include <stdint.h>

#include "../../include/gl355.h"

namespace gl355 {

struct NttShape {
    uint32_t log_n = 0, n_cosets = 1;
    bool inverse = false, in_bitrev = false, out_bitrev = false;
    bool pre = false, post = false;      // multiplier tables on the natural-order input / output index
    bool scale = false;                  // a constant multiplier != 1 at the store
    bool ratio = false;                  // the coset bases are base[0] * ratio^c
    bool out_contig = false;             // out_col_stride == n
    bool cosets_contig = false;          // coset_out_stride == n
    bool slot0_zero = true;              // coset_slot[0] == 0
    bool batch_fits_y = true;            // batch <= 65535: the batch may be a grid's second dimension
    uint32_t single_pass_max_log = 12;   // Ctx::ntt_single_pass_max_log
};

enum NttForm : uint8_t {
    NTT_POINTS,             // canon_points_kernel: n = 1
    NTT_ROWS16,             // ntt_rows_kernel<LT, LOG_T, INV>
    NTT_COLS16,             // ntt_cols_kernel<LOG_T, INV>
    NTT_ROWS8,              // ntt_rows_r8_kernel<LT, PRE, INV>
    NTT_COLS8,              // ntt_cols_r8_kernel<LOG_T, PRE> on 4096-element tiles
    NTT_COLS8_BIG,          // ntt_cols_r8_kernel<LOG_T, false, LT = 13>: 8192-element tiles
    NTT_COLS8_COSETS,       // ntt_cols_r8_cosets_kernel<LOG_T>: all cosets of a tile in one block
    NTT_COLS8_NAT,          // ntt_cols_r8_nat_kernel<LT, LOG_T, PASS>: natural -> natural in two column-type passes
    NTT_ROWS_L24,           // ntt_rows_l24s_kernel: 4096-point rows on 24-bit limbs
    NTT_COLS_L24_COSETS,    // ntt_cols_l24s_cosets_kernel: 32-point columns over all cosets
    NTT_COLS_SMALL_COSETS,  // ntt_cols_small_cosets_kernel<LOG_T>: 2 .. 8-point columns, streaming
    NTT_BITREV,             // bitrev_permute of the whole output, in place
    NTT_FORMS
};
static const char* const NTT_FORM_NAME[NTT_FORMS] = {"points", "rows16", "cols16", "rows8", "cols8", "cols8_big", "cols8_cosets", "cols8_nat",
                                                     "rows_l24", "cols_l24_cosets", "cols_small_cosets", "bitrev"};

// a multiplier table in the form a kernel reads it
enum NttTab : uint8_t {
    NTT_TAB_NONE,
    NTT_TAB_ONE_LEVEL,          // lo[4096] alone: n <= 2^12
    NTT_TAB_TWO_LEVEL,          // g^e = lo[e & 4095] * hi[e >> 12]
    NTT_TAB_FULL,               // one word per element (Ctx::full_pow_table / full_step_table)
    NTT_TAB_ONE_LEVEL_AS_FULL,  // n <= 2^12: the one-level table is the full one
    NTT_TAB_NAT,                // the step table in the store order of the natural -> natural flow (Ctx::nat_step_table)
};
static const char* const NTT_TAB_NAME[] = {"", "1", "2", "full", "1full", "nat"};

enum NttBuf : uint8_t { NTT_BUF_IN, NTT_BUF_OUT, NTT_BUF_MID };   // the plan's input, its output, a scratch copy of the transform at stride n

struct NttStep {
    NttForm form = NTT_POINTS;
    uint8_t lt = 12, log_t = 0, pre = 0, inv = 0, pass = 0;   // the instance: tile, transform dimension of this pass, PRE, INV, PASS
    uint8_t log_rows = 0;            // PassArgs::log_rows
    uint8_t xform_log_n = 0;         // the transform this pass belongs to: the whole one, or a 2^17-point row of the three-pass form
    uint8_t batch_shift = 0;         // != 0: the rows of the three-pass form, batch << batch_shift transforms of 2^xform_log_n contiguous points in the output
    bool fetch_step_root = false;    // first pass of a multi-pass transform: fetch the two-level tables of omega_(2^xform_log_n)^(+-1) here
    NttTab pre_tab = NTT_TAB_NONE, step_tab = NTT_TAB_NONE, post_tab = NTT_TAB_NONE;
    bool ratio_tab = false, mid_tab = false, scale = false;
    bool in_bitrev = false, out_natural = false, canon = false;
    bool collapse_cosets = false;    // second pass of a multi-coset LDE: the coset blocks tile the column, (column, coset) pairs are rows
    NttBuf src = NTT_BUF_IN, dst = NTT_BUF_OUT;
    const char* scope = "";          // profile scope
    uint32_t bytes_per_point = 0;    // algorithmic HBM bytes of the step = (batch << log_n) * this
};

struct NttRoute {
    uint32_t n_steps = 0;
    NttStep step[4];
    const char* msg = "";            // of a refusal
};

// X(LT, LOG_T, PRE, INV, PASS) per compiled instance of a form; an argument the form does not have is 0 (LT: 12).
#define GL355_NTT_ROWS16_INSTANCES(X)                                                                                                          \
    X(12, 1, 0, 0, 0) X(12, 2, 0, 0, 0) X(12, 3, 0, 0, 0) X(12, 4, 0, 0, 0) X(12, 5, 0, 0, 0) X(12, 6, 0, 0, 0) X(12, 7, 0, 0, 0)                \
    X(12, 8, 0, 0, 0) X(12, 9, 0, 0, 0) X(12, 10, 0, 0, 0) X(12, 11, 0, 0, 0) X(12, 12, 0, 0, 0) X(13, 13, 0, 0, 0) X(14, 14, 0, 0, 0)           \
    X(12, 1, 0, 1, 0) X(12, 2, 0, 1, 0) X(12, 3, 0, 1, 0) X(12, 4, 0, 1, 0) X(12, 5, 0, 1, 0) X(12, 6, 0, 1, 0) X(12, 7, 0, 1, 0)                \
    X(12, 8, 0, 1, 0) X(12, 9, 0, 1, 0) X(12, 10, 0, 1, 0) X(12, 11, 0, 1, 0) X(12, 12, 0, 1, 0) X(13, 13, 0, 1, 0) X(14, 14, 0, 1, 0)
#define GL355_NTT_COLS16_INSTANCES(X)                                                                                                          \
    X(12, 6, 0, 0, 0) X(12, 7, 0, 0, 0) X(12, 8, 0, 0, 0) X(12, 9, 0, 0, 0) X(12, 10, 0, 0, 0)                                                  \
    X(12, 3, 0, 1, 0) X(12, 4, 0, 1, 0) X(12, 5, 0, 1, 0) X(12, 6, 0, 1, 0) X(12, 7, 0, 1, 0) X(12, 8, 0, 1, 0) X(12, 9, 0, 1, 0) X(12, 10, 0, 1, 0)
#define GL355_NTT_ROWS8_INSTANCES(X)                                                                                                           \
    X(12, 12, 1, 0, 0) X(13, 13, 1, 0, 0) X(14, 14, 1, 0, 0) X(14, 14, 0, 0, 0) X(12, 12, 0, 1, 0) X(13, 13, 0, 1, 0) X(14, 14, 0, 1, 0)
#define GL355_NTT_COLS8_INSTANCES(X)                                                                                                           \
    X(12, 1, 1, 0, 0) X(12, 2, 1, 0, 0) X(12, 3, 1, 0, 0) X(12, 4, 1, 0, 0) X(12, 5, 1, 0, 0) X(12, 6, 1, 0, 0) X(12, 7, 1, 0, 0) X(12, 8, 1, 0, 0) \
    X(12, 5, 0, 0, 0) X(12, 6, 0, 0, 0) X(12, 7, 0, 0, 0)
#define GL355_NTT_COLS8_BIG_INSTANCES(X) X(13, 9, 0, 0, 0) X(13, 10, 0, 0, 0)
#define GL355_NTT_COLS8_COSETS_INSTANCES(X)                                                                                                    \
    X(12, 1, 0, 0, 0) X(12, 2, 0, 0, 0) X(12, 3, 0, 0, 0) X(12, 4, 0, 0, 0) X(12, 6, 0, 0, 0) X(12, 7, 0, 0, 0) X(12, 8, 0, 0, 0)
#define GL355_NTT_COLS8_NAT_INSTANCES(X)                                                                                                       \
    X(12, 8, 0, 0, 0) X(12, 9, 0, 0, 0) X(13, 10, 0, 0, 0) X(12, 7, 0, 0, 1) X(12, 8, 0, 0, 1) X(12, 9, 0, 0, 1) X(13, 10, 0, 0, 1)
#define GL355_NTT_COLS_SMALL_COSETS_INSTANCES(X) X(12, 1, 0, 0, 0) X(12, 2, 0, 0, 0) X(12, 3, 0, 0, 0)
// every list under its form; the forms without template arguments have the one instance
#define GL355_NTT_ALL_INSTANCES(F)                                                                                                             \
    F(NTT_POINTS, GL355_NTT_ONE_INSTANCE) F(NTT_ROWS16, GL355_NTT_ROWS16_INSTANCES) F(NTT_COLS16, GL355_NTT_COLS16_INSTANCES)                   \
    F(NTT_ROWS8, GL355_NTT_ROWS8_INSTANCES) F(NTT_COLS8, GL355_NTT_COLS8_INSTANCES) F(NTT_COLS8_BIG, GL355_NTT_COLS8_BIG_INSTANCES)             \
    F(NTT_COLS8_COSETS, GL355_NTT_COLS8_COSETS_INSTANCES) F(NTT_COLS8_NAT, GL355_NTT_COLS8_NAT_INSTANCES)                                       \
    F(NTT_ROWS_L24, GL355_NTT_ROWS_L24_INSTANCES) F(NTT_COLS_L24_COSETS, GL355_NTT_COLS_L24_COSETS_INSTANCES)                                   \
    F(NTT_COLS_SMALL_COSETS, GL355_NTT_COLS_SMALL_COSETS_INSTANCES) F(NTT_BITREV, GL355_NTT_ONE_INSTANCE)
#define GL355_NTT_ONE_INSTANCE(X) X(12, 0, 0, 0, 0)
#define GL355_NTT_ROWS_L24_INSTANCES(X) X(12, 12, 0, 0, 0)
#define GL355_NTT_COLS_L24_COSETS_INSTANCES(X) X(12, 5, 0, 0, 0)
#define GL355_NTT_STEP_IS(st, LT, LOG_T, PRE, INV, PASS) ((st).lt == LT && (st).log_t == LOG_T && (st).pre == PRE && (st).inv == INV && (st).pass == PASS)

// calls f(form, lt, log_t, pre, inv, pass) for every compiled instance
template <class F>
inline void ntt_for_each_instance(F f) {
#define GL355_NTT_VISIT(LT, LOG_T, PRE, INV, PASS) f(form, LT, LOG_T, PRE, INV, PASS);
#define GL355_NTT_VISIT_FORM(FORM, LIST) { const NttForm form = FORM; (void)form; LIST(GL355_NTT_VISIT) }
    GL355_NTT_ALL_INSTANCES(GL355_NTT_VISIT_FORM)
#undef GL355_NTT_VISIT_FORM
#undef GL355_NTT_VISIT
}
inline bool ntt_instance_listed(const NttStep& st) {
    bool found = false;
    ntt_for_each_instance([&](NttForm form, int lt, int log_t, int pre, int inv, int pass) {
        if (form == st.form && GL355_NTT_STEP_IS(st, lt, log_t, pre, inv, pass)) found = true;
    });
    return found;
}

// The grid of a step over `batch` columns and `n_cosets` cosets as its PassArgs carry them (the batch shifted and the cosets collapsed already);
// y == 0: the step launches nothing of its own (NTT_BITREV: bitrev_permute picks its kernel and grid)
struct NttGrid { uint64_t x; uint32_t y; };
inline NttGrid ntt_step_grid(const NttStep& st, uint64_t batch, uint32_t n_cosets) {
    const uint64_t rows = batch << st.log_rows;                                  // row kernels: rows of 2^log_t points
    const uint64_t tiles = ((1ull << st.log_rows) >> (st.lt - st.log_t)) * batch;   // column kernels: tiles of 2^(lt - log_t) adjacent columns
    switch (st.form) {
        case NTT_POINTS: return {(batch + 255) / 256, 1};
        case NTT_ROWS16: { const uint64_t rpt = 1ull << (st.lt - st.log_t); return {(rows + rpt - 1) / rpt * n_cosets, 1}; }
        case NTT_ROWS8: return {rows * n_cosets, 1};
        case NTT_ROWS_L24: return {rows, 1};
        case NTT_COLS16: case NTT_COLS8: case NTT_COLS8_BIG: return {tiles * n_cosets, 1};
        case NTT_COLS8_COSETS: case NTT_COLS8_NAT: return {tiles, 1};
        case NTT_COLS_L24_COSETS: return {((1ull << st.log_rows) >> 6) * batch, 1};
        case NTT_COLS_SMALL_COSETS: return {(1ull << st.log_rows) / 256, (uint32_t)batch};
        default: return {0, 0};
    }
}

namespace ntt_route_detail {

inline int32_t refuse(NttRoute& r, int32_t code, const char* msg) { r.n_steps = 0; r.msg = msg; return code; }

inline NttStep& add_step(NttRoute& r, const NttShape& s, const char* scope, uint32_t bytes_per_point) {
    NttStep& st = r.step[r.n_steps++];
    st = NttStep();
    st.inv = s.inverse;
    st.xform_log_n = (uint8_t)s.log_n;
    st.scope = scope;
    st.bytes_per_point = bytes_per_point;
    return st;
}

// the row kernel of a pass over rows of 2^log_t points whose tables and flags are set; n_cosets as the pass sees them
inline void pick_rows(NttStep& st, uint32_t log_t, uint32_t n_cosets, bool limb_rows) {
    const bool inv = st.inv, plain_io = !st.in_bitrev && st.canon && st.post_tab == NTT_TAB_NONE, tile = log_t >= 12 && log_t <= 14;
    st.log_t = (uint8_t)log_t;
    st.lt = (uint8_t)(log_t <= 12 ? 12 : log_t);
    if (limb_rows && !inv && log_t == 12 && n_cosets == 1 && st.pre_tab == NTT_TAB_NONE && plain_io && !st.scale && !st.out_natural) {
        // 4096-point rows of the two-pass LDE / forward transform on 24-bit limbs
        st.form = NTT_ROWS_L24;
        st.mid_tab = true;
    } else if (!inv && tile && plain_io && !st.scale && !st.out_natural && st.pre_tab != NTT_TAB_TWO_LEVEL) {
        // the commit-path shape: forward, whole rows of 2^12 .. 2^14 points in natural order, at most a full pre table
        st.form = NTT_ROWS8;
        if (st.pre_tab == NTT_TAB_ONE_LEVEL) st.pre_tab = NTT_TAB_ONE_LEVEL_AS_FULL;
        st.pre = st.pre_tab != NTT_TAB_NONE;
    } else if (inv && tile && plain_io && st.pre_tab == NTT_TAB_NONE) {
        // values -> coefficients without multiplier tables: natural order within the row and the 1/n at the store
        st.form = NTT_ROWS8;
    } else {
        st.form = NTT_ROWS16;
    }
}

// the column kernel of a first or second pass over 2^log_t points whose tables and flags are set
inline void pick_cols(NttStep& st, uint32_t log_t, bool batch_fits_y) {
    const bool inv = st.inv;
    st.log_t = (uint8_t)log_t;
    const bool r8 = st.step_tab == NTT_TAB_FULL && (st.pre_tab == NTT_TAB_NONE || (!inv && st.pre_tab == NTT_TAB_FULL)) && !st.in_bitrev &&
                    !st.out_natural && st.post_tab == NTT_TAB_NONE && !st.scale && !st.canon;
    const bool all_cosets = r8 && !inv && st.ratio_tab && st.pre_tab == NTT_TAB_FULL;
    if (all_cosets && log_t == 5 && st.log_rows == 12) st.form = NTT_COLS_L24_COSETS;
    // column dimension 2, 4 or 8 (n = 2^13 .. 2^15 with 4096-point rows): the streaming kernel, no tile
    else if (all_cosets && log_t <= 3 && st.log_rows == 12 && batch_fits_y) st.form = NTT_COLS_SMALL_COSETS;
    else if (all_cosets) st.form = NTT_COLS8_COSETS;
    else if (r8) { st.form = NTT_COLS8; st.pre = st.pre_tab == NTT_TAB_FULL; }
    else st.form = NTT_COLS16;
}

}  // namespace ntt_route_detail

inline int32_t ntt_route(const NttShape& s, NttRoute& r) {
    using namespace ntt_route_detail;
    r.n_steps = 0;
    r.msg = "";
    const uint32_t log_n = s.log_n;
    if (log_n == 0) {
        // the transform of a single point is that point: what is left of the contract is the canonical output
        add_step(r, s, "ntt_single_points", 16).inv = 0;
        return GL355_OK;
    }
    if (log_n > 24) return refuse(r, GL355_E_UNSUPPORTED, "ntt: log_n > 24 unsupported");
    if (s.n_cosets > 16 || s.n_cosets == 0) return refuse(r, GL355_E_INVALID_ARG, "ntt: bad coset count");
    const bool inv = s.inverse;
    const auto listed = [&]() {
        for (uint32_t i = 0; i < r.n_steps; i++)
            if (!ntt_instance_listed(r.step[i])) return refuse(r, GL355_E_UNSUPPORTED, "ntt: no kernel is compiled for a pass of this shape");
        return (int32_t)GL355_OK;
    };

    // n = 2^13, 2^14 in one pass need a 64 / 128-KB LDS tile and every VGPR of the CU: nothing else can share the CU with such a block.
    // single_pass_max_log < 14 sends the commit-path shape (natural in, bit-reversed out, no post-multiplier, contiguous coset blocks) of those
    // sizes through the two-pass path with 4096-point tiles instead.
    const bool two_pass_ok = !s.in_bitrev && s.out_bitrev && !s.post && (s.n_cosets == 1 || s.cosets_contig);
    if (log_n <= 12 || (log_n <= 14 && !(two_pass_ok && log_n > s.single_pass_max_log))) {
        NttStep& st = add_step(r, s, "ntt_rows_single_pass", 8 * (1 + s.n_cosets));
        // above 2^12 two-level lookups would cost an extra modmul per element
        st.pre_tab = !s.pre ? NTT_TAB_NONE : log_n > 12 ? NTT_TAB_FULL : NTT_TAB_ONE_LEVEL;
        st.post_tab = !s.post ? NTT_TAB_NONE : log_n > 12 ? NTT_TAB_TWO_LEVEL : NTT_TAB_ONE_LEVEL;
        st.scale = s.scale;
        st.in_bitrev = s.in_bitrev; st.out_natural = !s.out_bitrev; st.canon = true;
        pick_rows(st, log_n, s.n_cosets, false);
        return listed();
    }

    // natural order in AND out, plain forward transform of 2^14 < n <= 2^20 points: two column-type passes with the transposition in LDS
    // instead of two passes + the bit-reversal pass
    const bool plain_fwd = !inv && s.n_cosets == 1 && !s.pre && !s.post && !s.scale && s.slot0_zero;
    if (plain_fwd && !s.in_bitrev && !s.out_bitrev && log_n <= 20) {
        const uint32_t l2 = log_n / 2, l1 = log_n - l2;                          // l1 >= l2; both <= 10
        for (int pass = 0; pass < 2; pass++) {
            NttStep& st = add_step(r, s, pass ? "ntt_cols_pass2" : "ntt_cols_pass1", 8);
            st.form = NTT_COLS8_NAT;
            st.pass = (uint8_t)pass;
            st.log_t = (uint8_t)(pass ? l2 : l1);
            st.log_rows = (uint8_t)(pass ? l1 : l2);                             // the row stride of the matrix the pass walks
            st.lt = st.log_t <= 9 ? 12 : 13;                                     // 4096-element tiles while 8 adjacent columns fit
            st.fetch_step_root = !pass;
            st.step_tab = pass ? NTT_TAB_NONE : NTT_TAB_NAT;
            st.src = pass ? NTT_BUF_MID : NTT_BUF_IN;
            st.dst = pass ? NTT_BUF_OUT : NTT_BUF_MID;
        }
        return listed();
    }

    // Split of a two-pass transform N = N1 * N2.  The column pass works on tiles of 2^(12 - LOG_T) adjacent columns: with 4096-point rows a
    // 2^22 / 2^23-point transform leaves it 4 / 2 columns, so from 2^22 on the row dimension is 2^14.
    const uint32_t row = log_n >= 22 ? 14 : 12;
    if (!s.in_bitrev) {
        // natural in -> (cols over N1, twiddle at store) -> (rows over N2) -> bit-reversed out
        uint32_t l1 = log_n - row, l2 = row;
        // Plain forward transforms into contiguous columns.  From 2^22 points on THREE passes over 4096-element tiles beat two with 16384-point rows:
        // after the column pass over N1 = N / 2^17 the rows are independent 2^17-point transforms, each the usual column + row pair.  At 2^21 and
        // 2^22 TWO passes with 4096-point limb rows and a column pass on 8192-element tiles beat both (2^23 measured slower that way).
        const bool three = plain_fwd && s.out_contig && log_n >= 22, big = plain_fwd && s.out_contig && log_n >= 21 && log_n <= 22;
        if (big) { l2 = 12; l1 = log_n - l2; }
        else if (three) { l2 = 17; l1 = log_n - l2; }
        // full-size tables (<= 8 MiB each; the three-pass form: up to 128 MiB): 1 load + 1 modmul per element instead of 2 + 2
        const bool full = log_n <= 20 || three || big;
        NttStep& a = add_step(r, s, "ntt_cols_pass1", 8);
        a.fetch_step_root = true;
        a.log_rows = (uint8_t)l2;
        a.pre_tab = !s.pre ? NTT_TAB_NONE : (full && ((uint64_t)s.n_cosets << log_n) <= (1ull << 21)) ? NTT_TAB_FULL : NTT_TAB_TWO_LEVEL;
        a.step_tab = full ? NTT_TAB_FULL : NTT_TAB_TWO_LEVEL;
        a.ratio_tab = full && a.pre_tab == NTT_TAB_FULL && s.n_cosets > 1 && s.ratio;
        if (big) { a.form = NTT_COLS8_BIG; a.lt = 13; a.log_t = (uint8_t)l1; }
        else pick_cols(a, l1, s.batch_fits_y);
        if (three && !big) {
            NttShape sub;
            sub.log_n = l2; sub.out_bitrev = true; sub.out_contig = true; sub.batch_fits_y = false; sub.single_pass_max_log = s.single_pass_max_log;
            NttRoute rows;
            const int32_t rc = ntt_route(sub, rows);
            if (rc != GL355_OK) return refuse(r, rc, rows.msg);
            for (uint32_t i = 0; i < rows.n_steps; i++) {
                NttStep& st = r.step[r.n_steps++] = rows.step[i];
                st.batch_shift = (uint8_t)l1;
                st.src = st.dst = NTT_BUF_OUT;
            }
        } else {
            // each coset's intermediate lives in its own output block
            NttStep& b = add_step(r, s, "ntt_rows_pass2", 8);
            b.src = NTT_BUF_OUT;
            b.log_rows = (uint8_t)l1;
            b.scale = s.scale; b.canon = true;
            if (s.n_cosets != 1) {
                // the coset blocks are contiguous sub-ranges of every output column: (column, coset) pairs are 2^l1 * n_cosets rows per column
                if (!s.cosets_contig) return refuse(r, GL355_E_INVALID_ARG, "ntt: multi-coset two-pass needs contiguous coset blocks");
                uint32_t lc = 0;
                while ((1u << lc) < s.n_cosets) lc++;
                b.collapse_cosets = true;
                b.log_rows = (uint8_t)(l1 + lc);
                b.bytes_per_point = 8 * s.n_cosets;
            }
            pick_rows(b, l2, 1, true);
        }
        if (!s.out_bitrev) {
            // natural order requested: one extra permutation pass (not used on the commit path)
            if (s.n_cosets != 1) return refuse(r, GL355_E_UNSUPPORTED, "ntt: natural-order multi-coset output is done by the caller");
            add_step(r, s, "bitrev_permute", 16).form = NTT_BITREV;
            r.step[r.n_steps - 1].inv = 0;
            r.step[r.n_steps - 1].src = NTT_BUF_OUT;
        }
        if (s.post) return refuse(r, GL355_E_UNSUPPORTED, "ntt: post-multiplier needs natural-order output from the bitrev-input flow");
        return listed();
    }
    // bit-reversed in -> (rows over N1, natural within row) -> (cols over N2, twiddle at load) -> natural out
    if (s.n_cosets != 1) return refuse(r, GL355_E_UNSUPPORTED, "ntt: bitrev-input flow is single-coset");
    if (s.out_bitrev) return refuse(r, GL355_E_UNSUPPORTED, "ntt: bitrev -> bitrev not provided");
    const uint32_t l1 = row, l2 = log_n - row;
    NttStep& a = add_step(r, s, "ntt_bitrev_in_rows_pass1", 8);
    a.fetch_step_root = true;
    a.log_rows = (uint8_t)l2;                                                    // row index = bitrev(i2)
    a.in_bitrev = a.out_natural = true;
    pick_rows(a, l1, 1, false);
    NttStep& b = add_step(r, s, "ntt_bitrev_in_cols_pass2", 8);
    b.src = NTT_BUF_OUT;
    b.log_rows = (uint8_t)l1;                                                    // the matrix is [N2 rows][N1 columns]
    b.step_tab = NTT_TAB_TWO_LEVEL;
    b.post_tab = s.post ? NTT_TAB_TWO_LEVEL : NTT_TAB_NONE;
    b.scale = s.scale; b.canon = true;
    b.in_bitrev = b.out_natural = true;
    pick_cols(b, l2, s.batch_fits_y);
    return listed();
}

}  // namespace gl355
