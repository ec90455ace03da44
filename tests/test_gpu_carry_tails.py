"""The chained rows of the permutation on raw words, through the test hook ops GL355_GL_ROW_DENSE (one MDS layer: psd_mds_rows, psd_fold_multi<4>) and
GL355_GL_ROW_B3 (the rows of a block of three: psd_b3_dot with the lone psd_fold of y_1 / y_2 and psd_fold_multi<4> of the outgoing lanes).  A row's
high chain starts from (al >> 32) + c_hi, and top = ah' >> 32 times EPS goes onto (al_0, ah'_0) with its carry-out repaid; the records put al >> 32 and
the top word at 0, 1 and the largest value a row can reach, the start word at 2^32 - 1, and (al_0, ah'_0) + top EPS on both sides of 2^64.  Every
comparison is exact, against Python integers mod p.  (The product routines' new tail is driven by tests/test_gpu_gl_arith.py and the KAT / proof tests;
its model is tests/test_gl_tail_model.py.)

The CPU test counts, with a restatement of the two chains, how often each case occurs at each position of a four-wide group in what the GPU tests send."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_tables as gpt  # noqa: E402

P = gpt.P
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
EPS = M32
ROW_DENSE, ROW_B3 = 14, 15
MAX_RECORDS = 8192                  # lanes (twelve words, a selector and the constants) over all launches of this file

gpu = pytest.mark.gpu


# ---- the rows as term lists: (coefficient, index into the lane's twelve words) ---------------------------------------------------
def dense_rows():
    m = gpt.mds_matrix()
    return [[(m[r][j], j) for j in range(12)] for r in range(12)]


@functools.lru_cache(maxsize=None)
def block_tables():
    rc = gpt.load_rc()
    return rc, gpt.b3_tables(rc)


def block_rows():
    """row r of PSD_B3_MAC on u = a[0 .. 11], x = a[0 .. 2]: terms u_1 .. u_11, then x_0 ..  (12 / 13 / 14 of them)"""
    _, bt = block_tables()
    return [[(c, t + 1 if t < 11 else t - 11) for t, c in enumerate(row)] for row in bt["rows"]]


def row_events(terms, c, words):
    """-> (al >> 32, start word, top, whether (al_0, ah'_0) + top EPS passes 2^64, exact value) of one chained row"""
    al = (c & M32) + sum(k * (words[j] & M32) for k, j in terms)
    start = (al >> 32) + (c >> 32)
    assert start <= M32, "a record breaks the rows' precondition"
    ahp = start + sum(k * (words[j] >> 32) for k, j in terms)
    x = (al & M32) | ((ahp & M32) << 32)
    return al >> 32, start, ahp >> 32, x + (ahp >> 32) * EPS > M64, c + sum(k * words[j] for k, j in terms)


def edge_constants(rows):
    """per row the constant that puts the start word at 2^32 - 1 under all-ones low halves: c_lo = 2^32 - 1, c_hi = 2^32 - 1 - row sum"""
    return [((M32 - sum(k for k, _ in t)) << 32) | M32 for t in rows]


def steered(terms, c):
    """lanes whose row `terms` lands (al_0, ah'_0) + top EPS on both sides of 2^64: one word w_j carries the row (the one with the smallest and the one
    with the largest coefficient), its high half solved so that ah' = T 2^32 - d: for T = 1, 2 (top word 0 and 1), and for d around T - 1 (the sum
    passes 2^64 iff al_0 + (T - 1)(2^32 - 1) >= d 2^32)"""
    out = []
    single = sorted((k, j) for k, j in terms if k >= 2 and sum(1 for _, jj in terms if jj == j) == 1)
    for k, j in (single[0], single[-1]):
        for lo in (0, M32):
            al = (c & M32) + k * lo
            start = (al >> 32) + (c >> 32)
            t = np.arange(1, min(k, 1 << 16), dtype=np.int64)
            d = (t * (1 << 32) - start) % k
            picks = [0, 1] if len(t) > 1 else [0]
            for near in (0, 1, -1):
                hit = np.flatnonzero(d == t - 1 + near)
                picks += hit[:1].tolist() + hit[-1:].tolist()
            for i in picks:
                h = (int(t[i]) * (1 << 32) - int(d[i]) - start) // k
                if 0 <= h <= M32:
                    w = [0] * 12
                    w[j] = (h << 32) | lo
                    out.append(w)
    return out


def lanes_for(rows, c, seed):
    """the lanes of one launch: fixed words, one-hot words at every position, steered rows, random words"""
    rng = np.random.default_rng(seed)
    lanes = [[v] * 12 for v in (0, M64, M32, M32 << 32, P - 1, P, 1, 1 << 32)]
    for j in range(12):
        for v in (1, M32, M32 << 32, M64, 1 << 32, (1 << 32) | 1):
            w = [0] * 12
            w[j] = v
            lanes.append(w)
    for r, terms in enumerate(rows):
        lanes += steered(terms, c[r])
    lanes += rng.integers(0, 1 << 64, (32, 12), dtype=np.uint64).tolist()
    return lanes


@functools.lru_cache(maxsize=None)
def launches():
    """((op, selector, constants[14], rows[(row index, terms)], lanes), ...): every launch of the GPU tests"""
    rc, bt = block_tables()
    out = []
    d = dense_rows()
    for seed, c in enumerate(([0] * 12, rc[1], rc[26], edge_constants(d))):
        out.append((ROW_DENSE, 0, list(c) + [0, 0], tuple(enumerate(d)), lanes_for(d, c, 0xCA0 + seed)))
    b = block_rows()
    tight = bt["add"][14 * 5: 14 * 6]          # block 5 holds the tightest row (12)
    for seed, c in enumerate(([0] * 14, tight, bt["add"][:14], edge_constants(b))):
        for sel, pick in ((0, [0]), (1, [1]), (2, list(range(2, 14)))):
            sub = [b[r] for r in pick]
            out.append((ROW_B3, sel, list(c), tuple((r, b[r]) for r in pick), lanes_for(sub, [c[r] for r in pick], 0xCB0 + 4 * seed + sel)))
    return tuple(out)


def head_of_b(op, sel, c, n):
    b = np.zeros(n, dtype=np.uint64)
    b[0] = sel
    if op == ROW_DENSE:
        b[2:14] = np.array(c[:12], dtype=np.uint64)
    else:
        for r in range(14):
            b[2 + 2 * r], b[3 + 2 * r] = c[r] & M32, c[r] >> 32
    return b


# ---- CPU: what the records exercise -------------------------------------------------------------------------------------------------
def test_records_meet_every_case_at_every_position():
    total = 0
    for op in (ROW_DENSE, ROW_B3):
        # position in the four-wide group -> counts; the lone folds of y_1 / y_2 are position "lone"
        seen = {}
        for o, sel, c, rows, lanes in launches():
            if o != op:
                continue
            total += len(lanes)
            for k, (r, terms) in enumerate(rows):
                pos = "lone" if (op == ROW_B3 and sel < 2) else k % 4
                s = seen.setdefault(pos, dict(carry0=0, carry1=0, carry_max=0, top0=0, top1=0, top_max=0, start_max=0, passes=0, stays_near=0))
                ones = row_events(terms, c[r], [M64] * 12)
                for w in lanes:
                    carry, start, top, passes, _ = row_events(terms, c[r], w)
                    s["carry0"] += carry == 0; s["carry1"] += carry == 1; s["carry_max"] += carry == ones[0] and carry > 1
                    s["top0"] += top == 0; s["top1"] += top == 1; s["top_max"] += top == ones[2] and top > 1
                    s["start_max"] += start == M32
                    s["passes"] += passes
                    # did not pass, but a top word larger by two would have: within reach of the crossing
                    s["stays_near"] += (not passes) and top >= 1 and near_pass(terms, c[r], w)
        print("op %d: %s" % (op, seen))
        assert set(seen) == ({0, 1, 2, 3} if op == ROW_DENSE else {0, 1, 2, 3, "lone"})
        for pos, s in seen.items():
            assert all(v >= 4 for v in s.values()), (op, pos, s)
            assert s["passes"] >= 16 and s["stays_near"] >= 16, (op, pos, s)
    print("%d records in all" % total)
    assert total <= MAX_RECORDS


def near_pass(terms, c, w):
    al = (c & M32) + sum(k * (w[j] & M32) for k, j in terms)
    ahp = (al >> 32) + (c >> 32) + sum(k * (w[j] >> 32) for k, j in terms)
    x = (al & M32) | ((ahp & M32) << 32)
    return x + ((ahp >> 32) + 2) * EPS > M64


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def run_launch(ctx, op, sel, c, rows, lanes):
    a = np.array(lanes, dtype=np.uint64).reshape(-1)
    got = ctx.gl_arith_batch(op, a, head_of_b(op, sel, c, a.size)).reshape(-1, 12)
    n_out = 1 if (op == ROW_B3 and sel < 2) else 12
    for i, w in enumerate(lanes):
        for k, (r, terms) in enumerate(rows):
            want = row_events(terms, c[r], w)[4] % P
            assert int(got[i, k]) % P == want, "op %d selector %d lane %d row %d: got %x want %x (mod p)" % (op, sel, i, r, int(got[i, k]), want)
        assert not got[i, n_out:].any() if n_out == 1 else True


@gpu
def test_chained_dense_rows(ctx):
    for op, sel, c, rows, lanes in launches():
        if op == ROW_DENSE:
            run_launch(ctx, op, sel, c, rows, lanes)


@gpu
@pytest.mark.parametrize("sel", [0, 1, 2])
def test_chained_block_rows(ctx, sel):
    for op, s, c, rows, lanes in launches():
        if op == ROW_B3 and s == sel:
            run_launch(ctx, op, s, c, rows, lanes)


@gpu
def test_row_ops_refuse_what_they_cannot_run(ctx):
    import ctypes as C
    a = np.zeros(24, dtype=np.uint64)
    out = np.zeros(24, dtype=np.uint64)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for op in (ROW_DENSE, ROW_B3):
        assert ctx.lib.gl355_gl_arith_batch(ctx.h, op, pa, pa, po, 24) == -1          # the constants need 30 words of b
        assert ctx.lib.gl355_gl_arith_batch(ctx.h, op, pa, pa, po, 13) == -1
        assert ctx.lib.gl355_gl_arith_batch(ctx.h, op, pa, None, po, 36) == -1
        assert ctx.lib.gl355_gl_arith_batch(ctx.h, op, None, None, None, 0) == 0
