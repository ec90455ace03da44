"""GPU: the MSM configurations that a bit length selects (msm_plan in csrc/bn254_msm.hip: a cut window count, the one-window form, the same cut on
prepared bases) and the prover's commit_columns that chooses them (csrc/plonk_bn254.hip), at their boundaries, through the two test hooks
gl355_bn254_g1_msm_bits and gl355_plonk_pk_commit_columns.  Every comparison is exact: against the oracle's MSM up to 4096 points, above that
against one scalar multiplication of G (bases that are known multiples of G).  Every test first holds the plan the library reports to the Python
restatement (tests/pymodel_msm_plan.py), so a case that does not reach the path it names fails instead of passing.  A scalar that the planned
digits cannot hold is an error, never a wrong point."""
import numpy as np
import pytest

import pymodel_bn254_curve as pm
import pymodel_msm_plan as mp
from oracle_lib import Bn254Curve
from test_gpu_bn254_curve import PreparedBases, gpu_fixed_base, gpu_msm
from test_gpu_halo2 import TAU, build, h2

pytestmark = pytest.mark.gpu
E_INVALID_ARG = -1
U64 = (1 << 64) - 1


def msm_bits(ctx, pts, sc, max_bits, bases=None, rc_only=False):
    """gl355_bn254_g1_msm_bits -> ([sets][8] results, plan) or, with rc_only, the return code"""
    sc = np.ascontiguousarray(sc, dtype=np.uint64)
    sc = sc.reshape((-1,) + sc.shape[-2:])
    m, n = sc.shape[0], sc.shape[1]
    out = np.zeros((m, 8), dtype=np.uint64)
    plan = np.full(4, 0xAA, dtype=np.uint32)
    p = None if pts is None else np.ascontiguousarray(pts, dtype=np.uint64)
    rc = ctx.lib.gl355_bn254_g1_msm_bits(ctx.h, None if p is None else p.ctypes.data, bases.h if bases is not None else None, sc.ctypes.data, n, m, max_bits,
                                         out.ctypes.data, plan.ctypes.data)
    if rc_only:
        return rc
    ctx.check(rc)
    return out, [int(v) for v in plan]


def limbs_of(v):
    return [(v >> (64 * i)) & U64 for i in range(4)]


def const_scalars(n, v):
    a = np.zeros((n, 4), dtype=np.uint64)
    a[:] = np.array(limbs_of(v), dtype=np.uint64)
    return a


def rand_below(rng, n, bits):
    """n uniform scalars below 2^bits"""
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)
    for limb in range(4):
        keep = min(64, max(0, bits - 64 * limb))
        a[:, limb] &= np.uint64((1 << keep) - 1)
    return a


def to_obj(a):
    v = np.zeros(a.shape[0], dtype=object)
    for limb in range(4):
        v += a[:, limb].astype(object) << (64 * limb)
    return v


def negate(cv, p):
    q = p.copy()
    q[4:] = cv.scalars([pm.Q - cv.ints(p[4:])[0]])[0]
    return q


def boundary_sets(rng, n, max_bits):
    """the three scalar sets of the cut-window cases: every scalar 2^max_bits - 1 (the top digit carries in every window), uniform below 2^max_bits, and a sparse
    set -- one scalar 2^(max_bits - 1), the rest 0 or 1"""
    top = (1 << max_bits) - 1
    sparse = rng.integers(0, 2 if max_bits else 1, size=(n, 4), dtype=np.uint64)
    sparse[:, 1:] = 0
    if max_bits:
        sparse[n // 3] = limbs_of(1 << (max_bits - 1))
    return np.stack([const_scalars(n, top), rand_below(rng, n, max_bits), sparse])


def special_bases(cv, pts):
    """an identity, a repeated base, and a base next to its opposite (callers give the pair one scalar)"""
    pts[2] = 0
    pts[3] = pts[0]
    pts[5] = negate(cv, pts[4])
    return pts


@pytest.mark.parametrize("n", [64, 300, 4096])
def test_cut_window_count_vs_oracle(ctx, orc, n):
    cv = Bn254Curve(orc)
    rng = np.random.default_rng(0x5B0 + n)
    c = mp.plain_c(mp.lg_of(n))
    assert c == {64: 4, 300: 7, 4096: 10}[n]
    pts = special_bases(cv, cv.multiples_array(int(rng.integers(1, 1 << 40)), int(rng.integers(1, 1 << 40)), n))
    for max_bits in sorted({0, 1, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 20, 21, 40, 41, 64, 65, 253, 254, 255}):
        sets = boundary_sets(rng, n, max_bits)
        sets[:, 5] = sets[:, 4]
        out, plan = msm_bits(ctx, pts, sets, max_bits)
        assert plan == mp.plan_of(n, max_bits) and plan[2] == 0 and plan[1] == min(256 // c + 1, (max(1, max_bits) + c - 1) // c + 1), max_bits
        for j in range(3):
            assert np.array_equal(out[j], cv.msm_arrays(pts, sets[j])), (max_bits, j)


_multiples = {}


def multiples_of_3g(cv, n):
    if n not in _multiples:
        _multiples[n] = cv.multiples_array(3, 3, n)
        _multiples[n].setflags(write=False)
    return _multiples[n]


def expect_small(cv, v, weights):
    """(sum_i v_i weights_i mod r) G for values and weights whose products stay below 2^48: exact uint64 dot products over chunks of 2^12"""
    total = 0
    for lo in range(0, v.shape[0], 1 << 12):
        total += int(np.dot(v[lo:lo + (1 << 12)], weights[lo:lo + (1 << 12)]))
    return cv.mul(pm.G, total % pm.R)


@pytest.mark.parametrize("n,bits", [((1 << 14) + 1, (11, 12, 10)), (1 << 16, (11, 12, 13)), ((1 << 18) + 1, (11, 15, 16))])
def test_one_window_form(ctx, orc, n, bits):
    """bases (i + 1) * 3 G; uniform, all 2^max_bits - 1, all equal (one bucket takes every point: the workgroup path inside a one-window plan) and 0 / 1 scalars
    in ONE batched call.  The last max_bits of each size must NOT be one-window (nor 12 at 2^14 + 1: a window of 13 bits is the plain width there)"""
    cv = Bn254Curve(orc)
    rng = np.random.default_rng(0x5B1 + n)
    pts = multiples_of_3g(cv, n)
    weights = 3 * np.arange(1, n + 1, dtype=np.uint64)
    c = mp.plain_c(mp.lg_of(n))
    for max_bits in bits:
        vals = np.stack([rng.integers(0, 1 << max_bits, size=n, dtype=np.uint64), np.full(n, (1 << max_bits) - 1, dtype=np.uint64),
                         np.full(n, (1 << (max_bits - 1)) | 5, dtype=np.uint64), rng.integers(0, 2, size=n, dtype=np.uint64)])
        sc = np.zeros((4, n, 4), dtype=np.uint64)
        sc[:, :, 0] = vals
        out, plan = msm_bits(ctx, pts, sc, max_bits)
        one = 12 <= max_bits + 1 < c
        assert plan == mp.plan_of(n, max_bits) == ([max_bits + 1, 1, 1, 1] if one else [c, 2, 0, 1]), max_bits
        assert one == (max_bits != bits[-1] and (n, max_bits) != ((1 << 14) + 1, 12))
        for j in range(4):
            assert cv._unpt(out[j]) == expect_small(cv, vals[j], weights), (max_bits, j)


def test_one_window_at_the_k23_shape(ctx, orc):
    """the product's k = 23 range-check columns: 2^22 + 1 points (window width 20), 16-bit scalars -> one window of 17 bits; distinct bases s_i G from the
    fixed-base kernel (s_i < 2^32), so the sum is (sum v_i s_i mod r) G"""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip("needs 8 GB of free device memory, %.1f GB free" % (free / 2**30))
    cv = Bn254Curve(orc)
    n = (1 << 22) + 1
    rng = np.random.default_rng(0x5B2)
    s = rng.integers(1, 1 << 32, size=n, dtype=np.uint64)
    ssc = np.zeros((n, 4), dtype=np.uint64)
    ssc[:, 0] = s
    pts = gpu_fixed_base(ctx, cv._pt(pm.G), ssc)
    v = rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    v[7] = 0xFFFF
    sc = np.zeros((n, 4), dtype=np.uint64)
    sc[:, 0] = v
    out, plan = msm_bits(ctx, pts, sc, 16)
    assert plan == mp.plan_of(n, 16) == [17, 1, 1, 1]
    assert cv._unpt(out[0]) == expect_small(cv, v, s)


def test_prepared_cut_window_count_vs_oracle(ctx, orc):
    cv = Bn254Curve(orc)
    n = 4096
    rng = np.random.default_rng(0x5B3)
    pts = special_bases(cv, cv.multiples_array(int(rng.integers(1, 1 << 40)), int(rng.integers(1, 1 << 40)), n))
    pb = PreparedBases(ctx, pts)
    try:
        for max_bits in (12, 13, 24, 40, 60, 100, 256):
            sets = boundary_sets(rng, n, max_bits)
            sets[:, 5] = sets[:, 4]
            out, plan = msm_bits(ctx, None, sets, max_bits, bases=pb)
            assert plan == mp.plan_of(n, max_bits, True) == [12, min(22, (max_bits + 11) // 12 + 1), 0, 1], max_bits
            for j in range(3):
                assert np.array_equal(out[j], cv.msm_arrays(pts, sets[j])), (max_bits, j)
    finally:
        pb.close()


def test_prepared_cut_window_count_equals_plain(ctx, orc):
    """2^16 + 1 bases (i + 1) * 3 G with the special ones: prepared == the plain form of the same call, and the uniform set == one scalar multiplication"""
    cv = Bn254Curve(orc)
    n = (1 << 16) + 1
    rng = np.random.default_rng(0x5B4)
    pts = multiples_of_3g(cv, n).copy()
    mult = [3 * (i + 1) for i in range(n)]
    special_bases(cv, pts)
    mult[2], mult[3], mult[5] = 0, mult[0], -mult[4]
    pb = PreparedBases(ctx, pts)
    try:
        for max_bits in (40, 256):
            sets = boundary_sets(rng, n, max_bits)
            sets[:, 5] = sets[:, 4]
            out, plan = msm_bits(ctx, None, sets, max_bits, bases=pb)
            c = mp.prepared_c(17)
            assert c == 16 and plan == mp.plan_of(n, max_bits, True) == [c, 4 if max_bits == 40 else 17, 0, 1]
            plain, pplan = msm_bits(ctx, pts, sets, max_bits)
            assert pplan == mp.plan_of(n, max_bits) == [15, 4 if max_bits == 40 else 18, 0, 1]
            assert np.array_equal(out, plain), max_bits
            k = int(sum(int(v) * m for v, m in zip(to_obj(sets[1]), mult)) % pm.R)
            assert cv._unpt(out[1]) == cv.mul(pm.G, k), max_bits
    finally:
        pb.close()


@pytest.mark.parametrize("n,max_bits,prepared", [(300, 20, False), (1 << 16, 40, False), (1 << 16, 12, False), (1 << 16, 40, True)])
def test_overflow_is_an_error_never_a_wrong_point(ctx, orc, n, max_bits, prepared):
    cv = Bn254Curve(orc)
    rng = np.random.default_rng(0x5B5 + n + max_bits)
    pts = multiples_of_3g(cv, n)
    weights = [3 * (i + 1) for i in range(n)]
    lg = mp.lg_of(n)
    c, wps, one_window, _ = mp.plan(lg, max_bits, prepared)
    bad = mp.unrepresentable(lg, max_bits, prepared)
    assert bad == (1 << max_bits if one_window else 1 << (wps * c)) and one_window == int((n, max_bits) == (1 << 16, 12))
    fits = mp.largest(c, wps)                                # every digit at its largest
    assert mp.signed_digits(bad, c, wps)[1] and not mp.signed_digits(fits, c, wps)[1] and (1 << max_bits) - 1 <= fits < bad
    pb = PreparedBases(ctx, pts) if prepared else None
    try:
        good = rand_below(rng, n, max_bits)
        vals = to_obj(good)

        def point(values, skip=None):
            return cv.mul(pm.G, int(sum(int(v) * w for i, (v, w) in enumerate(zip(values, weights)) if i != skip) % pm.R))

        want = point(vals)
        out, plan = msm_bits(ctx, pts, good, max_bits, bases=pb)
        assert plan == [c, wps, one_window, int(c > 11)] and cv._unpt(out[0]) == want
        for idx in (0, n // 2, n - 1):
            sc = good.copy()
            sc[idx] = limbs_of(bad)
            assert msm_bits(ctx, pts, sc, max_bits, bases=pb, rc_only=True) == E_INVALID_ARG, idx
            assert b"max_bits" in ctx.lib.gl355_last_error(ctx.h)
            # the call after an error on the same context is right again
            out, _ = msm_bits(ctx, pts, good, max_bits, bases=pb)
            assert cv._unpt(out[0]) == want, idx
            # the largest scalar the digits hold, in the same place: accepted, and the right sum
            sc[idx] = limbs_of(fits)
            v2 = vals.copy()
            v2[idx] = fits
            out, _ = msm_bits(ctx, pts, sc, max_bits, bases=pb)
            assert cv._unpt(out[0]) == point(v2), idx
            if not prepared:                                 # the same scalar on an identity base does not count
                p2 = pts.copy()
                p2[idx] = 0
                sc[idx] = limbs_of(bad)
                out, _ = msm_bits(ctx, p2, sc, max_bits)
                assert cv._unpt(out[0]) == point(vals, skip=idx), idx
        if prepared:                                         # ... nor in a table, whose identity is all zeros too
            p2 = pts.copy()
            p2[n // 2] = 0
            pb2 = PreparedBases(ctx, p2)
            try:
                sc = good.copy()
                sc[n // 2] = limbs_of(bad)
                out, _ = msm_bits(ctx, None, sc, max_bits, bases=pb2)
                assert cv._unpt(out[0]) == point(vals, skip=n // 2)
            finally:
                pb2.close()
    finally:
        if pb is not None:
            pb.close()


@pytest.mark.parametrize("n", [300, 1 << 16])
def test_full_width_scalars_never_overflow(ctx, orc, n):
    """the public entry (max_bits = 256) with every scalar 2^256 - 1: ((2^256 - 1) mod r) * sum P_i"""
    cv = Bn254Curve(orc)
    pts = multiples_of_3g(cv, n)
    sc = np.full((n, 4), U64, dtype=np.uint64)
    want = cv.mul(pm.G, ((1 << 256) - 1) % pm.R * (3 * n * (n + 1) // 2) % pm.R)
    assert cv._unpt(gpu_msm(ctx, pts, sc)) == want
    out, plan = msm_bits(ctx, pts, sc, 256)
    assert plan == mp.plan_of(n, 256) and plan[0] * plan[1] > 256 and cv._unpt(out[0]) == want


# ---- commit_columns ------------------------------------------------------------------------------------------------------------------------
COLUMN_BITS = [0, 1, 1, 11, 12, 16, 13, 19, 20, 21, 39, 40, 41, 60, 64, 65, 200] + [253] * 6 + [16] * 17
TAIL_ROWS = 6
_columns = {}


def layout_columns(k):
    """40 columns of the bit lengths above (each holds one value with its top bit set, in the body; the rest uniform below it) and, for the rows a tail
    covers, full-width values below r for EVERY column: (columns [40][n][4], blinding [40][6][4])"""
    if k not in _columns:
        n = 1 << k
        rng = np.random.default_rng(0x5B6 + k)
        cols = np.stack([rand_below(rng, n, max(0, b - 1)) for b in COLUMN_BITS])
        for j, b in enumerate(COLUMN_BITS):
            if b:
                row = int(rng.integers(0, n - TAIL_ROWS))
                cols[j, row, (b - 1) // 64] |= np.uint64(1 << ((b - 1) % 64))
        blind = np.stack([rand_below(rng, TAIL_ROWS, 253) for _ in COLUMN_BITS])
        blind[:, :, 3] |= np.uint64(1 << 59)                 # 252 bits at least, below 2^253 < r
        cols.setflags(write=False)
        blind.setflags(write=False)
        _columns[k] = (cols, blind)
    return _columns[k]


def columns_under(k, tail):
    cols, blind = layout_columns(k)
    n = 1 << k
    if tail >= n:
        return cols
    c = cols.copy()
    c[:, tail:] = blind[:, TAIL_ROWS - (n - tail):]
    return c


def pk_commit(ctx, prover, which, cols, tail):
    out = np.full((cols.shape[0], 8), 0xAA, dtype=np.uint64)
    cols = np.ascontiguousarray(cols)
    ctx.check(ctx.lib.gl355_plonk_pk_commit_columns(prover.h, which, cols.ctypes.data, cols.shape[0], tail, out.ctypes.data))
    return out


_k12_body = {}


def k12_reference(cv, which, bases, tail):
    """the oracle's MSM per column: rows below n - 6 once per base set, the last six rows under each tail added to it"""
    cols, _ = layout_columns(12)
    n = 1 << 12
    if which not in _k12_body:
        _k12_body[which] = [cv._unpt(cv.msm_arrays(bases[:n - TAIL_ROWS], cols[j, :n - TAIL_ROWS])) for j in range(cols.shape[0])]
    under = columns_under(12, tail)
    return [cv.add(_k12_body[which][j], cv._unpt(cv.msm_arrays(bases[n - TAIL_ROWS:], under[j, n - TAIL_ROWS:]))) for j in range(cols.shape[0])]


@pytest.mark.parametrize("k,tables", [(12, 0), (12, 1), (16, 1)])
def test_commit_columns_vs_references(ctx, orc, k, tables, monkeypatch):
    """the prover's commit_columns on 40 columns whose lengths sit on its class boundaries, over g and g_lagrange, with no tail, an empty one, one row and
    six rows of full-width values.  k = 12 without and with the key's prepared tables against the oracle; k = 16 with GL355_PLONK_MSM_TABLES=1 (tables of
    2^16 points: 16-bit windows; every column of more than 20 bits runs on them) against gl355_kzg_commit per column, the full 256-bit path"""
    monkeypatch.setenv("GL355_PLONK_MSM_TABLES", str(tables))
    cv = Bn254Curve(orc)
    n = 1 << k
    # what the layout is for, by the restatement of the classing: mixed-length runs of short columns, class changes between neighbours, the six 253-bit
    # columns split five + one, the seventeen 16-bit columns split sixteen + one
    runs = mp.column_runs(COLUMN_BITS, n, bool(tables))
    assert [(r[1], r[2]) for r in runs] == [(9, 20), (3, 40), (2, 60), (2, 80), (1, 200), (5, 256), (1, 256), (16, 16), (1, 16)]
    assert [r[3] for r in runs] == [False] + [bool(tables)] * 6 + [False, False]
    cols, _ = layout_columns(k)
    ors = [int(np.bitwise_or.reduce(cols[j, :, 3])) << 192 | int(np.bitwise_or.reduce(cols[j, :, 2])) << 128 | int(np.bitwise_or.reduce(cols[j, :, 1])) << 64 |
           int(np.bitwise_or.reduce(cols[j, :, 0])) for j in range(40)]
    assert [v.bit_length() for v in ors] == COLUMN_BITS
    cs, cfg, w, prover = build(ctx, k, 9 if k == 12 else 12, n_perm=8)
    try:
        g, g_lagrange = h2.kzg_setup(ctx, k, TAU)            # the bases the key was built over (test_gpu_halo2.build)
        for which, bases in ((0, g), (1, g_lagrange)):
            for tail in (U64, n, n - 1, n - TAIL_ROWS):
                under = columns_under(k, tail)
                got = pk_commit(ctx, prover, which, under, tail)
                if k == 12:
                    assert [cv._unpt(p) for p in got] == k12_reference(cv, which, bases, tail), (which, tail)
                else:
                    for j in range(40):
                        one = np.zeros(8, dtype=np.uint64)
                        ctx.check(ctx.lib.gl355_kzg_commit(ctx.h, bases.ctypes.data, np.ascontiguousarray(under[j]).ctypes.data, k, 0, one.ctypes.data))
                        assert np.array_equal(got[j], one), (which, tail, j)
        # the hook's argument errors
        small = np.ascontiguousarray(cols[:2])
        out = np.zeros((2, 8), dtype=np.uint64)
        f = ctx.lib.gl355_plonk_pk_commit_columns
        assert f(None, 0, small.ctypes.data, 2, U64, out.ctypes.data) == E_INVALID_ARG
        assert f(prover.h, 0, None, 2, U64, out.ctypes.data) == E_INVALID_ARG
        assert f(prover.h, 0, small.ctypes.data, 2, U64, None) == E_INVALID_ARG
        assert f(prover.h, 2, small.ctypes.data, 2, U64, out.ctypes.data) == E_INVALID_ARG
        assert f(prover.h, 1, small.ctypes.data, 2, n + 1, out.ctypes.data) == E_INVALID_ARG
        assert f(prover.h, 1, small.ctypes.data, 2, U64 - 1, out.ctypes.data) == E_INVALID_ARG
        assert f(prover.h, 1, small.ctypes.data, 0, U64, None) == E_INVALID_ARG and f(prover.h, 1, small.ctypes.data, 0, U64, out.ctypes.data) == 0
    finally:
        prover.close()
