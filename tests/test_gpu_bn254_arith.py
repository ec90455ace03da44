"""GPU: the BN254 device arithmetic at the edges of its lazy bounds, through the test hooks gl355_bn254_arith_batch / gl355_bn254_g1_chain,
against plain integers (tests/pymodel_bn254_limbs.py) and affine points (tests/pymodel_bn254_curve.py).  Every result is checked three ways:
the exact value or congruence, the range the source comments promise, and (29-bit form) the limb normalisation."""
import random

import numpy as np
import pytest

import pymodel_bn254_curve as pc
import pymodel_bn254_limbs as pl
from pymodel_bn254_limbs import Q, R256, R261

pytestmark = pytest.mark.gpu
R = pc.R
FIELDS = ("fr", "fq")


def recs8(vals):
    return np.array([pl.pack8(v) for v in vals], dtype=np.uint32)


def recs29(vals):
    return np.array([pl.pack29(v) if isinstance(v, int) else v for v in vals], dtype=np.uint32)


def redc(a, b, m):
    """CIOS with a full-width quotient: (a b + M m) / 2^256, M = -a b m^-1 mod 2^256 -- the exact 256-bit result of m_mul"""
    t = a * b
    return (t + (-t * pow(m, -1, R256) % R256) * m) >> 256


def pairs(core, full):
    a = [x for x in core for _ in full] + list(full)
    b = [y for _ in core for y in full] + list(full)
    return a, b


# ---- the 8 x 32-bit form (bn254_field.cuh) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS)
def test_mont_binary_ops_all_structured_pairs(ctx, f):
    m = pl.MOD[f]
    full = pl.edge8(f)
    core = [v for v in full if v in (0, 1, 2, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1) or v.bit_count() > 250 or v % 37 == 0][:64]
    core = sorted(set(core) | {0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m - 2})
    a, b = pairs(core, full)
    assert len(a) > 50000
    A, B = recs8(a), recs8(b)
    fq = pl.FQ if f == "fq" else 0
    got = pl.vals8(pl.arith(ctx, fq | pl.M_MUL, A, B))
    bad = [(x, y) for x, y, r in zip(a, b, got) if r != redc(x, y, m) or r >= 2 * m]
    assert not bad, "m_mul: %d wrong, first %r" % (len(bad), bad[:2])
    ge_m = sum(1 for r in got if r >= m)
    assert ge_m > 1000                                                   # the rare [m, 2m) results are exercised
    got = pl.vals8(pl.arith(ctx, fq | pl.M_ADD, A, B))
    want = [x + y - 2 * m if x + y >= 2 * m else x + y for x, y in zip(a, b)]
    eq_2m = sum(1 for x, y in zip(a, b) if x + y == 2 * m)
    assert eq_2m >= 4                                                    # sums of exactly 2m (the >= of the conditional subtraction)
    bad = [(x, y, r) for x, y, r, w in zip(a, b, got, want) if r != w or r >= 2 * m]
    assert not bad, "m_add: %d wrong, first %r" % (len(bad), bad[:2])
    got = pl.vals8(pl.arith(ctx, fq | pl.M_SUB, A, B))
    bad = [(x, y, r) for x, y, r in zip(a, b, got) if r >= 2 * m or (r - x + y) % m or r != (x - y if x >= y else x - y + 2 * m)]
    assert not bad, "m_sub: %d wrong, first %r" % (len(bad), bad[:2])
    got = pl.arith(ctx, fq | pl.M_EQ, A, B)
    assert (got[:, 1:] == 0).all()
    assert [int(r) for r in got[:, 0]] == [int((x - y) % m == 0) for x, y in zip(a, b)]


@pytest.mark.parametrize("f", FIELDS)
def test_mont_unary_ops(ctx, f):
    m = pl.MOD[f]
    vals = pl.edge8(f)
    A = recs8(vals)
    fq = pl.FQ if f == "fq" else 0
    got = pl.vals8(pl.arith(ctx, fq | pl.M_CANON, A))
    assert got == [v % m for v in vals]
    got = pl.arith(ctx, fq | pl.M_IS_ZERO, A)
    assert [int(r) for r in got[:, 0]] == [int(v % m == 0) for v in vals] and not got[:, 1:].any()
    got = pl.vals8(pl.arith(ctx, fq | pl.M_TO_INT, A))
    assert got == [v * pow(R256, -1, m) % m for v in vals]
    nz = [v for v in vals if v % m][:400] + [1, m - 1, m + 1, 2 * m - 1]
    got = pl.vals8(pl.arith(ctx, fq | pl.M_INV, recs8(nz)))
    bad = [(v, r) for v, r in zip(nz, got) if r >= 2 * m or (r * v - R256 * R256) % m]
    assert not bad, "m_inv: %r" % bad[:2]
    # m_from_int over its whole domain [0, 2^256): exactly the product of the reduced input by R^2
    ints = pl.from_int_edges(f)
    assert max(ints) == R256 - 1 and any(v >= 5 * m for v in ints)
    got = pl.vals8(pl.arith(ctx, fq | pl.M_FROM_INT, recs8(ints)))
    want = [redc(v % m, R256 * R256 % m, m) for v in ints]
    bad = [(v, r) for v, r, w in zip(ints, got, want) if r != w or r >= 2 * m]
    assert not bad, "m_from_int: %r" % bad[:2]


# ---- the 29-bit form (bn254_f29.cuh) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,f", [(pl.F29_MUL, "fq"), (pl.F29_MUL_FR, "fr")])
def test_f29_mul_at_its_operand_bounds(ctx, op, f):
    m = pl.MOD[f]
    normal = pl.f29_normal_values() + [k * m + d for k in range(13) for d in (-1, 0, 1) if k * m + d >= 0]
    normal = sorted(set(normal))
    firsts = [pl.pack29(v) for v in normal] + pl.lazy_first_operands()
    amax = max(max(x[:8]) for x in firsts)
    assert amax >= 0x5a000000 and amax < 2 ** 30.6                       # first operands reach past 2^30.4, within 2^30.6
    a = [x for x in firsts for _ in normal]
    b = [pl.pack29(y) for _ in firsts for y in normal]
    assert len(a) > 20000
    got = pl.arith(ctx, op, np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32))
    bad = [i for i in range(len(a)) if not pl.f29_mul_ok(a[i], b[i], got[i], f)]
    assert not bad, "f29_mul: %d wrong, first a=%r b=%r got=%r" % (len(bad), a[bad[0]], b[bad[0]], got[bad[0]].tolist())


@pytest.mark.parametrize("op", sorted(pl.F29_SUB_K))
def test_f29_sub_lends_enough(ctx, op):
    k = pl.F29_SUB_K[op]
    C = pl.lent(k)
    mins = [v for v in pl.f29_normal_values() if v < R256]
    subs = pl.subtrahends(k)
    a = [pl.pack29(x) for x in mins for _ in subs]
    b = [pl.pack29(y) for _ in mins for y in subs]
    got = pl.arith(ctx, op, np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32))
    top_short = 0
    for i in range(len(a)):
        want = [a[i][j] + C[j] - b[i][j] for j in range(9)]
        assert all(0 <= w <= pl.M32 for w in want[:8]), "a constant lent too little for %r" % (b[i],)
        if want[8] < 0:                                                  # outside f29_sub's stated condition: the top limb wraps
            top_short += 1
            assert got[i].tolist() == want[:8] + [want[8] & pl.M32]
            continue
        assert got[i].tolist() == want
        assert pl.val29(got[i]) == pl.val29(a[i]) + k * Q - pl.val29(b[i])          # the integer identity: no limb wrapped
    assert top_short > 0
    # a wrapped top limb is still the right value modulo 2^32, so the re-normalisation every caller applies gives the true sum
    normed = pl.vals29(pl.arith(ctx, pl.F29_ADD_NORM, got, np.zeros_like(got)))
    assert normed == [pl.val29(x) + k * Q - pl.val29(y) for x, y in zip(a, b)]


def test_f29_neg_add_norm(ctx):
    vals = [v for v in pl.f29_normal_values() if v <= Q]                 # the callers negate a table coordinate (< q)
    got = pl.arith(ctx, pl.F29_NEG_C2, recs29(vals))
    assert [pl.val29(r) for r in got] == [2 * Q - v for v in vals]
    big = pl.f29_normal_values()
    a = [x for x in big for _ in big]
    b = [y for _ in big for y in big]
    got = pl.arith(ctx, pl.F29_ADD_NORM, recs29(a), recs29(b))
    assert pl.vals29(got) == [x + y for x, y in zip(a, b)] and all(pl.is_norm29(r) for r in got)
    lazy = pl.lazy_first_operands()
    got = pl.arith(ctx, pl.F29_NORM, np.array(lazy, dtype=np.uint32))
    assert pl.vals29(got) == [pl.val29(x) for x in lazy] and all(pl.is_norm29(r) for r in got)


def test_f29_conversions_and_zero_test(ctx):
    ints = sorted(set(pl.edge8("fq") + pl.from_int_edges("fq")))
    A = recs8(ints)
    s = pl.arith(ctx, pl.F29_FROM_U256, A)
    assert [r.tolist() for r in s] == [pl.pack29(v) for v in ints]
    assert pl.vals8(pl.arith(ctx, pl.F29_TO_U256, s)) == ints                          # round trip
    r_form = [v for v in ints if v < 2 * Q]
    A = recs8(r_form)
    for op in (pl.F29_LIFT, pl.F29_LIFT_INL):
        got = pl.arith(ctx, op, A)
        bound = 2 if op == pl.F29_LIFT else pl.PRODUCT_BOUND                             # lift: an m_mul (< 2 q); lift_inl: a product
        bad = [(v, r.tolist()) for v, r in zip(r_form, got) if not pl.is_norm29(r) or not pl.below(pl.val29(r), bound) or (pl.val29(r) - 32 * v) % Q]
        assert not bad, (op, bad[:2])
        low = pl.vals8(pl.arith(ctx, pl.F29_LOWER, got))                               # and back: the same residue, < 1.3 q
        assert all(pl.below(x, pl.PRODUCT_BOUND) and (x - v) % Q == 0 for x, v in zip(low, r_form))
    vals = [v for v in pl.f29_normal_values() if v < R261]
    low = pl.vals8(pl.arith(ctx, pl.F29_LOWER, recs29(vals)))
    assert all(pl.below(x, pl.PRODUCT_BOUND) and (x * 32 - v) % Q == 0 for x, v in zip(low, vals))
    tf = pl.vals8(pl.arith(ctx, pl.F29_TABLE_FORM, A))
    assert tf == [v * 32 % Q for v in r_form]
    # f29_is_zero_mod: exact on its domain [0, 2 q) -- 0, q, and non-zero values up to the edge
    dom = sorted({0, Q, 1, Q - 1, Q + 1, 2 * Q - 1, 2 * Q - 2} | {v for v in pl.f29_normal_values() if v < 2 * Q})
    got = pl.arith(ctx, pl.F29_IS_ZERO_MOD, recs29(dom))
    assert [int(x) for x in got[:, 0]] == [int(v % Q == 0) for v in dom]


def test_hasher_fr_enter_leave(ctx):
    ints = pl.from_int_edges("fr") + pl.edge8("fr")[:200]
    e = pl.arith(ctx, pl.HASH_FR_ENTER, recs8(ints))
    assert all(pl.is_norm29(r) and (pl.val29(r) - v * R261) % R == 0 and pl.val29(r) < 2 * R for r, v in zip(e, ints))
    assert pl.vals8(pl.arith(ctx, pl.HASH_FR_LEAVE, e)) == [v % R for v in ints]
    # fr_leave's domain: values below 169 r (the partial rounds let a value grow to ~85 r)
    lazy = [k * R + d for k in (0, 1, 2, 85, 168) for d in (0, 1, R - 1)]
    got = pl.vals8(pl.arith(ctx, pl.HASH_FR_LEAVE, recs29(lazy)))
    assert got == [v * pow(R261, -1, R) % R for v in lazy]


def test_bad_op_is_an_error(ctx, gl):
    a = np.zeros((1, 9), dtype=np.uint32)
    for op in (-1, 9, 15, 25, 31, 50):
        with pytest.raises(gl.Gl355Error):
            pl.arith(ctx, op, a, a)


# ---- point chains ---------------------------------------------------------------------------------------------------------------------
def points(n, seed):
    rng = random.Random(seed)
    return [pc.mul(pc.G, rng.randrange(1, R)) for _ in range(n)]


def neg(p):
    return None if p is None else (p[0], (-p[1]) % Q)


def check_trace(tr, want, form, bounds, normal):
    """tr (n_steps, 40) against the affine points `want`; bounds[i]: per-coordinate bound (multiples of q) or None; normal: 29-bit limbs"""
    assert tr.shape[0] == len(want)
    rf = "r" if form == "r" else "29"
    for i, (rec, p) in enumerate(zip(tr, want)):
        assert rec[37] != 0xFFFFFFFF, i
        cs, ident, _ = pl.trace_coords(rec, rf)
        if p is None:
            assert ident == 1, "step %d: expected the identity" % i
            continue
        assert ident == 0, "step %d: unexpected identity" % i
        if form == "xyzz":
            got = pl.affine_of(cs[0], cs[1], (cs[2], cs[3]), "xyzz")
        else:
            got = pl.affine_of(cs[0], cs[1], cs[2], rf)
        assert got == p, "step %d: wrong point" % i
        if normal:
            for c in range(4 if form == "xyzz" else 3):
                assert pl.is_norm29(rec[9 * c:9 * c + 9]), "step %d coordinate %d: limbs not normalised" % (i, c)
        b = bounds[i]
        if b is not None:
            for c, k in enumerate(b):
                assert pl.below(cs[c], k), "step %d coordinate %d: %.3f q above the documented %.1f q" % (i, c, cs[c] / Q, k)


def bucket_steps_and_points(pool, idx_sign):
    acc, want = None, []
    for e in idx_sign:
        p = pool[e & 0x7FFFFFFF]
        acc = pc.add(acc, neg(p) if e >> 31 else p)
        want.append(acc)
    return want


BUCKET_FORMS = [(pl.CHAIN_XYZZ, "xyzz"), (pl.CHAIN_JAC29, "29"), (pl.CHAIN_JAC, "r")]


@pytest.mark.parametrize("form,kind", BUCKET_FORMS)
def test_bucket_accumulator_special_cases(ctx, form, kind):
    P, Qp, T = points(3, 7)
    pool = [P, Qp, pc.add(P, Qp), neg(pc.add(P, Qp)), T, pc.add(pc.add(P, Qp), pc.add(P, Qp))]
    ops = [pl.pack8(p[0]) + pl.pack8(p[1]) + [0] * 10 for p in pool]
    chains = [
        [0, 1, 2, 4],                      # P, Q, P+Q: the doubling branch with zz != 1, then an ordinary add
        [0, 1, 3, 4, 0],                   # P, Q, -(P+Q): the identity mid-chain, then adds after it
        [0, 1, 2 | pl.NEG, 4, 4 | pl.NEG],  # P + Q - (P+Q) by a negative digit: identity; T - T: identity
        [0 | pl.NEG, 1 | pl.NEG, 3, 5],    # -P, -Q, -(P+Q): doubling of a negated sum, then + 2(P+Q): identity
        [4, 4, 4, 4, 0],                   # T + T from a fresh accumulator (zz = 1), then doubling again
    ]
    w = max(len(c) for c in chains)
    steps = np.array([c + [4] * (w - len(c)) for c in chains], dtype=np.uint32)
    tr = pl.chain(ctx, form, ops, steps)
    for c in range(len(chains)):
        want = bucket_steps_and_points(pool, steps[c].tolist())
        bnd = [None if kind == "r" else (pl.BUCKET_BOUND if kind == "xyzz" else pl.BUCKET_BOUND[:3])] * w
        if kind == "r":
            bnd = [(2, 2, 2)] * w
        check_trace(tr[c], want, kind, bnd, kind != "r")


@pytest.mark.parametrize("form,kind", BUCKET_FORMS)
def test_bucket_accumulator_long_random_chains(ctx, form, kind):
    pool = points(48, 11)
    pool += [pc.add(pool[0], pool[1]), neg(pool[2])]
    ops = [pl.pack8(p[0]) + pl.pack8(p[1]) + [0] * 10 for p in pool]
    rng = np.random.default_rng(5 + form)
    n_chains, n_steps = 4, 10000
    steps = rng.integers(0, len(pool), (n_chains, n_steps), dtype=np.uint32) | (rng.integers(0, 2, (n_chains, n_steps), dtype=np.uint32) << 31)
    tr = pl.chain(ctx, form, ops, steps)
    for c in range(n_chains):
        want = bucket_steps_and_points(pool, steps[c].tolist())
        bnd = (2, 2, 2) if kind == "r" else (pl.BUCKET_BOUND if kind == "xyzz" else pl.BUCKET_BOUND[:3])
        check_trace(tr[c], want, kind, [bnd] * n_steps, kind != "r")


# ---- the reduction forms: jac29_add / jac29_double (lifted or raw), and j_add / j_madd / j_double -------------------------------------------
def red_operands(pts, kind, rng, edge=False):
    """operand records for the points: 'r' 8 x 32 R-form Jacobian with a random z and non-canonical representatives (+ q where < 2q);
    '29' raw 29-bit coordinates, at the 12 q edge when edge is set"""
    out = []
    for p in pts:
        if p is None:
            out.append(pl.operand_record(0, 0, 0, 1, "29" if kind == "29" else "r") if kind == "29" else pl.operand_record(R256 % Q, R256 % Q, 0))
            continue
        z = rng.randrange(1, Q)
        x, y, zz = pl.jac_of(p, z, "r" if kind == "r" else "29")
        if kind == "r":
            x, y, zz = (v + Q if v + Q < 2 * Q and rng.random() < 0.5 else v for v in (x, y, zz))
            out.append(pl.operand_record(x, y, zz))
        else:
            k = 11 if edge else rng.randrange(0, 12)
            x, y, zz = (v + k * Q if v + k * Q < 12 * Q else v for v in (x, y, zz))
            out.append(pl.operand_record(x, y, zz, 0, "29"))
    return out


def red_model(pts, steps):
    """affine values and branch of each step of the two-accumulator chain: (point written, 'add' | 'dbl' | 'copy' | 'id')"""
    A = B = None
    want, kinds = [], []
    for s in steps:
        kind, k = s >> 28, s & 0x0FFFFFFF
        if kind in (pl.STEP_ADD, pl.STEP_MADD):
            o = pts[k]
            br = "copy" if A is None or o is None else ("dbl" if A == o else ("id" if A == neg(o) else "add"))
            A = pc.add(A, o)
            want.append(A)
        elif kind == pl.STEP_DOUBLE:
            br = "dbl"
            A = pc.add(A, A)
            want.append(A)
        elif kind == pl.STEP_SELF:
            br = "dbl"
            A = pc.add(A, A)
            want.append(A)
        else:
            br = "copy" if B is None or A is None else ("dbl" if A == B else ("id" if A == neg(B) else "add"))
            B = pc.add(B, A)
            want.append(B)
        kinds.append(br)
    return want, kinds


def red_chains(n_pts):
    ADD, DBL, ACC, SELF = (lambda k=0, t=t: pl.step(t, k) for t in (pl.STEP_ADD, pl.STEP_DOUBLE, pl.STEP_ACC, pl.STEP_SELF))
    level = []
    for u in range(8, -1, -1):                               # msm_level_kernel: run += S_u; if u: acc += run
        level.append(ADD(u % n_pts))
        if u:
            level.append(ACC())
    return [
        level,
        [ADD(0), ACC(), ACC(), ADD(1), ACC(), ACC()],        # acc == run: the doubling branch of jac29_add
        [ADD(n_pts - 1), ACC(), ADD(0), ACC(), ACC()],      # an empty item (the identity) first, as an empty bucket gives
        [ADD(0)] + [DBL()] * 300,                            # the reduction's `shift` loop: >= 256 doublings in a row
        [ADD(0), ADD(1), ADD(2), SELF(), ADD(3), ADD(4)],    # P, Q, -(P + Q): the identity mid-chain, adds after it
        [ADD(5), ADD(6), ADD(7), DBL(), ACC(), ADD(8), SELF(), ACC()],
    ]


def run_red(ctx, form, kind, edge):
    rng = random.Random(21 + form + edge)
    P, Qp = points(2, 3)
    pts = [P, Qp, neg(pc.add(P, Qp))] + points(6, 13 + form) + [None]
    ops = red_operands(pts, "29" if kind == "29" else "r", rng, edge)
    if edge:
        for o in ops[:-1]:
            v = [pl.val29(o[9 * c:9 * c + 9]) for c in range(3)]
            assert all(pl.below(x, pl.RED_INPUT) for x in v) and min(v) > 11 * Q - 1
    chains = red_chains(len(pts))
    w = max(len(c) for c in chains)
    steps = np.array([c + [pl.step(pl.STEP_ADD, 0)] * (w - len(c)) for c in chains], dtype=np.uint32)
    tr = pl.chain(ctx, form, ops, steps)
    for c in range(len(chains)):
        want, br = red_model(pts, steps[c].tolist())
        dbl = pl.RED_DBL_BOUND_LEVELS if kind == "lift" else pl.RED_DBL_BOUND         # lifted items: what the levels see
        if kind == "r":
            bnd = [(2, 2, 2)] * w
        else:
            bnd = [pl.RED_ADD_BOUND if b == "add" else dbl if b == "dbl" else (pl.RED_INPUT,) * 3 for b in br]
        check_trace(tr[c], want, "r" if kind == "r" else "29", bnd, kind != "r")


@pytest.mark.parametrize("form,kind,edge", [(pl.CHAIN_RED29_LIFT, "lift", False), (pl.CHAIN_RED29_RAW, "29", False),
                                            (pl.CHAIN_RED29_RAW, "29", True), (pl.CHAIN_J, "r", False)])
def test_reduction_formulas(ctx, form, kind, edge):
    run_red(ctx, form, kind, edge)


def test_j_madd_and_random_reduction_chain(ctx):
    rng = random.Random(99)
    pts = points(16, 17)
    ops = red_operands(pts, "r", rng)
    for i, p in enumerate(pts[:8]):                          # affine operands for j_madd: z = R mod q
        ops[i] = pl.operand_record(p[0] * R256 % Q, p[1] * R256 % Q, R256 % Q)
    kinds = [pl.STEP_ADD, pl.STEP_DOUBLE, pl.STEP_ACC, pl.STEP_SELF, pl.STEP_MADD]
    steps = []
    for c in range(4):
        s = [pl.step(pl.STEP_MADD, 0), pl.step(pl.STEP_MADD, 0), pl.step(pl.STEP_MADD, 1)]
        for _ in range(2000):
            k = rng.choice(kinds)
            s.append(pl.step(k, rng.randrange(8) if k == pl.STEP_MADD else rng.randrange(16)))
        steps.append(s)
    steps = np.array(steps, dtype=np.uint32)
    tr = pl.chain(ctx, pl.CHAIN_J, ops, steps)
    for c in range(4):
        want, _ = red_model(pts, steps[c].tolist())
        check_trace(tr[c], want, "r", [(2, 2, 2)] * steps.shape[1], False)
    rng2 = np.random.default_rng(3)
    for form, kind in ((pl.CHAIN_RED29_RAW, "29"), (pl.CHAIN_RED29_LIFT, "lift")):
        ops = red_operands(pts, "29" if kind == "29" else "r", rng)
        st = np.array([[pl.step(int(k), int(i)) for k, i in zip(rng2.integers(0, 4, 10000), rng2.integers(0, 16, 10000))] for _ in range(2)],
                      dtype=np.uint32)
        tr = pl.chain(ctx, form, ops, st)
        for c in range(2):
            want, br = red_model(pts, st[c].tolist())
            dbl = pl.RED_DBL_BOUND_LEVELS if kind == "lift" else pl.RED_DBL_BOUND
            bnd = [pl.RED_ADD_BOUND if b == "add" else dbl if b == "dbl" else (pl.RED_INPUT,) * 3 for b in br]
            check_trace(tr[c], want, "29", bnd, True)


def test_chain_refuses_bad_form_and_marks_bad_steps(ctx, gl):
    ops = np.zeros((1, pl.OPND_WORDS), dtype=np.uint32)
    with pytest.raises(gl.Gl355Error):
        pl.chain(ctx, 6, ops, np.zeros((1, 1), dtype=np.uint32))
    tr = pl.chain(ctx, pl.CHAIN_RED29_RAW, ops, np.array([[pl.step(pl.STEP_ADD, 5), pl.step(7, 0)]], dtype=np.uint32))
    assert (tr[0, :, 37] == 0xFFFFFFFF).all()
