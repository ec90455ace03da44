"""The Goldilocks product forms of gl_field.cuh / poseidon.cuh on raw words, through the test hook gl355_gl_arith_batch: gl_mul, gl_mul_multi<1..4>,
gl_mul_fill, gl_mul2_fill, gl_sqr, psd_sbox, psd_sbox4, psd_recombine, psd_recombine_multi<4>.  Each has its own inline-asm carry chain, and their three
conditional steps -- the carry-out of the middle sum, the borrow of `lo - w_hi` repaid with -EPS, the carry of `x + w_lo EPS` repaid with +EPS -- fire for
few random operands (the borrow for ~2^-32 of them), so the operands are structured: every ordered pair of the family V of
test_field_mul_structured_operands, plus random whole-range pairs, then the routines' own unreduced outputs as operands again.  Every comparison is
exact, against Python integers mod p.

The CPU tests here (not marked gpu) count, with a restatement of the 32-bit decomposition, how often each step fires in what the GPU tests send: the
model only counts events, it never produces an expected value."""
import ctypes as C
import functools

import numpy as np
import pytest

P = (1 << 64) - (1 << 32) + 1
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
EPS = M32
E_INVALID_ARG = -1
# GL355_GL_*
MUL, MULTI1, MULTI2, MULTI3, MULTI4, MUL_FILL, MUL2_FILL, SQR, SBOX, SBOX4, RECOMBINE, RECOMBINE_MULTI4 = range(12)
WIDTH = {MUL: 1, MULTI1: 1, MULTI2: 2, MULTI3: 3, MULTI4: 4, MUL_FILL: 1, MUL2_FILL: 2, SQR: 1, SBOX: 1, SBOX4: 4, RECOMBINE: 1, RECOMBINE_MULTI4: 4}
CIRC5 = (17, 15, 41, 16, 2)         # the MDS row entries of the fill forms' five fillers
HASH_KAT = 0xD110AA6A46373941       # hash_no_pad(1 .. 8)[0]

gpu = pytest.mark.gpu


def family_v():
    """the operands of test_field_mul_structured_operands: the edges and, for k < 64, 2^k, 2^k - 1, 2^k + 1 and 2^64 - 2^k"""
    vals = {0, 1, P - 1, P, P + 1, (1 << 64) - 1, 0xFFFFFFFF00000000, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFE00000001}
    for k in range(64):
        vals.update({(1 << k) % (1 << 64), ((1 << k) - 1) % (1 << 64), ((1 << k) + 1) % (1 << 64), ((1 << 64) - (1 << k)) % (1 << 64)})
    return sorted(vals)


def mul_events(a, b):
    """(middle carry, borrow, final carry) of the device product of two u64: the steps of gl_mul and its lock-step / filled forms"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    t = a0 * b0
    u = a0 * b1 + (t >> 32)
    v = a1 * b0 + u
    mid = v >> 64                                   # the carry-out of the middle sum: bit 32 of what enters w
    v &= M64
    w = a1 * b1 + ((mid << 32) | (v >> 32))
    lo = ((v & M32) << 32) | (t & M32)              # (t_lo, v_lo)
    borrow = lo < (w >> 32)
    x = (lo - (w >> 32) - (EPS if borrow else 0)) & M64
    final = x + (w & M32) * EPS > M64
    return bool(mid), borrow, final


@functools.lru_cache(maxsize=None)
def pair_records():
    """(a, b, events[n][3], want) of all ordered pairs of V and 4 096 random whole-range pairs"""
    v = np.array(family_v(), dtype=np.uint64)
    rng = np.random.default_rng(0x61A)
    a = np.concatenate([np.repeat(v, len(v)), rng.integers(0, 1 << 64, 4096, dtype=np.uint64)])
    b = np.concatenate([np.tile(v, len(v)), rng.integers(0, 1 << 64, 4096, dtype=np.uint64)])
    ev = np.array([mul_events(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=bool)
    want = np.array([x * y % P for x, y in zip(a.tolist(), b.tolist())], dtype=np.uint64)
    for x in (a, b, ev, want):
        x.setflags(write=False)
    return a, b, ev, want


def padded(x, width):
    """x with its first records repeated behind it up to a multiple of `width`"""
    extra = -len(x) % width
    return np.concatenate([x, x[:extra]]) if extra else x


def reduced(raw):
    return np.array([x % P for x in np.asarray(raw, dtype=np.uint64).tolist()], dtype=np.uint64)


def eq(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d records differ, first at %d: got %x want %x" % (what, len(bad), got.size, bad[0], int(got[bad[0]]), int(want[bad[0]])))


# ---- CPU: what the operands exercise ---------------------------------------------------------------------------------------------
def test_operand_family_fires_every_carry_step():
    v = family_v()
    assert len(v) == 255
    a, b, ev, _ = pair_records()
    n = len(v) ** 2
    assert len(a) == n + 4096
    mid, borrow, final = ev[:n, 0], ev[:n, 1], ev[:n, 2]
    counts = (int(mid.sum()), int(borrow.sum()), int(final.sum()), int((borrow & final).sum()))
    print("pairs of V: middle carry %d, borrow %d, final carry %d, borrow and final carry %d of %d" % (counts + (n,)))
    assert all(c >= 1000 for c in counts), counts
    sq = np.array([mul_events(x, x) for x in v], dtype=bool).sum(axis=0)
    print("squares of V: middle carry %d, borrow %d, final carry %d of %d" % (sq[0], sq[1], sq[2], len(v)))
    assert all(c >= 16 for c in sq), sq
    # the borrow as test_field_mul_structured_operands states it, on the whole product: the model agrees with it
    for x, y, e in zip(a[:n:97].tolist(), b[:n:97].tolist(), ev[:n:97]):
        assert e[1] == (((x * y) & M64) < ((x * y) >> 96))


@pytest.mark.parametrize("width", [2, 3, 4])
def test_every_position_of_a_wide_form_meets_every_step(width):
    """an N-wide form takes N consecutive records per lane, record i at position i % N; the list is sent rotated by j = 0 .. N - 1, and under each
    rotation every position sees each step at least 100 times"""
    _, _, ev, _ = pair_records()
    for j in range(width):
        e = padded(np.roll(ev, j, axis=0), width)
        for pos in range(width):
            c = e[pos::width].sum(axis=0)
            assert all(k >= 100 for k in c), (width, j, pos, c)


def composite_inputs():
    """V, V + p where that fits 64 bits, and 4 096 random words"""
    v = family_v()
    rng = np.random.default_rng(0x61B)
    return np.concatenate([np.array(v + [x + P for x in v if x + P <= M64], dtype=np.uint64), rng.integers(0, 1 << 64, 4096, dtype=np.uint64)])


def recombine_carries(al, ah):
    """(the carry of al1 + ah0 into the top word, the carry-out of x + top EPS) of psd_recombine"""
    s = (al >> 32) + (ah & M32)
    top = (ah >> 32) + (s >> 32)
    x = ((s & M32) << 32) | (al & M32)
    return s > M32, x + top * EPS > M64


@functools.lru_cache(maxsize=None)
def recombine_records():
    """(al, ah): a grid over both carries -- al1 and ah0 around the 2^32 crossing, small and large low words, top words 0, 1, 2, 2^29 - 1 and their
    neighbours up to the contract's edge ah1 = 2^32 - 2 -- and the two shapes the permutations produce: MDS rows (al, ah < 2^44) and block dot
    products (al, ah < 2^61)"""
    edge = (0, 1, 1 << 31, M32 - 1, M32)
    al, ah = [], []
    for al1 in edge:
        for ah0 in edge:
            for al0 in (0, 1, 2, 1 << 31, M32 - 2, M32 - 1, M32):
                for ah1 in (0, 1, 2, 3, (1 << 29) - 2, (1 << 29) - 1, M32 - 1):
                    al.append((al1 << 32) | al0)
                    ah.append((ah1 << 32) | ah0)
    rng = np.random.default_rng(0x61C)
    for bits in (44, 61):
        al += rng.integers(0, 1 << bits, 2048, dtype=np.uint64).tolist()
        ah += rng.integers(0, 1 << bits, 2048, dtype=np.uint64).tolist()
    assert all((y >> 32) + 1 < (1 << 32) for y in ah)          # the documented contract of psd_recombine
    return tuple(al), tuple(ah)


def test_recombine_operands_fire_both_carries():
    al, ah = recombine_records()
    c = np.array([recombine_carries(x, y) for x, y in zip(al, ah)], dtype=bool)
    print("recombine: %d records, carry into the top word %d, carry-out of top * EPS %d" % (len(al), c[:, 0].sum(), c[:, 1].sum()))
    assert c[:, 0].sum() >= 100 and c[:, 1].sum() >= 100
    for j in range(4):                      # and at every position of the four-wide form, under each rotation
        e = padded(np.roll(c, j, axis=0), 4)
        for pos in range(4):
            assert all(k >= 100 for k in e[pos::4].sum(axis=0)), (j, pos)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def fill_accumulators(a, b, width):
    """what the fill forms' five fillers leave in al / ah: per lane, from the lane's first record (0 at the other records of the lane)"""
    al, ah = b & np.uint64(M32), b >> np.uint64(32)
    with np.errstate(over="ignore"):
        for k, c in enumerate(CIRC5):
            x = a * np.uint64(k + 1) + b
            al = al + (x & np.uint64(M32)) * np.uint64(c)
            ah = ah + (x >> np.uint64(32)) * np.uint64(c)
    first = (np.arange(len(a)) % width) == 0
    return np.where(first, al, np.uint64(0)), np.where(first, ah, np.uint64(0))


def run_product(ctx, op, a, b, want, what):
    """one launch of a two-operand product form; -> the raw outputs"""
    w = WIDTH[op]
    pa, pb = padded(a, w), padded(b, w)
    got = ctx.gl_arith_batch(op, pa, pb)
    if op in (MUL_FILL, MUL2_FILL):
        got, al, ah = got
        wal, wah = fill_accumulators(pa, pb, w)
        eq(al, wal, what + ": low accumulator of the fillers")
        eq(ah, wah, what + ": high accumulator of the fillers")
    eq(reduced(got), padded(want, w), what)
    return got[:len(a)]


@gpu
@pytest.mark.parametrize("op", [MUL, MULTI1, MULTI2, MULTI3, MULTI4, MUL_FILL, MUL2_FILL])
def test_product_forms_on_structured_pairs(ctx, op):
    a, b, _, want = pair_records()
    raw = None
    for j in range(WIDTH[op]):          # record i at position (i + j) % N of its lane
        r = run_product(ctx, op, np.roll(a, j), np.roll(b, j), np.roll(want, j), "op %d rotated by %d" % (op, j))
        raw = r if raw is None else raw
    # second pass: the unreduced representatives the routine itself emits, as operands
    want2 = np.array([x * y % P for x, y in zip(raw.tolist(), b.tolist())], dtype=np.uint64)
    run_product(ctx, op, raw, b, want2, "op %d on its own outputs" % op)


@gpu
@pytest.mark.parametrize("op,power", [(SQR, 2), (SBOX, 7), (SBOX4, 7)])
def test_square_and_sbox(ctx, op, power):
    x = padded(composite_inputs(), WIDTH[op])
    raw = ctx.gl_arith_batch(op, x)
    eq(reduced(raw), np.array([pow(v, power, P) for v in x.tolist()], dtype=np.uint64), "op %d" % op)
    eq(reduced(ctx.gl_arith_batch(op, raw)), np.array([pow(v, power, P) for v in raw.tolist()], dtype=np.uint64), "op %d on its own outputs" % op)


@gpu
@pytest.mark.parametrize("op", [RECOMBINE, RECOMBINE_MULTI4])
def test_recombine(ctx, op):
    al, ah = recombine_records()
    want = np.array([(x + (y << 32)) % P for x, y in zip(al, ah)], dtype=np.uint64)
    al, ah = np.array(al, dtype=np.uint64), np.array(ah, dtype=np.uint64)
    for j in range(WIDTH[op]):
        w = WIDTH[op]
        got = ctx.gl_arith_batch(op, padded(np.roll(al, j), w), padded(np.roll(ah, j), w))
        eq(reduced(got), padded(np.roll(want, j), w), "op %d rotated by %d" % (op, j))


@gpu
def test_arguments(ctx):
    lib, h = ctx.lib, ctx.h
    a = np.arange(1, 13, dtype=np.uint64)
    out = np.zeros(36, dtype=np.uint64)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for op in (-1, 12, 1 << 20):
        assert lib.gl355_gl_arith_batch(h, op, pa, pa, po, 12) == E_INVALID_ARG, op
    for op, n in ((MULTI2, 3), (MULTI3, 4), (MULTI4, 6), (MUL2_FILL, 1), (SBOX4, 5), (RECOMBINE_MULTI4, 11)):
        assert lib.gl355_gl_arith_batch(h, op, pa, pa, po, n) == E_INVALID_ARG, (op, n)
    for op in range(12):
        assert lib.gl355_gl_arith_batch(h, op, None, pa, po, 12) == E_INVALID_ARG, op
        assert lib.gl355_gl_arith_batch(h, op, pa, pa, None, 12) == E_INVALID_ARG, op
        one_operand = op in (SQR, SBOX, SBOX4)
        assert lib.gl355_gl_arith_batch(h, op, pa, None, po, 12) == (0 if one_operand else E_INVALID_ARG), op
        assert lib.gl355_gl_arith_batch(h, op, None, None, None, 0) == 0, op          # nothing to do
    assert (out[12:] == 0).all()
    for form in (-1, 1, 2, 4):
        assert lib.gl355_poseidon_permute_lanes(h, form, pa, 1) == E_INVALID_ARG, form
    assert lib.gl355_poseidon_permute_lanes(h, 0, None, 1) == E_INVALID_ARG
    assert lib.gl355_poseidon_permute_lanes(h, 3, None, 0) == 0
    # the context stays usable
    assert ctx.hash_no_pad(np.arange(1, 9, dtype=np.uint64))[0] == HASH_KAT
