"""The reduction tail of the device product (csrc/gl_field.cuh gl_dev_reduce_tail, the tail of gl_mul_multi), instruction by instruction with every
result truncated to its register width, against Python integers mod p.  z = (t_lo, v_lo) - w_hi leaves a borrow b2, y = z + w_lo EPS a carry c1, and
ONE correction d = c1 - b2 in {-1, 0, 1} is applied as y - d (a signed 64-bit multiply-add by -1) and d added into the high word.  The model also
states what the device code relies on: y + d EPS never leaves [0, 2^64).

The (c1, b2) classes are rare for random operands ((0, 1) and (1, 1) need lo < w_hi < 2^32), so the inputs are the family V of
tests/test_gpu_gl_arith.py in all ordered pairs, random pairs, and a steered set with a small `lo` under a large `w_hi`."""
import functools

import numpy as np

from test_gpu_gl_arith import family_v

P = (1 << 64) - (1 << 32) + 1
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
EPS = M32


def s32(x):
    return x - (1 << 32) if x & (1 << 31) else x


def tail_model(t_lo, v_lo, w_hi, w_lo):
    """-> (r, c1, b2, exact) : the seven instructions on 32-bit registers and 64-bit register pairs; `exact` = y + d EPS over the integers"""
    # v_sub_co_u32  x0, bw = t_lo - w_hi
    x0 = (t_lo - w_hi) & M32
    bw = int(t_lo < w_hi)
    # v_subb_co_u32 x1, bw = v_lo - 0 - bw
    x1 = (v_lo - bw) & M32
    b2 = int(v_lo < bw)
    # v_mad_u64_u32 y, c = w_lo * 0xFFFFFFFF + (x0, x1)
    y = w_lo * M32 + ((x1 << 32) | x0)
    c1 = y >> 64
    y &= M64
    # v_cndmask_b32 d = c ? 1 : 0 ;  v_subb_co_u32 d = d - 0 - b2   (32-bit, wraps to 0xFFFFFFFF for -1)
    d = (c1 - b2) & M32
    # v_mad_i64_i32 r = d * (-1) + y   (signed 32 x 32 -> 64, added mod 2^64)
    r = (s32(d) * -1 + y) & M64
    # v_add_u32 r_hi += d
    r = ((((r >> 32) + d) & M32) << 32) | (r & M32)
    return r, c1, b2, y + s32(d) * EPS


def product_model(a, b):
    """the four multiply-adds and the middle carry of gl_mul, then the tail -> (r, c1, b2, exact)"""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    t = a0 * b0
    u = a0 * b1 + (t >> 32)
    v = a1 * b0 + u
    ch = v >> 64
    v &= M64
    w = a1 * b1 + ((ch << 32) | (v >> 32))
    assert w <= M64
    return tail_model(t & M32, v & M32, w >> 32, w & M32)


@functools.lru_cache(maxsize=None)
def operand_pairs():
    v = family_v()
    rng = np.random.default_rng(0x7A11)
    pairs = [(x, y) for x in v for y in v]
    assert len(pairs) == 65025
    pairs += list(zip(rng.integers(0, 1 << 64, 4096, dtype=np.uint64).tolist(), rng.integers(0, 1 << 64, 4096, dtype=np.uint64).tolist()))
    # steered: a = 2^64 - i, b = 2^64 - j with small i, j: the product is 2^128 - (i + j) 2^64 + i j, so the low 64 bits (i j) are small under a
    # top word of 2^32 - 1 -- the borrow fires; w_lo = 2^32 - (i + j) is large or, for i + j past 2^32, small, which moves the carry
    small = [1, 2, 3, 5, 255, 65535, (1 << 31) - 1, 1 << 31, M32 - 1, M32]
    steer = [int(x) for x in rng.integers(1, 1 << 16, 24, dtype=np.uint64)] + small
    pairs += [((1 << 64) - i, (1 << 64) - j) for i in steer for j in steer]
    return tuple(pairs)


def test_tail_model_equals_the_product_mod_p_and_never_wraps_twice():
    classes = {(0, 0): 0, (1, 0): 0, (0, 1): 0, (1, 1): 0}
    for a, b in operand_pairs():
        r, c1, b2, exact = product_model(a, b)
        classes[(c1, b2)] += 1
        assert 0 <= exact < (1 << 64), (hex(a), hex(b), c1, b2)          # the single correction neither carries nor borrows
        assert r == exact, (hex(a), hex(b))                              # and the three instructions that apply it compute it
        assert r % P == a * b % P, (hex(a), hex(b))
    print("(c1, b2) classes over %d pairs: %s" % (len(operand_pairs()), classes))
    assert all(n >= 100 for n in classes.values()), classes


def test_tail_on_raw_words():
    """the tail alone (gl_reduce128's device path takes any 128-bit value): edge words in every position"""
    edge = (0, 1, 2, 1 << 31, M32 - 1, M32)
    for t_lo in edge:
        for v_lo in edge:
            for w_hi in edge:
                for w_lo in edge:
                    r, c1, b2, exact = tail_model(t_lo, v_lo, w_hi, w_lo)
                    assert 0 <= exact < (1 << 64) and r == exact
                    assert r % P == (((v_lo << 32) | t_lo) - w_hi + w_lo * EPS) % P
