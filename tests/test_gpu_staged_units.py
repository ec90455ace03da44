"""The staged C entry points of DEEP, polynomial evaluation, FRI fold and query openings are B = 1 launches of the lock-step prover's
kernels (csrc/fri.hip).  These cases sit where that sharing can go wrong: more polynomial sources than the prover's four blocks,
challenges passed in their non-canonical spelling, the smallest folds, and openings of salted and unsalted batches."""
import ctypes as C

import numpy as np
import pytest

import fri_arity_model as fm
from oracle_lib import P, rand_field

pytestmark = pytest.mark.gpu


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def eq(a, b):
    assert np.array_equal(np.asarray(a, dtype=np.uint64).ravel(), np.asarray(b, dtype=np.uint64).ravel())


def fold(ctx, coeffs, a, beta):
    n = coeffs.size // 2
    out = np.zeros(2 * (n >> a), dtype=np.uint64)
    ctx.check(ctx.lib.gl355_fri_fold_arity(ctx.h, ptr(coeffs), n, a, ptr(np.ascontiguousarray(beta, dtype=np.uint64)), ptr(out)))
    return out


# n = 2^8: exactly one 256-coefficient DEEP block, every carry zero; n = 2^9: two blocks, the carry path
@pytest.mark.parametrize("log_n", [8, 9])
def test_more_sources_than_the_prover_has_blocks(gl, ctx, orc, log_n):
    rng = np.random.default_rng(0x5A0 + log_n)
    n = 1 << log_n
    cols = [rand_field(rng, (w, n)) for w in (3, 1, 2, 4, 1, 2)]
    pbs = [gl.PolynomialBatch.from_coeffs(ctx, c, 1, 0) for c in cols]
    # six batches, not in their order, (3, 1) named twice
    picks = [(3, 1), (0, 2), (5, 0), (1, 0), (3, 1), (4, 0), (2, 1), (0, 0), (3, 3)]
    refs = [(pbs[b], c) for b, c in picks]
    flat = np.stack([cols[b][c] for b, c in picks])
    alpha, zeta, zeta2 = rand_field(rng, 2), rand_field(rng, 2), rand_field(rng, 2)
    eq(gl.eval_polys(ctx, refs, zeta), orc.eval_polys_ext(flat, zeta))
    eq(gl.eval_polys(ctx, refs[2:3], zeta), orc.eval_polys_ext(flat[2:3], zeta))
    acc0 = np.zeros(2 * n, np.uint64)
    want1 = orc.deep_batch(flat, alpha, zeta, acc0)
    acc1 = gl.deep_batch(ctx, refs, alpha, zeta, acc0)
    eq(acc1, want1)
    # a second call accumulates on the non-zero acc of the first; then one polynomial alone
    want2 = orc.deep_batch(flat[4:7], alpha, zeta2, want1)
    eq(gl.deep_batch(ctx, refs[4:7], alpha, zeta2, acc1), want2)
    eq(gl.deep_batch(ctx, refs[2:3], alpha, zeta, want2), orc.deep_batch(flat[2:3], alpha, zeta, want2))
    for pb in pbs:
        pb.close()


def test_non_canonical_challenges(gl, ctx):
    """a word v < 2^32 - 1 and the word v + p name the same field element: byte-identical outputs for either spelling"""
    rng = np.random.default_rng(0x5B0)
    n = 1 << 9
    a = rand_field(rng, (3, n))
    pa = gl.PolynomialBatch.from_coeffs(ctx, a, 1, 0)
    refs = [(pa, 2), (pa, 0), (pa, 1)]
    small = lambda: rng.integers(0, (1 << 32) - 1, size=2, dtype=np.uint64)
    alpha, z, beta = small(), small(), small()
    up = lambda v: v + np.uint64(P)      # fits 64 bits: v + p < 2^64
    acc = rand_field(rng, 2 * n)
    eq(gl.eval_polys(ctx, refs, up(z)), gl.eval_polys(ctx, refs, z))
    want = gl.deep_batch(ctx, refs, alpha, z, acc)
    for al, zz in ((up(alpha), z), (alpha, up(z)), (up(alpha), up(z)), (np.array([alpha[0], alpha[1] + np.uint64(P)], np.uint64), z)):
        eq(gl.deep_batch(ctx, refs, al, zz, acc), want)
    coeffs = rand_field(rng, 2 * 64)
    for ab in (1, 2, 3, 4):
        eq(fold(ctx, coeffs, ab, up(beta)), fold(ctx, coeffs, ab, beta))
    pa.close()


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_fold_at_its_smallest(ctx, a):
    """n = 2^a: one output, the lane's input is the whole array; n = 2^(a+1): two"""
    rng = np.random.default_rng(0x5C0 + a)
    for n in (1 << a, 2 << a):
        coeffs, beta = rand_field(rng, 2 * n), rand_field(rng, 2)
        eq(fold(ctx, coeffs, a, beta), fm.fold(coeffs, a, beta))


@pytest.mark.parametrize("salted", [False, True])
@pytest.mark.parametrize("cap", [0, 2, 4])      # 4 = lde_bits: the path is empty
def test_open_batch_through_the_shared_kernel(gl, ctx, orc, salted, cap):
    rng = np.random.default_rng(0x5D0 + cap)
    log_n, rate_bits = 3, 1
    N = 1 << (log_n + rate_bits)
    pb = gl.PolynomialBatch.from_values(ctx, rand_field(rng, (3, 1 << log_n)), rate_bits, cap, salt=rand_field(rng, (4, N)) if salted else None)
    assert pb.leaf_len == (7 if salted else 3)
    idx = [0, N - 1, 5, 5]
    got = pb.open_batch(idx)
    assert len(got) == len(idx)
    for i, (leaf, sib) in zip(idx, got):
        l2, s2 = pb.open(i)
        assert leaf.shape == (pb.leaf_len,) and sib.shape == (log_n + rate_bits - cap, 4)
        eq(leaf, l2)
        eq(sib, s2)
        assert orc.merkle_verify(leaf, i, sib, pb.cap, cap)
    assert pb.open_batch([]) == []
    pb.close()
