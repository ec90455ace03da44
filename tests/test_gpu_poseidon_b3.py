"""The partial rounds in blocks of three (csrc/poseidon.cuh psd_partial_rounds_b3) on the device: the rounds alone on raw words through the test hook
(GL355_GL_PARTIAL_ROUNDS of gl355_gl_arith_batch) against the Python model of rounds 4 .. 25, and every kernel of merkle.hip that runs the one-lane
permutation -- the permutation entry point, the leaf hasher, the tree levels, the grinder -- against the oracle's naive permutation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_tables as gpt  # noqa: E402

pytestmark = pytest.mark.gpu

P = gpt.P
PARTIAL_ROUNDS = 13         # GL355_GL_PARTIAL_ROUNDS
LANES = 65                  # one full wave and one lane of the next


def edge_rows():
    """all words 2^64 - 1 (both halves of every term at their maximum), p - 1, 2^32 - 1, 2^32 (low halves zero), zero; then a lone p - 1 at word j"""
    rows = [[(1 << 64) - 1] * 12, [P - 1] * 12, [(1 << 32) - 1] * 12, [1 << 32] * 12, [0] * 12]
    rows += [[P - 1 if i == j else 0 for i in range(12)] for j in range(12)]
    return rows


def states(seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 64, (LANES, 12), dtype=np.uint64)
    e = np.array(edge_rows(), dtype=np.uint64)
    s[:len(e)] = e
    return s


def model_rounds_4_to_25(state, rc, m):
    """the state entering round 4 (constants added) -> the state entering round 26 (constants added), mod p"""
    s = [int(v) % P for v in state]
    for r in range(gpt.HALF_F, gpt.HALF_F + gpt.R_P):
        s[0] = pow(s[0], 7, P)
        s = [(v + c) % P for v, c in zip(gpt.mat_vec(m, s), rc[r + 1])]
    return s


def test_hook_equals_the_model_of_rounds_4_to_25(ctx):
    rc, m = gpt.load_rc(), gpt.mds_matrix()
    s = states(0xB3)
    want = np.array([model_rounds_4_to_25(row, rc, m) for row in s.tolist()], dtype=np.uint64)
    got = ctx.gl_arith_batch(PARTIAL_ROUNDS, s).reshape(LANES, 12)
    assert np.array_equal(got % np.uint64(P), want), np.argwhere(got % np.uint64(P) != want)[:4]
    # one lane alone, and a count that is no multiple of twelve
    assert np.array_equal(ctx.gl_arith_batch(PARTIAL_ROUNDS, s[7]) % np.uint64(P), want[7])
    assert ctx.lib.gl355_gl_arith_batch(ctx.h, PARTIAL_ROUNDS, s.ctypes.data, None, got.ctypes.data, 13) == -1         # GL355_E_INVALID_ARG


def test_permutation_entry_point(ctx, orc):
    s = states(0xB4)
    assert np.array_equal(ctx.poseidon_permute(s), orc.permute(s))


@pytest.mark.parametrize("leaf_len", [8, 9, 139])
def test_hash_leaves(ctx, orc, leaf_len):
    rng = np.random.default_rng(0xB5 + leaf_len)
    leaves = rng.integers(0, P, (LANES, leaf_len), dtype=np.uint64)
    leaves[0] = P - 1
    leaves[1] = 0
    want = np.array([orc.hash_no_pad(row) for row in leaves], dtype=np.uint64)
    assert np.array_equal(ctx.hash_leaves(leaves), want)


def test_tree(gl, ctx, orc):
    leaves = np.random.default_rng(0xB6).integers(0, P, (1 << 5, 9), dtype=np.uint64)
    tree = gl.MerkleTree(ctx, leaves, 1)
    dig, cap = orc.merkle_build(leaves, 1)
    assert np.array_equal(tree.digests, dig) and np.array_equal(tree.cap, cap)


def test_pow_grind(ctx, orc):
    st = np.random.default_rng(0xB7).integers(0, P, 12, dtype=np.uint64)
    assert ctx.pow_grind(st, 2, 6) == orc.pow_grind(st, 2, 6)
