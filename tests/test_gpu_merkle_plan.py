"""GPU: the Merkle launch plan under GL355_OPT_MERKLE_LANES_LOG (option 1).  The option steers every branch of merkle_build_above_leaves (merkle.hip):
how many levels go to merkle_top_kernel, the loop that shrinks the top for a forest of many subtrees, whether a level takes the 16-lane kernel or the
one-lane kernel, and whether there is a top kernel at all -- and "results never depend on it" (include/gl355.h).  Each case builds a tree on a fresh
context with the option set and the profile on, holds digests, cap and openings against the oracle, and reads the kernel mix that ran from the profile.

PLAN is a restatement of the launch code worked out on paper (launch_plan below), not a device's answer.  Leaves are 4 words, so a leaf is its own digest
and layer 1 -- in the top kernel where that starts at layer 1, otherwise in a level kernel -- permutes chosen words: the operand family of
tests/test_gpu_gl_arith.py mod p, interleaved with random words."""
import importlib

import numpy as np
import pytest

import fri_arity_cases as fc
from oracle_lib import P
from test_gpu_gl_arith import family_v

OPT_MERKLE_LANES_LOG = 1
E_INVALID_ARG = -1
gpu = pytest.mark.gpu

# (log_n, cap_height, lanes_log) -> (one-lane levels, 16-lane levels, (first layer, levels) of the top kernel or None)
PLAN = {
    # one subtree: form 3 of the 16-lane permutation, at most six levels in the top kernel
    (6, 0, 0): (5, 0, (6, 1)),
    (6, 0, 1): (4, 0, (5, 2)),
    (6, 0, 14): (0, 0, (1, 6)),
    (10, 0, 5): (4, 0, (5, 6)),
    (10, 0, 14): (0, 4, (5, 6)),
    (15, 0, 11): (3, 6, (10, 6)),
    (15, 0, 14): (0, 9, (10, 6)),
    # 64 subtrees: form 0, up to eight levels
    (14, 6, 5): (8, 0, None),
    (14, 6, 11): (2, 0, (3, 6)),
    (14, 6, 12): (1, 0, (2, 7)),
    (14, 6, 14): (0, 0, (1, 8)),            # the 128-node level of the top kernel straight from the chosen leaves
    (15, 6, 14): (0, 1, (2, 8)),
    # 256 subtrees
    (16, 8, 11): (4, 0, (5, 4)),
    (16, 8, 14): (1, 0, (2, 7)),            # the shrinking loop at the default setting
    (16, 8, 30): (0, 0, (1, 8)),
}


def launch_plan(log_n, cap_height, lanes_log):
    n, sub_bits, subtrees, lanes_max = 1 << log_n, log_n - cap_height, 1 << cap_height, 1 << lanes_log
    top_levels = min(6 if subtrees < 64 else 8, sub_bits)
    while top_levels > 1 and (n >> (sub_bits - top_levels + 1)) > lanes_max:
        top_levels -= 1
    top_from = sub_bits + 1
    if top_levels >= 1 and (n >> (sub_bits - top_levels + 1)) <= lanes_max:
        top_from = sub_bits - top_levels + 1
    level = lanes = 0
    for layer in range(1, sub_bits + 1):
        if layer == top_from:
            return level, lanes, (layer, top_levels)
        if (n >> layer) <= lanes_max:
            lanes += 1
        else:
            level += 1
    return level, lanes, None


def test_the_table_is_the_restated_launch_code():
    for (log_n, cap_height, lanes_log), want in PLAN.items():
        assert launch_plan(log_n, cap_height, lanes_log) == want, (log_n, cap_height, lanes_log)
    # between them the cases take every branch: no top kernel, a top that the loop shrank, a top cut by the subtree's height, both level kernels
    plans = list(PLAN.values())
    assert any(t is None for _, _, t in plans) and any(lv and ln for lv, ln, _ in plans)
    assert {t[1] for _, _, t in plans if t} >= {1, 2, 4, 6, 7, 8}


_trees = {}


def reference_tree(orc, log_n, cap_height):
    """(leaves, digests, cap, openings at 0, n - 1 and n / 2), once per shape"""
    key = (log_n, cap_height)
    if key not in _trees:
        n = 1 << log_n
        v = np.array([x % P for x in family_v()], dtype=np.uint64)
        leaves = np.random.default_rng(0x3D0 + log_n).integers(0, P, (n, 4), dtype=np.uint64)
        i = np.arange(n)
        leaves[:, 0] = v[i % len(v)]                      # chosen words at 0 and 2, random ones at 1 and 3
        leaves[:, 2] = v[(7 * i + 3) % len(v)]
        dig, cap = orc.merkle_build(leaves, cap_height)
        paths = {idx: orc.merkle_prove(dig, n, cap_height, idx) for idx in (0, n - 1, n // 2)}
        _trees[key] = (leaves, dig, cap, paths)
    return _trees[key]


@gpu
@pytest.mark.parametrize("log_n,cap_height,lanes_log", sorted(PLAN))
def test_tree_and_kernel_mix(gl, orc, log_n, cap_height, lanes_log):
    leaves, dig, cap, paths = reference_tree(orc, log_n, cap_height)
    n, subtrees = 1 << log_n, 1 << cap_height
    cx = gl.Context(0)
    try:
        cx.set_option(OPT_MERKLE_LANES_LOG, lanes_log)
        cx.profile_enable()
        t = gl.MerkleTree(cx, leaves, cap_height)
        prof = cx.profile_read()
        cx.profile_enable(False)
        assert np.array_equal(t.cap, cap)
        assert np.array_equal(t.digests, dig)
        for idx, want in paths.items():
            assert np.array_equal(t.prove(idx), want), idx
    finally:
        cx.close()
    level, lanes, top = PLAN[(log_n, cap_height, lanes_log)]
    got = tuple(prof.get(k, (0, 0.0, 0))[0] for k in ("merkle_level_kernel", "merkle_level_lanes_kernel", "merkle_top_kernel"))
    print("2^%d leaves, cap height %d, lanes_log %d: level %d, lanes %d, top %d (%d algorithmic bytes)" % (
        (log_n, cap_height, lanes_log) + got + (prof.get("merkle_top_kernel", (0, 0.0, 0))[2],)))
    assert got == (level, lanes, 1 if top else 0)
    if top:
        # the scope's algorithmic bytes give the layer the top kernel started from: 96 bytes per node of its levels
        first, levels = top
        assert levels == log_n - cap_height - first + 1
        assert prof["merkle_top_kernel"][2] == (2 * (n >> first) - subtrees) * 96


@gpu
def test_the_option_refuses_values_outside_0_to_30(gl):
    cx = gl.Context(0)
    try:
        for bad in (-1, 31):
            assert cx.lib.gl355_ctx_set_option(cx.h, OPT_MERKLE_LANES_LOG, bad) == E_INVALID_ARG, bad
        for good in (0, 30):
            assert cx.lib.gl355_ctx_set_option(cx.h, OPT_MERKLE_LANES_LOG, good) == 0, good
    finally:
        cx.close()


@gpu
def test_five_lock_step_units_are_the_same_bytes_under_every_setting(gl):
    """the lock-step circuit of test_three_lock_step_units_are_the_same_bytes_under_both_settings at cap height 4 and five units: a forest of 80 subtrees (not a
    power of two), form 0, with no 16-lane level at all, the top kernel alone, and everything between"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=[3], zero_knowledge=False, cap_height=4)
    builders = [fc.small_circuit(cfg, 0x7E0 + u) for u in range(5)]
    wit = [b.sparse_witness() for b, _ in builders]
    rows, pis, seeds = np.stack([w[1] for w in wit]), np.stack([pi for _, pi in builders]), [0x7E5 + u for u in range(5)]
    out = {}
    for setting in (0, 11, 14, 30):
        cx = gl.Context(0)
        try:
            cx.set_option(OPT_MERKLE_LANES_LOG, setting)
            data = builders[0][0].cb.build(cx, np.random.default_rng(0x7E9), min_degree_bits=6)
            assert data.fri_arity_bits == [3] and data.degree_bits == 6
            units = plonk.prove_sparse_units(cx, data, wit[0][0], rows, pis, seeds)
            singles = [plonk.prove_sparse(cx, data, wit[0][0], rows[u], pis[u], seeds[u], flat_only=True) for u in range(5)]
            for u in range(5):
                assert np.array_equal(units[u], singles[u]), (setting, u)
                data.verify(units[u], pis[u])
            out[setting] = units
        finally:
            cx.close()
    for setting in (11, 14, 30):
        assert np.array_equal(out[0], out[setting]), setting
