"""GPU: the resident Merkle tree (gl355_merkle_tree_*, api.DeviceMerkleTree): leaves replaced in place, paths read in batches.

Every case builds a tree on a fresh context, updates it, and compares `digests`, `cap`, `leaves` and `prove_batch` at {0, n - 1, an updated index, its
sibling, a duplicate} byte for byte with the CPU oracle's merkle_build / merkle_prove on the updated leaf array (merkle_update_model.expected).  Where
a case is about the path the update takes, the kernel mix is read from the profile (scopes are named after the kernels) and held against
merkle_update_model.kernel_mix, the plan restated in Python.  Leaves are canonical words: random ones, with the operand family of
tests/test_gpu_gl_arith.py mod p at words 0 and 2, as in tests/test_gpu_merkle_plan.py.

GL355_OPT_MERKLE_UPDATE_FULL_LOG only chooses between the dirty path and a whole rebuild, so the cases that are about the dirty path set it to 0 (a
rebuild only when every leaf changes) rather than depend on its default; test_option_* runs the default."""
import ctypes as C

import numpy as np
import pytest

import merkle_update_model as mm
from oracle_lib import Bn254Oracle, P
from test_gpu_gl_arith import family_v

E_INVALID_ARG = -1
gpu = pytest.mark.gpu


def make_leaves(n, leaf_len, seed):
    v = np.array([x % P for x in family_v()], dtype=np.uint64)
    leaves = np.random.default_rng(seed).integers(0, P, (n, leaf_len), dtype=np.uint64)
    i = np.arange(n)
    leaves[:, 0] = v[(i + seed) % len(v)]
    if leaf_len > 2:
        leaves[:, 2] = v[(7 * i + 3 + seed) % len(v)]
    return leaves


def probes(n, updated):
    u = int(updated)
    return [0, n - 1, u] + ([u ^ 1] if n > 1 else []) + [u]


def compare(gl, orc, hash_orc, t, want, cap_height, updated):
    """the resident tree `t` against want = (leaves, digests, cap) of the oracle"""
    leaves, dig, cap = want
    n = leaves.shape[0]
    assert np.array_equal(t.cap, cap)
    assert np.array_equal(t.digests, dig)
    assert np.array_equal(t.leaves, leaves)
    idx = probes(n, updated)
    got = t.prove_batch(idx)
    assert got.shape == (len(idx), (n.bit_length() - 1) - cap_height, 4)
    for q, i in enumerate(idx):
        assert np.array_equal(got[q], orc.merkle_prove(dig, n, cap_height, i)), i      # merkle_prove only indexes the digests: any hasher's
    assert np.array_equal(t.get_batch(idx), leaves[idx])
    host = t.to_host()
    assert np.array_equal(host.prove_host(idx[2]), got[2]) and np.array_equal(host.cap, cap)


def run_case(gl, orc, log_n, cap_height, leaf_len, updates, seed, lanes_log=None, full_log=0, hasher=0, want_mix=True):
    """build, apply every (indices, rows) of `updates` with one update call each, compare; -> the kernel mix of the last update"""
    n = 1 << log_n
    leaves = make_leaves(n, leaf_len, seed)
    hash_orc = Bn254Oracle(orc) if hasher else orc
    cx = gl.Context(0)
    try:
        if lanes_log is not None:
            cx.set_option(mm.OPT_MERKLE_LANES_LOG, lanes_log)
        if full_log is not None:
            cx.set_option(mm.OPT_MERKLE_UPDATE_FULL_LOG, full_log)
        t = gl.DeviceMerkleTree(cx, leaves, cap_height, hasher=hasher)
        cx.profile_enable()
        for indices, rows in updates:
            cx.profile_read()
            t.update(indices, rows)
            prof = cx.profile_read()
        cx.profile_enable(False)
        compare(gl, orc, hash_orc, t, mm.expected(hash_orc, leaves, updates, cap_height), cap_height, updates[-1][0][-1])
        t.close()
    finally:
        cx.close()
    got = mm.mix_of_profile(prof)
    if want_mix:
        want = mm.kernel_mix(log_n, cap_height, updates[-1][0], mm.LANES_LOG_DEFAULT if lanes_log is None else lanes_log,
                              mm.FULL_LOG_DEFAULT if full_log is None else full_log, hasher)
        print("2^%d leaves of %d words, cap height %d, %d pairs: %r" % (log_n, leaf_len, cap_height, len(updates[-1][0]), got))
        assert got == want
    return got


def random_update(n, k, leaf_len, seed, unique=True):
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, size=k, replace=False) if unique else rng.integers(0, n, k)
    return idx.astype(np.uint64), make_leaves(k, leaf_len, seed + 1)


@gpu
@pytest.mark.parametrize("log_n,cap_height,indices", [(0, 0, [0]), (1, 0, [1]), (4, 4, [3, 12])])
def test_degenerate_trees(gl, orc, log_n, cap_height, indices):
    """one leaf; two leaves, whose only node is the cap entry; all cap and no layer"""
    rows = make_leaves(len(indices), 4, 0xD0 + log_n)
    mix = run_case(gl, orc, log_n, cap_height, 4, [(np.array(indices, dtype=np.uint64), rows)], 0xD10 + log_n)
    assert "merkle_update_level_kernel" not in mix and "merkle_update_level_lanes_kernel" not in mix


@gpu
@pytest.mark.parametrize("k", [1, 2, 64])
def test_climb_only(gl, orc, k):
    """2^8 leaves: at most 64 dirty nodes in layer 1, so an update is the leaf kernel and one climb launch"""
    n = 256
    if k == 2:
        idx, rows = np.array([101, 100], dtype=np.uint64), make_leaves(2, 4, 0xC12)      # a sibling pair
    else:
        idx, rows = random_update(n, k, 4, 0xC10 + k)
    mix = run_case(gl, orc, 8, 0, 4, [(idx, rows)], 0xC1B)
    assert mix == {"merkle_update_leaves_kernel": 1, "merkle_update_climb_kernel": 1}


@gpu
@pytest.mark.parametrize("lanes_log,level_scope", [(None, "merkle_update_level_lanes_kernel"), (5, "merkle_update_level_kernel")])
def test_level_kernels_then_climb(gl, orc, lanes_log, level_scope):
    """2^10 leaves, 200 random ones change: the wide layers take the 16-lane kernel at the default MERKLE_LANES_LOG and the one-lane kernel at 5,
    the climb takes over at the first layer with at most 64 dirty nodes"""
    idx, rows = random_update(1024, 200, 4, 0x1E7)
    mix = run_case(gl, orc, 10, 0, 4, [(idx, rows)], 0x1E8, lanes_log=lanes_log)
    assert mix["merkle_update_climb_kernel"] == 1 and mix[level_scope] >= 2 and len(mix) == 3


@gpu
def test_cap_subtrees(gl, orc):
    """2^10 leaves under a cap of 8 entries, updates in subtrees 2 and 5 only: the digests and cap entries of the other six are compared too"""
    rng = np.random.default_rng(0xCA9)
    idx = np.concatenate([2 * 128 + rng.choice(128, 20, replace=False), 5 * 128 + rng.choice(128, 70, replace=False)]).astype(np.uint64)
    rng.shuffle(idx)
    run_case(gl, orc, 10, 3, 4, [(idx, make_leaves(idx.size, 4, 0xCAA))], 0xCAB)
    # and with more than 64 cap subtrees dirty there is no climb layer: every layer takes a level kernel (form 0: 128 subtrees)
    idx = (np.arange(100) * 8 + 3).astype(np.uint64)
    mix = run_case(gl, orc, 10, 7, 4, [(idx, make_leaves(idx.size, 4, 0xCAC))], 0xCAD)
    assert "merkle_update_climb_kernel" not in mix and mix["merkle_update_level_lanes_kernel"] == 3


@gpu
@pytest.mark.parametrize("leaf_len", [4, 5, 8, 9, 135])
def test_leaf_lengths(gl, orc, leaf_len):
    """a leaf of at most 4 words is its own digest; 5 and 8 words are one sponge chunk, 9 two, 135 seventeen"""
    idx = np.array([63, 0, 17, 16, 40], dtype=np.uint64)
    run_case(gl, orc, 6, 0, leaf_len, [(idx, make_leaves(5, leaf_len, 0x1E0 + leaf_len))], 0x1EA + leaf_len)


@gpu
def test_leaf_length_below_four_is_zero_padded(gl, orc):
    run_case(gl, orc, 5, 1, 3, [(np.array([9, 31], dtype=np.uint64), make_leaves(2, 3, 0x1E3))], 0x1E4)


@gpu
def test_repeated_index_keeps_its_last_leaf(gl, orc):
    rows = make_leaves(4, 4, 0x2E9)
    idx = np.array([77, 5, 77, 5], dtype=np.uint64)
    n = 256
    leaves = make_leaves(n, 4, 0x2EA)
    cx = gl.Context(0)
    try:
        t = gl.DeviceMerkleTree(cx, leaves, 0)
        t.update(idx, rows)
        assert np.array_equal(t.get(77), rows[2]) and np.array_equal(t.get(5), rows[3])
        compare(gl, orc, orc, t, mm.expected(orc, leaves, [(idx, rows)], 0), 0, 77)
        # the same bytes as the two last pairs alone
        want = mm.expected(orc, leaves, [(idx[2:], rows[2:])], 0)
        assert np.array_equal(t.digests, want[1]) and np.array_equal(t.cap, want[2])
    finally:
        cx.close()


@gpu
def test_second_update_restores_the_first(gl, orc):
    n = 1024
    leaves = make_leaves(n, 4, 0x5EC)
    dig, cap = orc.merkle_build(leaves, 2)
    idx, rows = random_update(n, 90, 4, 0x5ED)
    cx = gl.Context(0)
    try:
        cx.set_option(mm.OPT_MERKLE_UPDATE_FULL_LOG, 0)
        t = gl.DeviceMerkleTree(cx, leaves, 2)
        assert np.array_equal(t.digests, dig) and np.array_equal(t.cap, cap)
        t.update(idx, rows)
        assert not np.array_equal(t.cap, cap)
        compare(gl, orc, orc, t, mm.expected(orc, leaves, [(idx, rows)], 2), 2, idx[0])
        t.update(idx[::-1].copy(), leaves[idx[::-1]])
        compare(gl, orc, orc, t, (leaves, dig, cap), 2, idx[0])
    finally:
        cx.close()


@gpu
def test_option_chooses_the_path_and_never_the_bytes(gl, orc):
    """2^10 leaves.  One leaf under FULL_LOG = 31 is a whole rebuild; every leaf under FULL_LOG = 0 is one too (an update of at least n >> 0 = n
    leaves), so all leaves but one are updated under 0 as well, which is the dirty path at its widest; the default (4) rebuilds from 64 leaves
    on.  Every run gives the oracle's bytes, compared inside run_case."""
    n = 1024
    one = random_update(n, 1, 4, 0x0F1)
    every = random_update(n, n, 4, 0x0F2)
    but_one = (every[0][:-1].copy(), every[1][:-1].copy())
    assert run_case(gl, orc, 10, 0, 4, [one], 0x0F3, full_log=31)["merkle_top_kernel"] == 1
    assert run_case(gl, orc, 10, 0, 4, [one], 0x0F3, full_log=None) == {"merkle_update_leaves_kernel": 1, "merkle_update_climb_kernel": 1}
    assert run_case(gl, orc, 10, 0, 4, [every], 0x0F3, full_log=0)["merkle_top_kernel"] == 1
    assert run_case(gl, orc, 10, 0, 4, [every], 0x0F3, full_log=None)["merkle_top_kernel"] == 1
    assert run_case(gl, orc, 10, 0, 4, [but_one], 0x0F3, full_log=0)["merkle_update_climb_kernel"] == 1
    assert run_case(gl, orc, 10, 0, 4, [but_one], 0x0F3, full_log=None)["merkle_top_kernel"] == 1
    assert "merkle_top_kernel" not in run_case(gl, orc, 10, 0, 4, [random_update(n, 63, 4, 0x0F4)], 0x0F3, full_log=None)
    assert run_case(gl, orc, 10, 0, 4, [random_update(n, 64, 4, 0x0F5)], 0x0F3, full_log=None)["merkle_top_kernel"] == 1


@gpu
def test_option_refuses_values_outside_0_to_31(gl):
    cx = gl.Context(0)
    try:
        for bad in (-1, 32):
            assert cx.lib.gl355_ctx_set_option(cx.h, mm.OPT_MERKLE_UPDATE_FULL_LOG, bad) == E_INVALID_ARG, bad
        for good in (0, 31):
            assert cx.lib.gl355_ctx_set_option(cx.h, mm.OPT_MERKLE_UPDATE_FULL_LOG, good) == 0, good
    finally:
        cx.close()


@gpu
@pytest.mark.parametrize("cap_height", [0, 2])
def test_bn254_hasher(gl, orc, cap_height):
    """the second hasher has no 16-lane update form: every dirty layer takes its one-lane kernel"""
    idx, rows = random_update(64, 5, 4, 0xB25 + cap_height)
    mix = run_case(gl, orc, 6, cap_height, 4, [(idx, rows)], 0xB27, hasher=gl.HASH_BN254_POSEIDON)
    assert mix == {"bn254_merkle_update_leaves_kernel": 1, "bn254_merkle_update_level_kernel": 6 - cap_height}
    # a leaf long enough for the sponge
    run_case(gl, orc, 4, cap_height, 9, [random_update(16, 3, 9, 0xB29)], 0xB2A + cap_height, hasher=gl.HASH_BN254_POSEIDON)


@gpu
def test_errors_leave_the_tree_untouched(gl, orc):
    n = 64
    leaves = make_leaves(n, 4, 0xE44)
    dig, cap = orc.merkle_build(leaves, 1)
    cx = gl.Context(0)
    lib = cx.lib
    try:
        t = gl.DeviceMerkleTree(cx, leaves, 1)
        rows = make_leaves(3, 4, 0xE45)
        idx = np.array([5, n, 6], dtype=np.uint64)                # the second index is one past the end
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.gl355_merkle_tree_update(t.h, p(idx), 3, p(rows)) == E_INVALID_ARG
        with pytest.raises(gl.Gl355Error):
            t.update(idx, rows)
        compare(gl, orc, orc, t, (leaves, dig, cap), 1, 5)        # nothing was written, not even leaf 5
        out = np.zeros((3, 5, 4), dtype=np.uint64)
        assert lib.gl355_merkle_tree_prove_batch(t.h, p(idx), 3, p(out)) == E_INVALID_ARG and not out.any()
        assert lib.gl355_merkle_tree_leaves(t.h, p(idx), 3, p(out)) == E_INVALID_ARG and not out.any()
        # NULL arguments are codes, nothing aborts
        ok = np.array([5], dtype=np.uint64)
        assert lib.gl355_merkle_tree_update(None, p(ok), 1, p(rows)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_update(t.h, None, 1, p(rows)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_update(t.h, p(ok), 1, None) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_prove_batch(None, p(ok), 1, p(out)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_prove_batch(t.h, None, 1, p(out)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_prove_batch(t.h, p(ok), 1, None) == E_INVALID_ARG
        for fn in (lib.gl355_merkle_tree_cap, lib.gl355_merkle_tree_digests):
            assert fn(None, p(out)) == E_INVALID_ARG and fn(t.h, None) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_leaves(t.h, None, 0, None) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_info(None, None, None, None, None) == E_INVALID_ARG
        h = C.c_void_p()
        assert lib.gl355_merkle_tree_create(cx.h, 0, None, n, 4, 0, C.byref(h)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_create(cx.h, 0, p(leaves), n, 4, 0, None) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_create(None, 0, p(leaves), n, 4, 0, C.byref(h)) == E_INVALID_ARG
        assert lib.gl355_merkle_tree_create(cx.h, 2, p(leaves), n, 4, 0, C.byref(h)) == E_INVALID_ARG          # no such hasher
        assert lib.gl355_merkle_tree_create(cx.h, 0, p(leaves), n - 1, 4, 0, C.byref(h)) == E_INVALID_ARG      # not a power of two
        assert lib.gl355_merkle_tree_create(cx.h, 0, p(leaves), n, 4, 7, C.byref(h)) == E_INVALID_ARG          # cap above the leaves
        assert lib.gl355_merkle_tree_destroy(None) == 0
        # n_idx = 0 is a no-op, whatever the pointers
        assert lib.gl355_merkle_tree_update(t.h, None, 0, None) == 0
        assert lib.gl355_merkle_tree_prove_batch(t.h, None, 0, None) == 0
        t.update(np.zeros(0, dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
        compare(gl, orc, orc, t, (leaves, dig, cap), 1, 5)
        vals = (C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int32())
        assert lib.gl355_merkle_tree_info(t.h, *[C.byref(v) for v in vals]) == 0
        assert [v.value for v in vals] == [n, 4, 1, 0]
    finally:
        cx.close()
