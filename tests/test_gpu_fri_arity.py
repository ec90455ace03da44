"""gl355_fri_prove with reduction arities above 2, word for word against the tail composed in tests/fri_arity_model.py from the
oracle's primitives and a host Challenger started from the same state: caps, final polynomial, PoW witness, indices, every opened
leaf, every path and the transcript's next squeezes (the pattern of tests/test_gpu_fri_prove.py: rate_bits = 3, 3 queries).  Then
the one-layer parity surface (gl355_fri_fold_arity, gl355_fri_layer_commit_arity_h) and the refusals."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fri_arity_model as fm
from oracle_lib import rand_field

pytestmark = pytest.mark.gpu

RATE_BITS, N_QUERIES = 3, 3
E_INVALID_ARG, E_UNSUPPORTED = -1, -5
HASH_POSEIDON, HASH_BN254_POSEIDON = 0, 1
# log_n, cap_height, arities, pow_bits, hasher
SHAPES = [(4, 0, [2], 0, 0),           # first hashed leaf, 8 words
          (5, 2, [3], 6, 0),           # 16-word leaves
          (6, 0, [4], 0, 0),           # 32-word leaves
          (6, 1, [3, 2], 8, 0),        # mixed, two final coefficients
          (5, 2, [1, 2, 1], 4, 0),     # unhashed and hashed leaves in one proof
          (3, 2, [3], 0, 0),           # sum of the arity bits = log_n: one coefficient
          (3, 3, [3], 0, 0),           # a layer exactly as wide as the cap: empty path
          (4, 0, [2], 0, 1)]           # Bn254PoseidonHash trees and transcript


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def started_challenger(plonk, seed, hasher=0):
    ch = plonk.Challenger(hasher)
    ch.observe(rand_field(np.random.default_rng(seed), 11))
    return ch


def fri_prove(ctx, ch, coeffs, log_n, cap_height, arities, pow_bits):
    """-> rc, caps, final, w, idx, evals [q][ev_total], sibs [q][sib_total / 4][4]"""
    shape = fm.layer_shape(log_n + RATE_BITS, cap_height, arities)
    ev_total, depth_total = sum(max(w, 0) for w, _ in shape), sum(max(d, 0) for _, d in shape)
    arity = np.array(arities, dtype=np.uint32)
    caps = np.zeros(max(1, len(arities) * (4 << cap_height)), dtype=np.uint64)
    final = np.zeros(max(2, 2 * ((1 << log_n) >> min(sum(arities), log_n))), dtype=np.uint64)
    w = C.c_uint64()
    idx = np.zeros(N_QUERIES, dtype=np.uint64)
    evals = np.zeros((N_QUERIES, max(1, ev_total)), dtype=np.uint64)
    sibs = np.zeros((N_QUERIES, max(1, depth_total), 4), dtype=np.uint64)
    rc = ctx.lib.gl355_fri_prove(ctx.h, ptr(coeffs), log_n, RATE_BITS, cap_height, ptr(arity), len(arities), pow_bits, N_QUERIES, C.byref(ch.c),
                                 ptr(caps), ptr(final), C.byref(w), ptr(idx), ptr(evals), ptr(sibs))
    return rc, caps, final, w.value, idx, evals, sibs


@pytest.mark.parametrize("log_n,cap_height,arities,pow_bits,hasher", SHAPES)
def test_fri_prove_equals_the_model_composition(ctx, orc, log_n, cap_height, arities, pow_bits, hasher):
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    coeffs = rand_field(np.random.default_rng(0x6F0 + log_n + sum(arities)), 2 << log_n)
    want_ch, ch = started_challenger(plonk, 0x6F1, hasher), started_challenger(plonk, 0x6F1, hasher)
    want_caps, want_final, want_w, want_idx, layers = fm.fri_tail(orc, want_ch, coeffs, RATE_BITS, cap_height, arities, pow_bits, N_QUERIES, hasher)
    rc, caps, final, w, idx, evals, sibs = fri_prove(ctx, ch, coeffs, log_n, cap_height, arities, pow_bits)
    ctx.check(rc)
    assert np.array_equal(caps[:want_caps.size], want_caps.reshape(-1))
    assert final.size == want_final.size == 2 * ((1 << log_n) >> sum(arities)) and np.array_equal(final, want_final)
    assert w == want_w
    assert np.array_equal(idx, want_idx)
    shape = fm.layer_shape(log_n + RATE_BITS, cap_height, arities)
    ev_off = np.concatenate([[0], np.cumsum([w_ for w_, _ in shape])]).astype(int)
    sib_off = np.concatenate([[0], np.cumsum([d for _, d in shape])]).astype(int)
    for q, x in enumerate(idx.tolist()):
        s = 0
        for l, (leaves, dig) in enumerate(layers):
            s += arities[l]
            i = x >> s
            got_leaf, got_sib = evals[q, ev_off[l]:ev_off[l + 1]], sibs[q, sib_off[l]:sib_off[l + 1]]
            assert np.array_equal(got_leaf, leaves[i]), (q, l)
            if hasher == HASH_POSEIDON and shape[l][1]:
                assert np.array_equal(got_sib, orc.merkle_prove(dig, leaves.shape[0], cap_height, i)), (q, l)
            assert orc.merkle_verify(got_leaf, i, got_sib, want_caps[l], cap_height, hasher), (q, l)
    # the transcript ends where the composition's does
    assert np.array_equal(ch.squeeze(3), want_ch.squeeze(3))


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_one_layer_fold_and_commit(ctx, orc, a):
    """gl355_fri_fold_arity and gl355_fri_layer_commit_arity_h at n = 64 against the model; a = 1 also against the existing entry points"""
    n, cap_height = 64, 1
    rng = np.random.default_rng(0x6E0 + a)
    coeffs, beta, values = rand_field(rng, 2 * n), rand_field(rng, 2), rand_field(rng, 2 * n)
    out = np.zeros(2 * (n >> a), dtype=np.uint64)
    ctx.check(ctx.lib.gl355_fri_fold_arity(ctx.h, ptr(coeffs), n, a, ptr(beta), ptr(out)))
    assert np.array_equal(out, fm.fold(coeffs, a, beta))
    want_leaves = fm.layer_leaves(orc, values, a)
    for hasher in (HASH_POSEIDON, HASH_BN254_POSEIDON):
        want_dig, want_cap = fm.merkle_build(orc, want_leaves, cap_height, hasher)
        leaves = np.zeros((n >> a, 2 << a), dtype=np.uint64)
        dig = np.zeros((2 * ((n >> a) - (1 << cap_height)), 4), dtype=np.uint64)
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        ctx.check(ctx.lib.gl355_fri_layer_commit_arity_h(ctx.h, hasher, ptr(values), n, a, cap_height, ptr(leaves), ptr(dig), ptr(cap)))
        assert np.array_equal(leaves, want_leaves) and np.array_equal(dig, want_dig) and np.array_equal(cap, want_cap), hasher
    if a == 1:
        assert np.array_equal(ctx.fri_fold(coeffs, beta).reshape(-1), out)
        tree = ctx.fri_layer_commit(values, cap_height)
        want_dig, want_cap = fm.merkle_build(orc, want_leaves, cap_height)
        assert np.array_equal(tree.leaves, want_leaves) and np.array_equal(tree.digests, want_dig) and np.array_equal(tree.cap, want_cap)


# log_n, cap_height, arities, code
REFUSALS = [(5, 0, [0], E_INVALID_ARG),            # an arity of 0 bits
            (5, 0, [2, 0], E_INVALID_ARG),
            (6, 0, [5], E_UNSUPPORTED),            # folds by 32
            (4, 0, [3, 2], E_INVALID_ARG),         # sum of the arity bits > log_n
            (5, 6, [3], E_INVALID_ARG)]            # layer of 2^5 leaves below a cap of 2^6


@pytest.mark.parametrize("log_n,cap_height,arities,code", REFUSALS)
def test_refusals_leave_the_context_usable(ctx, orc, log_n, cap_height, arities, code):
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    coeffs = rand_field(np.random.default_rng(0x6D0), 2 << log_n)
    rc = fri_prove(ctx, started_challenger(plonk, 0x6F1), coeffs, log_n, cap_height, arities, 0)[0]
    assert rc == code
    assert ctx.hash_no_pad(np.arange(1, 9, dtype=np.uint64))[0] == 0xD110AA6A46373941
    # the one-layer entry points refuse the same arities
    if len(arities) == 1 and arities[0] in (0, 5):
        out = np.zeros(2 << log_n, dtype=np.uint64)
        assert ctx.lib.gl355_fri_fold_arity(ctx.h, ptr(coeffs), 1 << log_n, arities[0], ptr(coeffs[:2].copy()), ptr(out)) == code
        assert ctx.lib.gl355_fri_layer_commit_arity_h(ctx.h, 0, ptr(coeffs), 1 << log_n, arities[0], 0, ptr(out), ptr(out), ptr(out)) == code
