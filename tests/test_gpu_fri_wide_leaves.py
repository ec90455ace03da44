"""GPU: the two leaf stages of the wide-arity FRI layer trees.  GL355_OPT_LEAF_LANES_LOG (option 7) picks, per layer, the 16-lanes-per-leaf
kernel that reads the value columns (fri_wide_leaves_units_kernel) or the copy + one-lane-per-leaf pair; the option never changes a
result.  Each shape runs gl355_fri_prove on a fresh context with the option at 0 (never) and at 31 (always) and is held word for word
against tests/fri_arity_model.fri_tail, computed once per shape: caps, final polynomial, PoW witness, indices, opened leaves, paths and the
transcript's next squeezes.  Shapes are the smallest where a wave of four leaf groups is partly filled, a layer is exactly as wide as
its cap, a leaf takes four permutations, two widths meet in one proof, and an arity-2 layer sits between them."""
import importlib

import numpy as np
import pytest

import fri_arity_cases as fc
import fri_arity_model as fm
from oracle_lib import rand_field
from test_gpu_fri_arity import HASH_BN254_POSEIDON, HASH_POSEIDON, N_QUERIES, RATE_BITS, fri_prove, started_challenger

pytestmark = pytest.mark.gpu

OPT_LEAF_LANES_LOG = 7
E_INVALID_ARG = -1
# log_n, cap_height, arities, hasher
SHAPES = [(4, 1, [3], HASH_POSEIDON),           # a layer of 16 leaves
          (3, 2, [3], HASH_POSEIDON),           # 8 leaves at the cap's 4
          (3, 3, [3], HASH_POSEIDON),           # exactly as wide as the cap: the digests are the cap
          (5, 0, [4], HASH_POSEIDON),           # four permutations per leaf
          (6, 1, [2, 4], HASH_POSEIDON),        # 128 leaves, then 8: two widths in one proof
          (7, 0, [1, 2, 3], HASH_POSEIDON),     # an arity-2 layer, untouched, in front of the two branches
          (4, 0, [2], HASH_BN254_POSEIDON)]     # the other hasher keeps the old path under both settings
_model = {}


def model(orc, plonk, log_n, cap_height, arities, hasher):
    key = (log_n, cap_height, str(arities), hasher)
    if key not in _model:
        coeffs = rand_field(np.random.default_rng(0x7F0 + log_n + sum(arities)), 2 << log_n)
        ch = started_challenger(plonk, 0x7F1, hasher)
        _model[key] = (coeffs, fm.fri_tail(orc, ch, coeffs, RATE_BITS, cap_height, arities, 0, N_QUERIES, hasher), ch.squeeze(3))
    return _model[key]


@pytest.mark.parametrize("setting", [0, 31])
@pytest.mark.parametrize("log_n,cap_height,arities,hasher", SHAPES)
def test_both_leaf_stages_give_the_model_tail(gl, orc, log_n, cap_height, arities, hasher, setting):
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    coeffs, (want_caps, want_final, want_w, want_idx, layers), want_next = model(orc, plonk, log_n, cap_height, arities, hasher)
    cx = gl.Context(0)
    try:
        cx.set_option(OPT_LEAF_LANES_LOG, setting)
        ch = started_challenger(plonk, 0x7F1, hasher)
        rc, caps, final, w, idx, evals, sibs = fri_prove(cx, ch, coeffs.copy(), log_n, cap_height, arities, 0)
        cx.check(rc)
    finally:
        cx.close()
    assert np.array_equal(caps[:want_caps.size], want_caps.reshape(-1))
    assert np.array_equal(final, want_final) and w == want_w and np.array_equal(idx, want_idx)
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
    assert np.array_equal(ch.squeeze(3), want_next)


def test_three_lock_step_units_are_the_same_bytes_under_both_settings(gl):
    """[3] on the degree-2^6 circuit: three units x a layer of 64 leaves in one launch"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=[3], zero_knowledge=False, cap_height=1)
    builders = [fc.small_circuit(cfg, 0x7E0 + u) for u in range(3)]
    wit = [b.sparse_witness() for b, _ in builders]
    rows, pis, seeds = np.stack([w[1] for w in wit]), np.stack([pi for _, pi in builders]), [0x7E5, 0x7E6, 0x7E7]
    out = {}
    for setting in (0, 31):
        cx = gl.Context(0)
        try:
            cx.set_option(OPT_LEAF_LANES_LOG, setting)
            data = builders[0][0].cb.build(cx, np.random.default_rng(0x7E9), min_degree_bits=6)
            assert data.fri_arity_bits == [3] and data.degree_bits == 6
            units = plonk.prove_sparse_units(cx, data, wit[0][0], rows, pis, seeds)
            singles = [plonk.prove_sparse(cx, data, wit[0][0], rows[u], pis[u], seeds[u], flat_only=True) for u in range(3)]
            for u in range(3):
                assert np.array_equal(units[u], singles[u]), (setting, u)
                data.verify(units[u], pis[u])
            out[setting] = units
        finally:
            cx.close()
    assert np.array_equal(out[0], out[31])


def test_the_option_refuses_values_outside_0_to_31(gl):
    cx = gl.Context(0)
    try:
        for bad in (-1, 32, 1 << 40):
            assert cx.lib.gl355_ctx_set_option(cx.h, OPT_LEAF_LANES_LOG, bad) == E_INVALID_ARG, bad
        for good in (0, 17, 31):
            assert cx.lib.gl355_ctx_set_option(cx.h, OPT_LEAF_LANES_LOG, good) == 0, good
    finally:
        cx.close()
