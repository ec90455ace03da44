"""CPU: the FRI model of tests/fri_arity_model.py held on its own, for arity bits a = 1..4 on a random polynomial of degree 2^5, rate 1:
the fold against the oracle's arity-2 fold, the verifier step against the folded polynomial, and the model's tail against its own trees."""
import importlib

import numpy as np
import pytest

import fri_arity_model as fm
import pymodel as pm
from oracle_lib import P, rand_field

LOG_N, RATE_BITS = 5, 1


def poly(seed):
    return rand_field(np.random.default_rng(seed), 2 << LOG_N)


def ext_eval(coeffs, x):
    return pm.ext_poly_eval([fm.ext(c) for c in np.asarray(coeffs).reshape(-1, 2)], (x % P, 0))


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_fold_is_a_successive_arity_2_folds(orc, a):
    """out[k] = sum_j beta^j c[A k + j] equals a folds by 2 with beta, beta^2, beta^4, beta^8"""
    coeffs, beta = poly(0xA0 + a), rand_field(np.random.default_rng(0xB0 + a), 2)
    want, b = coeffs, fm.ext(beta)
    for _ in range(a):
        want = orc.fri_fold(want, np.array(b, dtype=np.uint64))
        b = fm.mul(b, b)
    got = fm.fold(coeffs, a, beta)
    assert got.size == (2 << LOG_N) >> a and np.array_equal(got, want)


@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_step_interpolates_the_folded_polynomial(orc, a):
    """for 6 sampled indices: the opened leaf's value at `within` is the polynomial at x, and the interpolated value is the folded
    polynomial at x^A"""
    coeffs, beta = poly(0xC0 + a), rand_field(np.random.default_rng(0xD0 + a), 2)
    lde_bits = LOG_N + RATE_BITS
    leaves = fm.layer_leaves(orc, orc.lde_ext(coeffs, RATE_BITS, 7), a)
    assert leaves.shape == ((1 << lde_bits) >> a, 2 << a)
    folded = fm.fold(coeffs, a, beta)
    omega = pm.root_of_unity(lde_bits)
    for idx in np.random.default_rng(0xE0 + a).integers(0, 1 << lde_bits, 6).tolist():
        x = 7 * pow(omega, pm.bitrev(idx, lde_bits), P) % P
        evals = [fm.ext(v) for v in leaves[idx >> a].reshape(-1, 2)]
        opened, nxt, coset, x_next = fm.step(evals, idx, x, a, beta)
        assert coset == idx >> a and x_next == pow(x, 1 << a, P)
        assert opened == ext_eval(coeffs, x), idx
        assert nxt == ext_eval(folded, x_next), idx


# cap_height, arities
TAILS = [(0, [1]), (0, [2]), (2, [3]), (0, [4]), (1, [3, 2]), (2, [1, 2, 1]), (1, [2, 2, 1])]


@pytest.mark.parametrize("cap_height,arities", TAILS)
def test_model_tail_opens_its_own_trees(orc, cap_height, arities):
    """the composition alone: the leaf a query opens in every layer verifies against that layer's cap with the oracle's own path, a
    neighbouring leaf does not, and the opened values chain through the verifier step down to the final polynomial"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    coeffs = poly(0xF0 + sum(arities))
    ch = plonk.Challenger()
    ch.observe(rand_field(np.random.default_rng(0x5F1), 11))
    betas_ch = plonk.Challenger()
    betas_ch.observe(rand_field(np.random.default_rng(0x5F1), 11))
    caps, final, w, idx, layers = fm.fri_tail(orc, ch, coeffs, RATE_BITS, cap_height, arities, 4, 3)
    assert final.size == 2 * ((1 << LOG_N) >> sum(arities))
    betas = []
    for cap in caps:
        betas_ch.observe(cap)
        betas.append(betas_ch.get_extension_challenge())
    lde_bits = LOG_N + RATE_BITS
    shape = fm.layer_shape(lde_bits, cap_height, arities)
    omega = pm.root_of_unity(lde_bits)
    for x_index in idx.tolist():
        x = 7 * pow(omega, pm.bitrev(x_index, lde_bits), P) % P
        cur, prev = x_index, ext_eval(coeffs, x)
        for l, (leaves, dig) in enumerate(layers):
            a = arities[l]
            i = cur >> a
            assert leaves.shape[1] == shape[l][0]
            sib = orc.merkle_prove(dig, leaves.shape[0], cap_height, i)
            assert sib.shape[0] == shape[l][1]
            assert orc.merkle_verify(leaves[i], i, sib, caps[l], cap_height)
            assert not orc.merkle_verify(leaves[i ^ 1], i, sib, caps[l], cap_height)
            opened, prev_next, cur, x = fm.step([fm.ext(v) for v in leaves[i].reshape(-1, 2)], cur, x, a, betas[l])
            assert opened == prev, (x_index, l)
            prev = prev_next
        assert ext_eval(final, x) == prev
