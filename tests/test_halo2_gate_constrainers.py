"""CPU: the 12 gate constrainers, eval_filtered_constraint and GoldilocksExtensionAlgebraChip (halo2_plonk_chips.py) against the formulas of
plonk_verifier.py, on the smallest parameters that run every loop twice, for a random vector and one built from the edge values of
halo2_fri_cases.EDGE.  Every recording: status clean, host replay equal to the recorder's eager columns, the mock model clean."""
import pytest

import halo2_verifier_cases as hv
import plonk_verifier as pv

hg = hv.hg
N_CONSTRAINTS = dict(noop=0, constant=2, public_input=4, base_sum=3, poseidon=123, arithmetic=2, arithmetic_extension=4, multiplication_extension=4,
                     poseidon_mds=24, random_access=2 * (2 + 2) + 1, reducing=4, reducing_extension=4)


@pytest.mark.parametrize("vector", [0, 1], ids=["random", "edge"])
@pytest.mark.parametrize("name", sorted(hv.GATES))
def test_gate_constraints_equal_the_model(name, vector):
    rec, cells, want = hv.gate_case(name, vector)
    assert len(cells) == len(want) == N_CONSTRAINTS[name]
    assert [hv.val(c) for c in cells] == want
    if vector == 0 and want:
        assert any(w != pv.E0 for w in want)                         # random wires satisfy no gate
    hv.accepted(rec)


@pytest.mark.parametrize("vector", [0, 1], ids=["random", "selects_gate_2"])
@pytest.mark.parametrize("num_selectors", [2, 1])
def test_filtered_constraints(num_selectors, vector):
    rec, got, want, cd, (consts, wires, pi_hash) = hv.filtered_case(num_selectors, vector)
    assert max(hi - lo for lo, hi in cd["groups"]) >= 3
    assert [hv.val(c) for c in got] == want and len(got) == cd["num_gate_constraints"]
    # the same sums through plonk_verifier.eval_vanishing_poly itself: without challenges its terms are the gate constraints alone
    alone = dict(cd, degree_bits=3, num_routed_wires=0, quotient_degree_factor=8, num_partial_products=0, k_is=[], num_challenges=0)
    op = dict(constants=consts, wires=wires, plonk_zs=[], plonk_zs_next=[], plonk_sigmas=[], partial_products=[])
    alphas = [3, hv.P - 2]
    assert pv.eval_vanishing_poly(alone, (5, 6), (7, 8), op, pi_hash, [], [], alphas) == [pv.reduce_with_powers(want, pv.base(a)) for a in alphas]
    # the UNUSED_SELECTOR factor is there exactly when there is more than one selector
    n_const = sum(1 for e in rec.entries if e[2] == hg.OP_CONST and e[4][0] == hv.hp.UNUSED_SELECTOR and not any(e[4][1:]))
    assert n_const == (1 if num_selectors > 1 else 0)
    if vector == 1:                                                  # selector 0 opens to 2: of its group only gate 2 passes its filter
        noop = hv.GATES["noop"]
        others_off = dict(cd, gates=[g if cd["selector_indices"][i] != 0 or i == 2 else noop for i, g in enumerate(cd["gates"])])
        assert hv.filtered_want(others_off, consts, wires, pi_hash) == want and any(w != pv.E0 for w in want)
    hv.accepted(rec)


def test_extension_algebra_chip():
    rec, out = hv.algebra_case()
    assert {name for name, _, _ in out} == {"mul_add", "mul", "sub", "scalar_mul_add", "scalar_mul", "convert", "inner_product", "zero"}
    for name, got, want in out:
        assert (hv.val(got[0]), hv.val(got[1])) == want, name
    hv.accepted(rec)
