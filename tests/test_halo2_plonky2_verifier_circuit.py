"""CPU: Plonky2VerifierCircuit (halo2_verifier_circuit.py) on the two real proofs of halo2_fri_cases (12 public inputs: two hasher
permutations; one hiding, one not) and on a third whose circuit uses all 12 gate kinds.  The instances are the public inputs; every challenge
equals the restated get_challenges; the vanishing polynomial at zeta equals plonk_verifier.eval_vanishing_poly; the host replay equals the
recorder and the mock model is clean.  Six one-word mutations are rejected, and all but the public input by the quotient identity itself."""
import numpy as np
import pytest

import halo2_verifier_cases as hv

hg, fc, K = hv.hg, hv.fc, hv.K
CASES = ["zk", "plain", "all_gates"]
MUTATIONS = ["wire_opening", "constant_opening", "zs_next_opening", "partial_product_opening", "quotient_opening", "public_input"]


@pytest.mark.parametrize("name", CASES)
def test_circuit_accepts_the_proof(name):
    c = hv.verifier_case(name)
    rec, circuit = c.rec, c.circuit
    print("%s: %d rows, k = %d, %d entries, %d levels" % (name, rec.rows_used, rec.k, len(rec.entries), len(rec.level_widths())))
    assert rec.k == K == 17 and rec.status() == (hg.NO_FAILURE, 0)
    assert rec.instance == [int(v) for v in c.pi] and len(rec.instance) == circuit.num_public_inputs
    advice, status = hg.synthesize_host(rec.tape(), rec.k, c.inputs)
    assert status == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert fc.mock_failures_fast(rec, advice) == []
    cells, want, acc = circuit.challenge_cells, c.challenges, c.accepted
    vals = lambda e: tuple(x.value for x in e)      # noqa: E731
    for key in ("betas", "gammas", "alphas"):
        assert list(vals(cells[key])) == [int(v) for v in acc[key]] and len(cells[key]) == c.cd["num_challenges"]
    assert vals(cells["zeta"]) == want["zeta"] == tuple(int(v) for v in acc["zeta"])
    assert vals(cells["fri_alpha"]) == want["fri_alpha"] and [vals(b) for b in cells["fri_betas"]] == want["fri_betas"]
    assert cells["pow_response"].value == want["pow_response"] and [x.value for x in cells["indices"]] == want["indices"]
    assert [vals(v) for v in circuit.vanishing_cells] == c.vanishing and len(c.vanishing) == c.cd["num_challenges"]
    assert len(circuit.identity_rows) == 4 * c.cd["num_challenges"] and len(circuit.round_rows) == c.cd["num_query_rounds"]
    assert circuit.round_rows[-1][1] == rec.rows_used


def test_the_third_circuit_uses_all_twelve_gates():
    c = hv.verifier_case("all_gates")
    assert sorted(int(g[0]) for g in c.cd["gates"]) == list(range(12))
    assert c.cd["num_selectors"] > 1 and max(hi - lo for lo, hi in c.cd["groups"]) >= 3
    assert len(c.pi) == 5                                            # one hasher permutation; the Semaphore proofs take two


def test_the_two_old_circuits_record_as_before():
    """FriVerifierCircuit shares its helpers with the new circuit: the same proof gives the tape halo2_fri_cases recorded, and the new
    circuit's tape differs from it (it is no subclass accident)"""
    c = fc.case(False)
    again = hv.vc.FriVerifierCircuit(c.cd).record(c.inputs)
    assert again.artifact().digest() == c.rec.artifact().digest()
    assert hv.verifier_case("plain").rec.artifact().digest() != c.rec.artifact().digest()


def test_vanishing_polynomial_alone_on_random_openings():
    rec, got, want, identity_rows = hv.vanishing_alone_case()
    assert [hv.val(v) for v in got] == want
    first, count = rec.status()
    assert count >= 1
    failing = hv.failing_assert_rows(rec)
    assert failing and all(rows <= set(identity_rows) for rows in failing)      # nothing but the identity fails
    advice, status = hg.synthesize_host(rec.tape(), rec.k, np.array(rec.inputs, dtype=np.uint64))
    assert status == (first, count) and np.array_equal(advice, rec.advice())
    assert int(rec.tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutation_is_rejected_by_the_identity(mutation, name="all_gates"):
    c = hv.verifier_case(name)
    bad = hv.verifier_mutations(name)[mutation]
    assert int((bad != c.inputs).sum()) == 1
    tape = c.rec.tape()
    advice, (first, count) = hg.synthesize_host(tape, c.rec.k, bad)
    assert count >= 1
    circuit = hv.vc.Plonky2VerifierCircuit(c.cd)
    again = circuit.record(bad)
    assert np.array_equal(again.tape(), tape)                        # the recording does not depend on the proof
    assert again.status() == (first, count)
    assert np.array_equal(advice, again.advice())
    if mutation != "public_input":                                   # a public input moves every challenge; the others must fail the identity itself
        identity = set(circuit.identity_rows)
        assert any(rows <= identity for rows in hv.failing_assert_rows(again)), "only FRI rejects this mutation"
    else:
        assert again.instance != c.rec.instance
