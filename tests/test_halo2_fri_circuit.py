"""CPU: FriVerifierChip's arithmetic and FriVerifierCircuit (halo2_verifier_circuit.py) on two real proofs made by the CPU prover
(halo2_fri_cases.py: one hiding, one not).  next_eval, batch_initial_polynomials and x_from_subgroup against the formulas of
plonk_verifier.py:326-352 for both coset positions; the circuits against the restated get_challenges, the host replay and the mock model;
four one-word mutations, each replayed on the unchanged tape, fail an ASSERT_EQ entry exactly as the re-recorded circuit says."""
import numpy as np
import pytest

import halo2_fri_cases as fc
import plonk_verifier as pv
import pymodel as pm
from test_halo2_goldilocks import mock_failures

hg, cs, P, K = fc.hg, fc.cs, fc.P, fc.K
add, sub, mul, base = pv.add, pv.sub, pv.mul, pv.base


def chip(rec, lde_bits=4, hiding=False):
    g = hg.GoldilocksChip(rec)
    g.load_table()
    return g, hg.FriVerifierChip(rec, g.assign_constant(hg.GENERATOR), lde_bits, 1, [1, 1], hiding, 3)


def accepted(rec):
    advice, status = hg.synthesize_host(rec.tape(), K, rec.inputs)
    assert status == rec.status() == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert mock_failures(rec, advice) == []


def test_vectorised_mock_rules_equal_the_model():
    """mock_failures_fast against the tree-walking model, record for record: satisfied, a failing assert (copy constraints only), and
    changed cells that break an arithmetic gate, a range lookup and a Poseidon round"""
    rec, _ = fc.extension_case()
    advice = rec.advice()
    assert fc.mock_failures_fast(rec, advice) == mock_failures(rec, advice) == []
    bad, _ = fc.zero_divisor_case()
    assert fc.mock_failures_fast(bad, bad.advice()) == mock_failures(bad, bad.advice()) != []
    row = next(e[3] for e in rec.entries if e[2] == hg.OP_MULADD_EXT)
    prec, _ = cs.permute_case()
    for r, col, r0, v in ((rec, rec.ar.r.index, row, 1), (rec, rec.ar.r_limbs[1].index, row + 1, 1 << 16), (prec, prec.po.state[2].index, prec.rows_used - 20, 1)):
        advice = r.advice()
        advice[col, r0, 0] += np.uint64(v)
        got = fc.mock_failures_fast(r, advice)
        assert got == mock_failures(r, advice) and any(f[0] == 0 for f in got)
        assert any(f[0] == 2 for f in got) == (v == 1 << 16)          # the limb that left the range table is a LOOKUP record


@pytest.mark.parametrize("within", [0, 1])
def test_next_eval(within):
    x, beta, a1, b1 = 0x1234567, (P - 3, 77), (5, P - 1), (0, 9)
    rec = hg.Recorder(K, [within, x, *beta, *a1, *b1])
    g, fri = chip(rec)
    cells = [g.assign_value(hg.Input(i)) for i in range(8)]
    bit = g.to_bits(cells[0], 1)
    got = fri.next_eval(bit, cells[1], [cells[4:6], cells[6:8]], 1, cells[2:4])
    start = x if within == 0 else (P - x) % P                        # plonk_verifier.py:343-347
    a0, b0 = base(start), base((P - start) % P)
    want = add(a1, mul(mul(sub(beta, a0), sub(b1, a1)), pm.ext_inv(sub(b0, a0))))
    assert (got[0].value, got[1].value) == want
    accepted(rec)


@pytest.mark.parametrize("index", [0b0110, 0b1011])
def test_x_from_subgroup(index):
    rec = hg.Recorder(K, [index])
    g, fri = chip(rec)
    bits = g.to_bits(g.assign_value(hg.Input(0)), 64)[:4]
    got = fri.x_from_subgroup(list(reversed(bits)))
    assert got.value == pow(pm.root_of_unity(4), pm.bitrev(index, 4), P)      # plonk_verifier.py:326 without the coset shift
    accepted(rec)


@pytest.mark.parametrize("hiding", [False, True])
def test_batch_initial_polynomials(hiding):
    rng = np.random.default_rng(0xBA7C)
    widths, nch = [3, 2, 2, 2], 2
    salt = [0, 4, 4, 4] if hiding else [0] * 4
    words = [int(v) for v in rng.integers(0, P, 2 + 2 + 2 + 1 + 4 + sum(widths) + sum(salt), dtype=np.uint64)]
    rec = hg.Recorder(K, words)
    g, fri = chip(rec, hiding=hiding)
    it = iter([g.assign_value(hg.Input(i)) for i in range(len(words))])
    take = lambda m: [next(it) for _ in range(m)]      # noqa: E731
    zeta, zeta_next, alpha, (x,), red0, red1 = take(2), take(2), take(2), take(1), take(2), take(2)
    trees = [(take(w + s), []) for w, s in zip(widths, salt)]
    info = hg.FriInstanceInfo(zeta, zeta_next, widths, nch)
    got = fri.batch_initial_polynomials(info, alpha, x, trees, [red0, red1])
    val = lambda e: (e[0].value, e[1].value)      # noqa: E731
    total = pv.E0                                                    # plonk_verifier.py:327-333
    for (point, polys), red in zip(info.batches, (red0, red1)):
        evals = [base(trees[o][0][i].value) for o, i in polys]
        num = sub(pv.reduce_with_powers(evals, val(alpha)), val(red))
        den = sub(base(x.value), val(point))
        total = add(mul(total, pv.ext_pow(val(alpha), len(evals))), mul(num, pm.ext_inv(den)))
    assert val(got) == total
    assert [len(polys) for _, polys in info.batches] == [sum(widths), nch]
    accepted(rec)


@pytest.mark.parametrize("zk", [True, False], ids=["hiding", "plain"])
def test_circuit_accepts_the_proof(zk):
    c = fc.case(zk)
    rec, circuit = c.rec, c.circuit
    assert rec.k == K and rec.status() == (hg.NO_FAILURE, 0)
    advice, status = hg.synthesize_host(rec.tape(), rec.k, c.inputs)
    assert status == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert fc.mock_failures_fast(rec, advice) == []                 # gates and lookups on every row with a selector on, every copy constraint
    assert rec.instance == [int(v) for v in c.pi_hash]
    cells, want = circuit.challenge_cells, c.challenges
    val = lambda e: tuple(x.value for x in e)      # noqa: E731
    assert val(cells["fri_alpha"]) == want["fri_alpha"] and [val(b) for b in cells["fri_betas"]] == want["fri_betas"]
    assert cells["pow_response"].value == want["pow_response"] and want["pow_response"] >> (64 - c.cd["pow_bits"]) == 0
    assert [x.value for x in cells["indices"]] == want["indices"]
    stored = [q["index"] for q in c.parse(c.flat)["opening_proof"]["query_round_proofs"]]
    assert [v & ((1 << circuit.lde_bits) - 1) for v in want["indices"]] == stored and any(v >> circuit.lde_bits for v in want["indices"])
    rows = circuit.round_rows
    assert len(rows) == 2 and rows[0][1] == rows[1][0] and rows[1][1] == rec.rows_used
    if zk:
        assert all(len(leaf) == w + (4 if o else 0) for o, ((leaf, _), w) in enumerate(zip(circuit.queries[0][1], circuit.widths)))


def test_stored_index_and_stored_words_are_not_read():
    c = fc.case(False)
    bad = c.inputs.copy()
    bad[c.circuit.queries[1][0]] ^= 5                                # the proof's stored index word of the second round
    _, status = hg.synthesize_host(c.rec.tape(), c.rec.k, bad)
    assert status == (hg.NO_FAILURE, 0)


@pytest.mark.parametrize("zk", [True, False], ids=["hiding", "plain"])
@pytest.mark.parametrize("name", ["quotient_opening", "final_poly", "pow_witness", "pi_hash"])
def test_mutation_fails_an_assert(zk, name):
    c = fc.case(zk)
    bad = fc.mutations(zk)[name]
    assert int((bad != c.inputs).sum()) == 1
    tape = c.rec.tape()
    advice, (first, count) = hg.synthesize_host(tape, c.rec.k, bad)
    assert count >= 1 and int(tape.reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    again = c.circuit.__class__(c.cd).record(bad)
    assert np.array_equal(again.tape(), tape)                        # the recording does not depend on the proof
    assert again.status() == (first, count)
    assert np.array_equal(advice, again.advice())
