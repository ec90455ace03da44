"""CPU: FriOpeningsCircuit (halo2_verifier_circuit.py) on a proof-shaped input vector small enough for the host: a plonky2 proof layout with
lde 2^4, cap height 1, two query rounds and two FRI layers, whose Merkle trees are built with the oracle's BN254-Poseidon hasher (the opened
values are random: part 1 checks the openings, not the arithmetic between them).  The host replay equals the recorder cell for cell and
reports no failure, and the mock model (gates, lookups, copy constraints) accepts it; the caps and the indices are the instances; a flipped sibling word fails an ASSERT_EQ entry and breaks copy constraints
only inside that round's rows.  The wrap proof's circuit runs in test_gpu_halo2_synth.py."""
import importlib

import numpy as np
import pytest

import halo2_synth_cases as cs
from oracle_lib import Bn254Oracle
from test_halo2_goldilocks import mock_failures

hg, P = cs.hg, cs.P
vc = importlib.import_module("stark-verifier_amd.halo2_verifier_circuit")

COMMON = dict(degree_bits=3, rate_bits=1, cap_height=1, num_query_rounds=2, arity_bits=[1, 1], hiding=False, hasher=1, num_challenges=2, num_selectors=1,
              num_constants=1, num_routed_wires=3, num_wires=9, num_partial_products=1, quotient_degree_factor=2)
INDICES = (11, 4)


def small_proof(bn):
    """-> (common data with its constants_sigmas cap, the flat proof words)"""
    rng = np.random.default_rng(0xF21)
    circuit = vc.FriOpeningsCircuit(dict(COMMON, constants_sigmas_cap=np.zeros((2, 4), dtype=np.uint64)))
    words = lambda m: [int(v) for v in rng.integers(0, P, m, dtype=np.uint64)]       # noqa: E731
    initial_leaves = [[words(ll) for _ in range(16)] for ll in circuit.leaf_len]
    trees = [cs.merkle_tree(bn, leaves, 1) for leaves in initial_leaves]
    flat = np.array(words(circuit.proof_words), dtype=np.uint64)
    flat[:8] = [circuit.proof_words, 3, 2, 2, 0, 0, 1, 2]
    layers = []
    for layer in range(2):
        leaves = [words(4) for _ in range(8 >> layer)]
        layers.append((leaves,) + cs.merkle_tree(bn, leaves, 1))

    def put(positions, values):
        flat[positions] = np.array(values, dtype=np.uint64)
    for o, (cap, _) in enumerate(trees):
        if o:
            for pos, h in zip(circuit.initial_caps[o], cap):
                put(pos, h)
    for l, (_, cap, _) in enumerate(layers):
        for pos, h in zip(circuit.layer_caps[l], cap):
            put(pos, h)
    for (index_pos, initial, steps), index in zip(circuit.queries, INDICES):
        flat[index_pos] = index
        for o, (leaf_pos, sib_pos) in enumerate(initial):
            put(leaf_pos, initial_leaves[o][index])
            for pos, h in zip(sib_pos, trees[o][1][index]):
                put(pos, h)
        for l, (leaf_pos, sib_pos) in enumerate(steps):
            leaves, _, proofs = layers[l]
            put(leaf_pos, leaves[index >> (l + 1)])
            for pos, h in zip(sib_pos, proofs[index >> (l + 1)]):
                put(pos, h)
    return dict(COMMON, constants_sigmas_cap=np.array(trees[0][0], dtype=np.uint64)), flat


@pytest.fixture(scope="module")
def recorded(orc):
    cd, flat = small_proof(Bn254Oracle(orc))
    circuit = vc.FriOpeningsCircuit(cd)
    inputs = circuit.inputs(flat)
    return circuit, inputs, circuit.record(inputs)


def test_shape_and_instances(recorded):
    circuit, inputs, rec = recorded
    assert rec.k == 17 and circuit.n_inputs == inputs.size == circuit.proof_words + 8
    caps = [int(inputs[w]) for cap in circuit.initial_caps + circuit.layer_caps for h in cap for w in h]
    assert rec.instance == caps + list(INDICES)
    assert len(circuit.round_rows) == 2 and circuit.round_rows[0][1] == circuit.round_rows[1][0] and circuit.round_rows[1][1] == rec.rows_used


def test_host_replay_accepts_the_openings(recorded):
    circuit, inputs, rec = recorded
    assert rec.status() == (hg.NO_FAILURE, 0)
    advice, status = hg.synthesize_host(rec.tape(), rec.k, inputs)
    assert status == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert mock_failures(rec, advice) == []          # gates and lookups on every row with a selector on, every copy constraint


@pytest.mark.parametrize("query,what", [(1, "initial"), (0, "layer")])
def test_flipped_sibling_fails_inside_its_round(recorded, query, what):
    circuit, inputs, rec = recorded
    _, initial, steps = circuit.queries[query]
    word = initial[2][1][1][3] if what == "initial" else steps[1][1][0][0]
    bad = inputs.copy()
    bad[word] ^= 1
    advice, (first, count) = hg.synthesize_host(rec.tape(), rec.k, bad)
    assert count >= 1 and int(rec.tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    lay = rec.layout()
    fails = cs.copy_failures(rec.cs, lay.mapping_array(), advice, lay.fixed_array(), rec.instance)
    lo, hi = circuit.round_rows[query]
    assert fails and all(lo <= f[2] < hi for f in fails)
