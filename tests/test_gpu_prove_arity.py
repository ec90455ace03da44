"""GPU: whole proofs at FRI reduction arities above 2 -- gl355_prove / gl355_prove_sparse_units of a small gate-zoo circuit with
CircuitConfig(reduction_arity_bits = 3 | 2 | [1, 3]), zero-knowledge on and off, 3 queries.  Each proof has the length the layout rule
gives, is accepted by gl355_verify and by the Python model verifier (tests/fri_arity_model.py), and both reject the same mutations of
its FRI layers at the same named check."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fri_arity_cases as fc
import fri_arity_model as fm

pytestmark = pytest.mark.gpu

CONFIGS = [(3, True), (3, False), (2, True), (2, False), ([1, 3], True), ([1, 3], False)]
MIN_DEGREE_BITS = 7      # without blinding rows the circuit has 2^5 rows, which ConstantArityBits(a, 5) does not fold at all
_cases = {}


def case(gl, ctx, arity, zk):
    """the circuit built on the device once per config, three witnesses of it and the first one's proof"""
    key = (str(arity), zk)
    if key not in _cases:
        plonk = importlib.import_module("stark-verifier_amd.plonk")
        cfg = fc.config_of(plonk, reduction_arity_bits=arity, zero_knowledge=zk)
        builders = [fc.small_circuit(cfg, 0x7A0 + u) for u in range(3)]
        b, pi = builders[0]
        data = b.cb.build(ctx, np.random.default_rng(0x7A9), min_degree_bits=0 if zk else MIN_DEGREE_BITS)
        idx, rows = b.sparse_witness()
        flat = plonk.prove_sparse(ctx, data, idx, rows, pi, 0x7B0, flat_only=True)
        _cases[key] = dict(plonk=plonk, data=data, idx=idx, rows=rows, pi=pi, flat=flat, builders=builders)
    return _cases[key]


@pytest.mark.parametrize("arity,zk", CONFIGS)
def test_proof_has_the_computed_length_and_both_verifiers_accept(gl, ctx, orc, arity, zk):
    c = case(gl, ctx, arity, zk)
    data, plonk, flat = c["data"], c["plonk"], c["flat"]
    cd = data.common()
    assert any(a > 1 for a in cd["arity_bits"]), cd["arity_bits"]
    assert isinstance(arity, int) or cd["arity_bits"] == arity
    words = ctx.lib.gl355_proof_words(C.byref(data.prover_data(ctx)))
    assert flat.size == words == fm.proof_words(cd) == int(flat[0])
    # shorter than the arity-2 proof of the same circuit by the layer part of every query
    cd2 = dict(cd, arity_bits=[1] * sum(cd["arity_bits"]))
    assert fm.proof_words(cd2) > words
    assert fc.verdicts(orc, gl, plonk, data, flat, c["pi"]) == (None, None)


@pytest.mark.parametrize("arity,zk", [(3, True), ([1, 3], False)])
def test_mutations_are_rejected_at_the_same_check(gl, ctx, orc, arity, zk):
    c = case(gl, ctx, arity, zk)
    data, plonk = c["data"], c["plonk"]
    for name, bad, want in fc.mutations(data.common(), c["flat"]):
        c_check, m_check = fc.verdicts(orc, gl, plonk, data, bad, c["pi"])
        assert m_check == want, name
        assert c_check == want.split()[0], name


def test_a_proof_of_another_arity_is_refused_by_its_shape(gl, ctx, orc):
    """a proof made with arities [3] offered to verifier data saying [1, 1, 1]"""
    c = case(gl, ctx, 3, False)
    data, plonk = c["data"], c["plonk"]
    assert data.fri_arity_bits == [3]
    other = fc.small_circuit(fc.config_of(plonk, reduction_arity_bits=[1, 1, 1], zero_knowledge=False), 0x7A0)[0].cb.layout(MIN_DEGREE_BITS)
    assert other.degree_bits == data.degree_bits and other.fri_arity_bits == [1, 1, 1]
    other.set_digest(data.constants_sigmas_cap)
    assert np.array_equal(other.circuit_digest, data.circuit_digest)
    assert fc.verdicts(orc, gl, plonk, other, c["flat"], c["pi"]) == ("shape", "shape")


def test_an_explicit_all_ones_array_gives_the_bytes_of_null(gl, ctx):
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=1, zero_knowledge=True)
    b, pi = fc.small_circuit(cfg, 0x7A0)
    data = b.cb.build(ctx, np.random.default_rng(0x7A9))
    idx, rows = b.sparse_witness()
    assert data.fri_arity_bits and all(a == 1 for a in data.fri_arity_bits)
    pd = data.prover_data(ctx)
    assert pd.fri_arity_bits
    with_array = plonk.prove_sparse(ctx, data, idx, rows, pi, 0x7B1, flat_only=True)
    saved, pd.fri_arity_bits = pd.fri_arity_bits, None
    try:
        assert not pd.fri_arity_bits
        with_null = plonk.prove_sparse(ctx, data, idx, rows, pi, 0x7B1, flat_only=True)
    finally:
        pd.fri_arity_bits = saved
    assert np.array_equal(with_array, with_null)
    data.verify(with_null, pi)


def test_the_staged_prover_follows_the_arities(gl, ctx, orc):
    """plonk.prove_staged (gl355_fri_prove with the circuit's arities, behind the individual entry points) gives a proof the model accepts"""
    c = case(gl, ctx, [1, 3], False)
    data, plonk = c["data"], c["plonk"]
    wires = np.zeros((data.config.num_wires, 1 << data.degree_bits), dtype=np.uint64)
    wires[:, c["idx"]] = c["rows"].T
    proof = plonk.prove_staged(ctx, data, wires, c["pi"], np.random.default_rng(0x7B7))
    assert [len(e) for e, _ in proof["opening_proof"]["query_round_proofs"][0]["steps"]] == [4, 16]
    fm.verify(orc, data.common(), proof)


@pytest.mark.parametrize("arity,zk", [(3, True), ([1, 3], False)])
def test_three_lock_step_units_equal_the_single_proofs(gl, ctx, arity, zk):
    c = case(gl, ctx, arity, zk)
    data, plonk = c["data"], c["plonk"]
    wit = [b.sparse_witness() for b, _ in c["builders"]]
    assert all(np.array_equal(w[0], c["idx"]) for w in wit)
    rows = np.stack([w[1] for w in wit])
    pis = np.stack([pi for _, pi in c["builders"]])
    seeds = [0x7B0, 0x7B3, 0x7B4]
    flat = plonk.prove_sparse_units(ctx, data, c["idx"], rows, pis, seeds)
    assert np.array_equal(flat[0], c["flat"])
    for u in (1, 2):
        assert np.array_equal(flat[u], plonk.prove_sparse(ctx, data, c["idx"], rows[u], pis[u], seeds[u], flat_only=True)), u
        data.verify(flat[u], pis[u])
