"""CPU: gl355_verify and the Python model verifier (tests/fri_arity_model.py) on a proof with FRI reduction arities [2, 3], made once
on the GPU and committed as tests/golden/fri_arity_proof.json (tests/golden/make_fri_arity_golden.py).  The circuit tables are
rebuilt on the host from the fixture's configuration; the preprocessed commitment comes from the fixture and must reproduce its
circuit digest.  Both verifiers accept the proof and reject the same mutations of its FRI layers at the same named check."""
import base64
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import fri_arity_cases as fc
import fri_arity_model as fm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_arity_proof.json")


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(FIXTURE))
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    b, pi = fc.small_circuit(plonk.CircuitConfig(**g["config"]), g["circuit_seed"])
    data = b.cb.layout(g["min_degree_bits"])
    data.set_digest(np.array(g["constants_sigmas_cap"], dtype=np.uint64))
    raw = base64.b64decode(g["proof_b64"])
    return dict(g=g, plonk=plonk, data=data, pi=pi, raw=raw, flat=np.frombuffer(raw, dtype="<u8").astype(np.uint64))


def test_fixture_is_the_recorded_proof_of_this_circuit(golden):
    g, data = golden["g"], golden["data"]
    assert hashlib.sha256(golden["raw"]).hexdigest() == g["sha256"]
    assert data.degree_bits == g["degree_bits"] <= 6 and data.fri_arity_bits == g["fri_arity_bits"] == [2, 3]
    assert [int(v) for v in data.circuit_digest] == g["circuit_digest"]
    assert [int(v) for v in golden["pi"]] == g["public_inputs"]
    assert golden["flat"].size == g["proof_words"] == fm.proof_words(data.common()) == int(golden["flat"][0])


def test_both_verifiers_accept(orc, gl, golden):
    assert fc.verdicts(orc, gl, golden["plonk"], golden["data"], golden["flat"], golden["pi"]) == (None, None)


def test_mutations_are_rejected_at_the_same_check(orc, gl, golden):
    data = golden["data"]
    seen = []
    for name, bad, want in fc.mutations(data.common(), golden["flat"]):
        c_check, m_check = fc.verdicts(orc, gl, golden["plonk"], data, bad, golden["pi"])
        assert m_check == want, name
        assert c_check == want.split()[0], name
        seen.append(want.split()[0])
    assert seen == ["merkle", "fold", "fold", "pow"]
    # a mutated public input fails earlier, in both
    pi = golden["pi"].copy()
    pi[1] ^= np.uint64(1)
    c_check, m_check = fc.verdicts(orc, gl, golden["plonk"], data, golden["flat"], pi)
    assert c_check is not None and m_check is not None


def test_a_proof_of_another_arity_is_refused_by_its_shape(orc, gl, golden):
    g, plonk = golden["g"], golden["plonk"]
    for arities in ([1, 1, 1, 1, 1], [3, 2], [2]):
        cfg = plonk.CircuitConfig(**dict(g["config"], reduction_arity_bits=arities))
        other = fc.small_circuit(cfg, g["circuit_seed"])[0].cb.layout(g["min_degree_bits"])
        other.set_digest(np.array(g["constants_sigmas_cap"], dtype=np.uint64))
        assert [int(v) for v in other.circuit_digest] == g["circuit_digest"]
        assert fc.verdicts(orc, gl, plonk, other, golden["flat"], golden["pi"]) == ("shape", "shape"), arities


def test_out_of_scope_consumers_refuse_by_name(golden):
    """the artifact, the in-circuit verifier and the Halo2 verifier circuit speak arity-2 FRI only"""
    data, plonk = golden["data"], golden["plonk"]
    with pytest.raises(ValueError, match="arity-2 FRI only"):
        data.export_blob(np.zeros(0, dtype=np.uint32))
    rec = importlib.import_module("stark-verifier_amd.recursion")
    gad = importlib.import_module("stark-verifier_amd.gadgets")
    proof = plonk.parse_proof(data, golden["flat"])
    proof["public_inputs"] = golden["pi"]
    with pytest.raises(ValueError, match="arity-2 FRI only"):
        rec.verify_proof(gad.GadgetBuilder(), data.common(), proof)
    hvc = importlib.import_module("stark-verifier_amd.halo2_verifier_circuit")
    with pytest.raises(ValueError, match="arity-2 FRI only"):
        hvc.FriOpeningsCircuit(dict(data.common(), hasher=1))


def test_config_accepts_an_int_or_a_list(golden):
    plonk = golden["plonk"]
    assert plonk.CircuitConfig(reduction_arity_bits=3).fri_reduction_arity_bits(13) == [3, 3, 3]
    assert plonk.CircuitConfig(reduction_arity_bits=4).fri_reduction_arity_bits(13) == [4, 4]
    assert plonk.CircuitConfig().fri_reduction_arity_bits(13) == [1] * 8
    assert plonk.CircuitConfig(reduction_arity_bits=[1, 3]).fri_reduction_arity_bits(13) == [1, 3]
    for bad in (5, [0, 1], [4, 5], 0):
        with pytest.raises(ValueError):
            plonk.CircuitConfig(reduction_arity_bits=bad).fri_reduction_arity_bits(13)
    with pytest.raises(ValueError):
        plonk.CircuitConfig(reduction_arity_bits=[4, 4]).fri_reduction_arity_bits(6)
