"""CPU: gl355_verify and the Python model verifier on a proof of a circuit that contains CosetInterpolationGate -- the gate-zoo circuit
of tests/coset_interpolation_cases.py (one row of each of {2, 4}, {3, 8}, {4, 6}), proven once on the GPU and committed as
tests/golden/coset_interpolation_proof.json (tests/golden/make_coset_interpolation_golden.py).  The circuit tables are rebuilt on the
host; the preprocessed commitment comes from the fixture and must reproduce its circuit digest.  Both verifiers accept the proof, and
both reject it at the vanishing identity when any opened wire of a column an interpolation row uses is changed."""
import base64
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import coset_interpolation_cases as cc
import coset_interpolation_model as cim
import fri_arity_cases as fc
import fri_arity_model as fm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coset_interpolation_proof.json")


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(FIXTURE))
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    b, pi, rows = cc.zoo_circuit(plonk.CircuitConfig(**g["config"]), g["circuit_seed"])
    data = b.cb.layout(g["min_degree_bits"])
    data.set_digest(np.array(g["constants_sigmas_cap"], dtype=np.uint64))
    raw = base64.b64decode(g["proof_b64"])
    return dict(g=g, plonk=plonk, data=data, pi=pi, raw=raw, rows=rows, flat=np.frombuffer(raw, dtype="<u8").astype(np.uint64))


def test_fixture_is_the_recorded_proof_of_this_circuit(golden):
    g, data = golden["g"], golden["data"]
    assert g["config"] == cc.CASE["config"] and g["circuit_seed"] == cc.CASE["circuit_seed"]
    assert hashlib.sha256(golden["raw"]).hexdigest() == g["sha256"] and len(golden["raw"]) <= 24 * 1024
    assert data.degree_bits == g["degree_bits"] == 6 and data.fri_arity_bits == g["fri_arity_bits"]
    assert [[int(t), int(p)] for t, p in data.gates] == g["gates"]
    assert sorted(p for t, p in data.gates if t == cim.COSET_INTERPOLATION) == sorted(cim.param(b, d) for b, d in ((2, 4), (3, 8), (4, 6)))
    assert [int(v) for v in data.circuit_digest] == g["circuit_digest"]
    assert [int(v) for v in golden["pi"]] == g["public_inputs"]
    assert golden["flat"].size == g["proof_words"] == fm.proof_words(data.common()) == int(golden["flat"][0])
    assert [w for _, w in golden["rows"]] == [15, 23, 47]


def test_both_verifiers_accept(orc, gl, golden, monkeypatch):
    cim.install(monkeypatch)
    assert fc.verdicts(orc, gl, golden["plonk"], golden["data"], golden["flat"], golden["pi"]) == (None, None)


def test_the_unpatched_model_does_not_know_the_gate(orc, gl, golden):
    """the accept above is the model's evaluator of the gate at work, not a verifier that skips what it does not know"""
    c_check, m_check = fc.verdicts(orc, gl, golden["plonk"], golden["data"], golden["flat"], golden["pi"])
    assert c_check is None and m_check == "unknown gate"


def test_a_changed_wire_opening_fails_the_vanishing_identity_in_both(orc, gl, golden, monkeypatch):
    cim.install(monkeypatch)
    cd, flat = golden["data"].common(), golden["flat"]
    n_cap = 1 << cd["cap_height"]
    wires_open = 8 + 3 * 4 * n_cap + 2 * (cd["num_selectors"] + cd["num_constants"] + cd["num_routed_wires"])
    for col in range(max(w for _, w in golden["rows"])):          # the 47 columns of the {4, 6} row; the smaller gates use a prefix
        for part in (0, 1) if col in (0, 1, 14, 22, 45, 46) else (col & 1,):
            bad = flat.copy()
            bad[wires_open + 2 * col + part] ^= np.uint64(1)
            c_check, m_check = fc.verdicts(orc, gl, golden["plonk"], golden["data"], bad, golden["pi"])
            assert c_check == "quotient identity fails at zeta", (col, part, c_check)
            assert m_check.startswith("quotient identity fails for challenge"), (col, part, m_check)
