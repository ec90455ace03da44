"""CPU: the in-circuit verifier on FRI arities above 2 (recursion.verify_proof with CircuitConfig.use_interpolation_gate), on the committed
proof with arities [2, 3] of tests/golden/fri_arity_proof.json, whose circuit is rebuilt as in test_verify_arity_host.py.

The outer circuit's witness must satisfy every gate (the big-integer model of each gate, coset_interpolation_model.check_rows) and
every copy constraint; the recorded tape, replayed on the host from the flat proof's words, must give the same rows; and the FRI-layer
mutations of fri_arity_cases.mutations -- which both native verifiers reject -- must fail here too: the Python pass at a connect(),
the replay at an ASSERT_EQ entry."""
import base64
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import coset_interpolation_model as cim
import fri_arity_cases as fc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_arity_proof.json")


def _mod(name):
    return importlib.import_module("stark-verifier_amd." + name)


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(FIXTURE))
    plonk = _mod("plonk")
    b, pi = fc.small_circuit(plonk.CircuitConfig(**g["config"]), g["circuit_seed"])
    data = b.cb.layout(g["min_degree_bits"])
    data.set_digest(np.array(g["constants_sigmas_cap"], dtype=np.uint64))
    flat = np.frombuffer(base64.b64decode(g["proof_b64"]), dtype="<u8").astype(np.uint64)
    return dict(plonk=plonk, data=data, cd=data.common(), pi=pi, flat=flat)


def outer_pass(golden, flat, flag=True):
    """the eager gadget pass of an outer circuit that verifies `flat` -> (builder, public-input values)"""
    plonk, rec, gad = golden["plonk"], _mod("recursion"), _mod("gadgets")
    cfg = plonk.CircuitConfig(use_interpolation_gate=flag, zero_knowledge=False, cap_height=1, num_query_rounds=3)
    b = gad.GadgetBuilder(cfg)
    tagged = plonk.parse_proof_tagged(golden["cd"], flat, golden["pi"], 0)
    rec.verify_proof(b, golden["cd"], tagged)
    return b, b.finalize_public_inputs()


@pytest.fixture(scope="module")
def outer(golden):
    b, pi_vals = outer_pass(golden, golden["flat"])
    tape, idx, pi_pos = b.witness_tape()
    return dict(b=b, pi_vals=pi_vals, tape=tape, idx=idx, pi_pos=pi_pos)


def replay(gl, outer, flat, pi):
    lib = gl._lib.load()
    tape, nw = outer["tape"], outer["b"].nw
    inputs = np.concatenate([np.asarray(flat, dtype=np.uint64), np.asarray(pi, dtype=np.uint64)])
    rows = np.empty((outer["idx"].size, nw), dtype=np.uint64)
    failed = C.c_uint64(0)
    rc = lib.gl355_witness_replay(tape.ctypes.data, tape.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data, rows.size, nw, C.byref(failed))
    return rc, rows, failed.value


def test_outer_circuit_builds_and_every_row_satisfies_its_gate(golden, outer):
    b, plonk = outer["b"], golden["plonk"]
    assert golden["cd"]["arity_bits"] == [2, 3] and outer["pi_vals"] == [int(v) for v in golden["pi"]]
    pi_hash = [int(v) for v in plonk.host_hash_no_pad(np.array(outer["pi_vals"], dtype=np.uint64))]
    seen = cim.check_rows(b, pi_hash)
    # one interpolation row per query and layer: {2, 4} for the arity-4 layer, {3, 8} for the arity-8 layer
    assert seen[cim.COSET_INTERPOLATION] == 2 * golden["cd"]["num_query_rounds"]
    assert [g for g in b.cb.gate_types if g[0] == cim.COSET_INTERPOLATION] == [(12, cim.param(2, 4)), (12, cim.param(3, 8))]
    assert set(seen) == set(range(13)) - {7}         # every gate kind the builder emits (MulExtension is not one), the thirteenth included
    data = b.cb.layout(0)
    assert data.degree_bits <= 11
    wires = np.zeros((b.nw, 1 << data.degree_bits), dtype=np.uint64)
    idx, vals = b.sparse_witness()
    wires[:, idx] = vals.T
    plonk.check_copy_constraints(data, wires)
    assert data.num_gate_constraints == 123 and len(data.gates) <= 16


def test_tape_replay_from_the_flat_proof_gives_the_same_rows(gl, golden, outer):
    b = outer["b"]
    idx, vals = b.sparse_witness()
    rc, rows, _ = replay(gl, outer, golden["flat"], golden["pi"])
    assert rc == 0 and np.array_equal(outer["idx"], idx) and np.array_equal(rows, vals)
    assert [int(v) for v in rows.reshape(-1)[outer["pi_pos"]]] == outer["pi_vals"]
    assert (outer["tape"][:, 0] == 14).sum() == 2 * golden["cd"]["num_query_rounds"]
    # the query rounds stay independent segments with the interpolation entries inside them
    n_seq, seg_lens = b.tape_layout
    assert len(seg_lens) == golden["cd"]["num_query_rounds"] and not (outer["tape"][:n_seq, 0] == 14).any()


def test_fri_layer_mutations_fail_in_circuit(gl, golden, outer):
    gad = _mod("gadgets")
    names = []
    for name, bad, _ in fc.mutations(golden["cd"], golden["flat"]):
        with pytest.raises(AssertionError, match=r"connect\(\) of targets with different values"):
            outer_pass(golden, bad)
        rc, _, failed = replay(gl, outer, bad, golden["pi"])
        assert rc == -6 and outer["tape"][failed][0] == gad.TAPE_ASSERT_EQ, name
        names.append(name)
    assert len(names) == 4


def test_flag_off_refuses_with_the_arity_2_message(golden):
    with pytest.raises(ValueError, match="the in-circuit verifier supports arity-2 FRI only"):
        outer_pass(golden, golden["flat"], flag=False)
    with pytest.raises(ValueError, match="2, 4, 8 or 16"):
        rec, gad = _mod("recursion"), _mod("gadgets")
        b = gad.GadgetBuilder(golden["plonk"].CircuitConfig(use_interpolation_gate=True))
        rec.verify_proof(b, dict(golden["cd"], arity_bits=[5]), None)


def test_halo2_gate_constrainer_refuses_the_gate_by_name():
    hpc = _mod("halo2_plonk_chips")
    with pytest.raises(ValueError, match="CosetInterpolationGate"):
        hpc.GateConstrainer(None, (cim.COSET_INTERPOLATION, cim.param(3, 8)))


@pytest.mark.parametrize("bits,degree", [(2, 4), (3, 8), (4, 6), (4, 2)])
def test_in_circuit_evaluator_equals_the_model_on_random_extension_wires(bits, degree):
    """recursion.eval_gate of the gate, for inner circuits that themselves contain it: the targets' values are the model's constraints"""
    from oracle_lib import rand_field
    rec, gad = _mod("recursion"), _mod("gadgets")
    lay = cim.layout(bits, degree)
    rng = np.random.default_rng(0xE7A + bits + degree)
    w = [(int(a), int(c)) for a, c in rand_field(rng, (lay["num_wires"], 2))]
    b = gad.GadgetBuilder()
    got = rec.eval_gate(b, (cim.COSET_INTERPOLATION, cim.param(bits, degree)), [], [b.add_virtual_ext(v) for v in w], None)
    want = cim.eval_gate((cim.COSET_INTERPOLATION, cim.param(bits, degree)), [], w, None)
    assert [(t[0].v, t[1].v) for t in got] == want and any(c != (0, 0) for c in want)
    assert not any(g[0] == cim.COSET_INTERPOLATION for g in b.cb.gate_types)       # evaluating the gate does not need the gate
