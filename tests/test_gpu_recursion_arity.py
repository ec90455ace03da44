"""GPU: recursion over FRI arities above 2.  Inner proofs of the small gate-zoo circuit (fri_arity_cases.small_circuit, degree 2^6) at
reduction arities [4], [2, 3] and [1, 3] are verified by an outer circuit built with CircuitConfig.use_interpolation_gate (own arity
2), which is proven on the device and accepted by gl355_verify.  The outer witness comes once from the eager Python pass and once
through export_blob -> NativeCircuit (the tape, interpreted on the device): the rows are equal, and so are the proofs.  A second
level verifies the outer proof -- its inner circuit contains CosetInterpolationGate, so recursion.eval_gate of the gate runs -- and a
mutated inner FRI layer is refused by the device tape at the entry the host replay names.  3 queries and cap height 1 throughout."""
import ctypes as C
import importlib

import numpy as np
import pytest

import coset_interpolation_model as cim
import fri_arity_cases as fc

pytestmark = pytest.mark.gpu

ARITIES = [[4], [2, 3], [1, 3]]
_cases = {}


def _mod(name):
    return importlib.import_module("stark-verifier_amd." + name)


def outer_config(plonk):
    return plonk.CircuitConfig(use_interpolation_gate=True, zero_knowledge=False, cap_height=1, num_query_rounds=3)


def case(ctx, arities):
    """two inner proofs (two witnesses of one circuit) at `arities`, the outer circuit built from the first, its artifact"""
    key = str(arities)
    if key not in _cases:
        plonk, rec = _mod("plonk"), _mod("recursion")
        cfg = fc.config_of(plonk, reduction_arity_bits=arities, zero_knowledge=False, cap_height=1)
        inner = []
        for u in range(2):
            b, pi = fc.small_circuit(cfg, 0xA50 + u)
            if u == 0:
                data = b.cb.build(ctx, np.random.default_rng(0xA5), min_degree_bits=6)
            idx, rows = b.sparse_witness()
            inner.append((plonk.prove_sparse(ctx, data, idx, rows, pi, 0xA60 + u, flat_only=True), pi))
            data.verify(*inner[-1])
        assert data.fri_arity_bits == arities and data.degree_bits == 6
        rc = rec.RecursiveCircuit(ctx, data.common(), k=1, config=outer_config(plonk)).build([inner[0]], np.random.default_rng(0xA6))
        _cases[key] = dict(plonk=plonk, rec=rec, data=data, inner=inner, rc=rc, nat=rc.native())
    return _cases[key]


def parsed(plonk, data, flat, pi):
    proof = plonk.parse_proof(data, flat)
    proof["public_inputs"] = pi
    return proof


@pytest.mark.parametrize("arities", ARITIES, ids=str)
def test_outer_proof_by_the_python_pass_and_by_the_device_tape(gl, ctx, arities):
    c = case(ctx, arities)
    plonk, rc, nat, inner = c["plonk"], c["rc"], c["nat"], c["inner"]
    outer = rc.data
    assert outer.fri_arity_bits and all(a == 1 for a in outer.fri_arity_bits) and outer.degree_bits <= 11
    want_gates = {(12, plonk.coset_interpolation_param(a, 8)) for a in arities if a > 1}
    assert {g for g in outer.gates if g[0] == cim.COSET_INTERPOLATION} == want_gates
    # the eager pass: witness rows and proof
    b, pi_vals = rc._run([parsed(plonk, c["data"], *inner[0])])
    assert b.structure_hash() == rc.structure
    idx, rows = b.sparse_witness()
    flat_py = plonk.prove_sparse(ctx, outer, idx, rows, np.array(pi_vals, dtype=np.uint64), 0xA70, flat_only=True)
    outer.verify(flat_py, np.array(pi_vals, dtype=np.uint64))
    # the artifact: the device tape interpreter fills the same rows (and the host replay too), for both inner proofs at once
    inputs = np.stack([np.concatenate([f, p]) for f, p in inner])
    d_rows, d_pis = nat.witness_rows(ctx, inputs, on_device=True)
    h_rows, h_pis = nat.witness_rows(ctx, inputs, on_device=False)
    assert np.array_equal(d_rows, h_rows) and np.array_equal(d_pis, h_pis)
    assert np.array_equal(d_rows[0], rows) and [int(v) for v in d_pis[0]] == pi_vals
    # two units: the witness comes from the device replay inside gl355_circuit_prove_tape_units
    flats, pis = nat.prove_tape_units(ctx, inputs, [0xA70, 0xA71])
    assert np.array_equal(flats[0], flat_py) and np.array_equal(pis, d_pis)
    outer.verify(flats[1], pis[1])
    assert np.array_equal(pis[1], inner[1][1])


def test_second_level_verifies_a_circuit_that_contains_the_gate(gl, ctx):
    c = case(ctx, [2, 3])
    plonk, rec, rc = c["plonk"], c["rec"], c["rc"]
    flat1, pis1 = rc.prove_flat([c["inner"][0]], 0xA80)
    cd1 = rc.data.common()
    assert sum(1 for g in cd1["gates"] if g[0] == cim.COSET_INTERPOLATION) == 2
    rc2 = rec.RecursiveCircuit(ctx, cd1, k=1, config=outer_config(plonk)).build([(flat1, pis1)], np.random.default_rng(0xA8))
    assert not any(g[0] == cim.COSET_INTERPOLATION for g in rc2.data.gates)      # level 1 folds by 2: level 2 needs no interpolation
    flat2, pis2 = rc2.prove_flat([(flat1, pis1)], 0xA81)
    rc2.data.verify(flat2, pis2)
    assert np.array_equal(pis2, c["inner"][0][1])
    # an opened wire of an interpolation row's column, flipped in the level-1 proof, breaks level 2's vanishing identity
    bad = flat1.copy()
    n_cap = 1 << cd1["cap_height"]
    wires_open = 8 + 3 * 4 * n_cap + 2 * (cd1["num_selectors"] + cd1["num_constants"] + cd1["num_routed_wires"])
    bad[wires_open + 2 * 30] ^= np.uint64(1)
    with pytest.raises(AssertionError, match="witness generation failed"):
        rc2.witness([(bad, pis1)])


def test_a_mutated_inner_fri_layer_is_refused_by_the_tape(gl, ctx):
    c = case(ctx, [2, 3])
    gad, nat, rc = _mod("gadgets"), c["nat"], c["rc"]
    flat, pi = c["inner"][0]
    for name, bad, _ in fc.mutations(c["data"].common(), flat):
        inputs = np.concatenate([bad, pi])
        rows = np.empty((rc.row_idx.size, 135), dtype=np.uint64)
        failed = C.c_uint64(0)
        rcode = ctx.lib.gl355_witness_replay(rc.tape.ctypes.data, rc.tape.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data,
                                             rows.size, 135, C.byref(failed))
        assert rcode == -6 and rc.tape[failed.value][0] == gad.TAPE_ASSERT_EQ, name
        with pytest.raises(gl.Gl355Error) as ei:
            nat.witness_rows(ctx, inputs[None, :], on_device=True)
        assert ei.value.code == -6 and ei.value.failed_entry == failed.value, name
