"""CPU: CosetInterpolationGate -- the big-integer model (tests/coset_interpolation_model.py) against the gate's definition and against the
interpolant it exists for (fri_arity_model.interpolate), and the library's host witness generators (gl355_coset_interpolation_witness,
the COSET_INTERP tape entry of gl355_witness_replay) against the model.  Arithmetic is exact: every comparison is equality."""
import ctypes as C
import importlib

import numpy as np
import pytest

import coset_interpolation_model as cim
import fri_arity_model as fm
import plonk_verifier as pv
import pymodel as pm
from oracle_lib import P, rand_field

BITS = [2, 3, 4]
#        bits: (degree, intermediates, routed wires, wires, constraints) at max_quotient_degree_factor 8
WANT = {2: (4, 0, 13, 15, 4), 3: (8, 0, 21, 23, 4), 4: (6, 2, 37, 47, 12)}


def _plonk():
    return importlib.import_module("stark-verifier_amd.plonk")


def _gad():
    return importlib.import_module("stark-verifier_amd.gadgets")


def _inputs(bits, seed):
    rng = np.random.default_rng(seed)
    v = [int(x) for x in rand_field(rng, 2 * (1 << bits) + 3)]
    return v[0] or 1, [(v[1 + 2 * i], v[2 + 2 * i]) for i in range(1 << bits)], (v[-2], v[-1])


@pytest.mark.parametrize("bits", BITS)
def test_layout(bits):
    degree, n_int = cim.with_max_degree(bits, 8)
    lay = cim.layout(bits, degree)
    assert (degree, n_int, lay["num_routed"], lay["num_wires"], lay["num_constraints"]) == WANT[bits]
    assert lay["n_int"] == n_int and lay["values"][0] == 1 and lay["point"] == 1 + 2 * lay["n"] and lay["value"] == lay["point"] + 2
    assert lay["start_int"] == lay["point"] + 4 and lay["shifted"] == lay["start_int"] + 4 * n_int
    # the fold's chunks cover every point once
    covered = [i for lo, hi in cim.chunks(lay) for i in range(lo, hi)]
    assert covered == list(range(lay["n"]))
    # the product's tables say the same
    plonk = _plonk()
    p = plonk.coset_interpolation_param(bits, 8)
    assert p == cim.param(bits, degree)
    sh = plonk.coset_interpolation_shape(p)
    assert {k: sh[k] for k in ("n_int", "point", "value", "start_int", "shifted", "num_wires", "num_constraints")} == \
           {k: lay[k] for k in ("n_int", "point", "value", "start_int", "shifted", "num_wires", "num_constraints")}
    assert plonk._GATE_DEGREE[cim.COSET_INTERPOLATION](p) == degree and plonk._GATE_CONSTRAINTS[cim.COSET_INTERPOLATION](p) == lay["num_constraints"]
    assert plonk.gate_id_string(cim.COSET_INTERPOLATION, p).startswith("CosetInterpolationGate { subgroup_bits: %d, degree: %d, barycentric_weights: [%d, " %
                                                                      (bits, degree, cim.weights_by_product(bits)[0]))


@pytest.mark.parametrize("bits", BITS)
def test_weights_by_product_and_on_the_subgroup_agree(bits):
    assert cim.weights_by_product(bits) == cim.weights_on_subgroup(bits) == _plonk().coset_interpolation_weights(bits)
    assert cim.domain(bits)[1] == pm.root_of_unity(bits) and len(set(cim.domain(bits))) == 1 << bits


@pytest.mark.parametrize("bits", BITS)
def test_constraints_vanish_on_the_generated_witness_and_on_no_other(bits):
    degree, _ = cim.with_max_degree(bits, 8)
    shift, values, point = _inputs(bits, 0xC1 + bits)
    w = cim.generate(bits, degree, shift, values, point)
    gate = (cim.COSET_INTERPOLATION, cim.param(bits, degree))
    assert all(c == pv.E0 for c in cim.eval_gate(gate, [], [pv.base(v) for v in w], None))
    for j in range(len(w)):            # every wire is constrained
        bad = list(w)
        bad[j] = (bad[j] + 1) % P
        assert any(c != pv.E0 for c in cim.eval_gate(gate, [], [pv.base(v) for v in bad], None)), "wire %d is free" % j


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("degree_of", ["with_max_degree", 2, "n"])
def test_value_is_the_interpolant_on_the_coset(bits, degree_of):
    n = 1 << bits
    degree = cim.with_max_degree(bits, 8)[0] if degree_of == "with_max_degree" else (2 if degree_of == 2 else n)
    shift, values, point = _inputs(bits, 0xD1 + bits)
    w = cim.generate(bits, degree, shift, values, point)
    lay = cim.layout(bits, degree)
    g = pm.root_of_unity(bits)
    points = [shift * pow(g, i, P) % P for i in range(n)]
    want = fm.interpolate(points, [pv.ext(v) for v in values], pv.ext(point))
    assert (w[lay["value"]], w[lay["value"] + 1]) == want
    assert all(c == pv.E0 for c in cim.eval_gate((cim.COSET_INTERPOLATION, cim.param(bits, degree)), [], [pv.base(v) for v in w], None))


@pytest.mark.parametrize("bits", BITS)
def test_library_generator_equals_the_model(gl, bits):
    plonk = _plonk()
    for degree in sorted({cim.with_max_degree(bits, 8)[0], 2, 3, 1 << bits}):
        shift, values, point = _inputs(bits, 0xE1 + 16 * bits + degree)
        want = cim.generate(bits, degree, shift, values, point)
        lay = cim.layout(bits, degree)
        got = plonk.coset_interpolation_witness(cim.param(bits, degree), np.array(want[:lay["point"] + 2], dtype=np.uint64))
        assert [int(v) for v in got] == want, (bits, degree)


def test_library_generator_refuses_bad_parameters_and_a_zero_shift(gl):
    lib = gl._lib.load()
    w = np.ones(64, dtype=np.uint64)
    for bits, degree in ((1, 2), (5, 4), (2, 1), (2, 5), (4, 17), (0, 0)):
        assert lib.gl355_coset_interpolation_witness(bits, degree, w.ctypes.data) == -1, (bits, degree)      # GL355_E_INVALID_ARG
    w[0] = 0
    assert lib.gl355_coset_interpolation_witness(2, 4, w.ctypes.data) == -6                                    # GL355_E_WITNESS
    w[0] = P                                                                                                   # zero, non-canonical
    assert lib.gl355_coset_interpolation_witness(2, 4, w.ctypes.data) == -6
    with pytest.raises(ValueError, match="shift is zero"):
        _plonk().coset_interpolation_witness(cim.param(2, 4), np.zeros(11, dtype=np.uint64))


def _builder_with_three_gates(seed, flag=True):
    plonk, gad = _plonk(), _gad()
    b = gad.GadgetBuilder(plonk.CircuitConfig(use_interpolation_gate=flag, zero_knowledge=False))
    outs = []
    for bits in BITS:
        shift, values, point = _inputs(bits, seed + bits)
        st = b.add_virtual_target(plonk.Src(shift, 0))
        vt = [b.add_virtual_ext((plonk.Src(v[0], 0), plonk.Src(v[1], 0))) for v in values]
        pt = b.add_virtual_ext((plonk.Src(point[0], 0), plonk.Src(point[1], 0)))
        outs.append((bits, shift, values, point, b.interpolate_coset(bits, st, vt, pt)))
    return b, outs


def test_interpolate_coset_rows_and_value():
    b, outs = _builder_with_three_gates(0xF0)
    assert cim.check_rows(b)[cim.COSET_INTERPOLATION] == 3
    for bits, shift, values, point, out in outs:
        g = pm.root_of_unity(bits)
        want = fm.interpolate([shift * pow(g, i, P) % P for i in range(1 << bits)], [pv.ext(v) for v in values], pv.ext(point))
        assert (out[0].v, out[1].v) == want
        assert out[0].col < b.routed and out[1].col < b.routed           # the value can be copied on
    gates = [g for g in b.cb.gate_types if g[0] == cim.COSET_INTERPOLATION]
    assert gates == [(12, cim.param(2, 4)), (12, cim.param(3, 8)), (12, cim.param(4, 6))]
    # the degree-8 gate sits alone in its selector group
    data = b.cb.layout(0)
    gi = data.gates.index((12, cim.param(3, 8)))
    assert data.groups[data.selector_indices[gi]] == (gi, gi + 1)
    plonk = _plonk()
    wires = np.zeros((b.nw, 1 << data.degree_bits), dtype=np.uint64)
    idx, vals = b.sparse_witness()
    wires[:, idx] = vals.T
    plonk.check_copy_constraints(data, wires)


def test_interpolate_coset_needs_the_flag():
    with pytest.raises(ValueError, match="use_interpolation_gate"):
        _builder_with_three_gates(0xF0, flag=False)
    b = _gad().GadgetBuilder()
    assert b.cb.config.use_interpolation_gate is False


def test_tape_replay_equals_the_eager_witness(gl):
    plonk, lib = _plonk(), gl._lib.load()
    b, _ = _builder_with_three_gates(0xF8)
    # the inputs in tape order: every INPUT entry reads its own position
    flat = []
    for k, e in enumerate(b.tape):
        if e[0] == 1:
            flat.append(b.rows[e[1] // b.nw][e[1] % b.nw])
            b.tape[k] = (1, e[1], len(flat) - 1, 0, 0)
    tape, idx, _ = b.witness_tape()
    _, want = b.sparse_witness()
    inputs = np.array(flat, dtype=np.uint64)
    rows = np.empty_like(want)
    failed = C.c_uint64(0)
    assert (tape[:, 0] == 14).sum() == 3
    rc = lib.gl355_witness_replay(tape.ctypes.data, tape.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data, rows.size, b.nw, C.byref(failed))
    assert rc == 0 and np.array_equal(rows, want)
    # a zero shift is a failed entry: the first gate's shift is input 0
    first = int(np.nonzero(tape[:, 0] == 14)[0][0])
    inputs[0] = 0
    rc = lib.gl355_witness_replay(tape.ctypes.data, tape.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data, rows.size, b.nw, C.byref(failed))
    assert (rc, failed.value) == (-6, first)
    inputs[0] = flat[0]
    # wrong bits / degree / offsets are invalid arguments, reported at the entry
    for field, value in ((2, 1), (2, 5), (3, 1), (3, 17), (1, int(tape[first, 1]) + 1), (1, rows.size - 8), (1, rows.size + b.nw)):
        bad = tape.copy()
        bad[first, field] = value
        rc = lib.gl355_witness_replay(bad.ctypes.data, bad.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data, rows.size, b.nw, C.byref(failed))
        assert (rc, failed.value) == (-1, first), (field, value)
