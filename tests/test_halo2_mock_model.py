"""CPU: the MockProver model (tests/halo2_mock_model.py) on hand-made circuits whose answer is known by construction, the cap that keeps the
device comparison of tests/test_gpu_plonk_check.py from being vacuous (every mutation class that applies to a circuit makes the model report a
failure, for every circuit and seed that test uses), and gl355_plonk_check_witness without a context: an error code, no abort."""
import ctypes as C
import importlib

import numpy as np
import pytest

import halo2_mock_cases as mc
from halo2_mock_model import GATE, GATE_POISONED, LOOKUP, PERMUTATION, MockModel

h2 = importlib.import_module("stark-verifier_amd.halo2")


def test_next_rotation_at_the_last_usable_row_is_poisoned_unless_the_selector_is_off():
    cs = h2.ConstraintSystem()
    a, q = cs.advice_column(), cs.selector()
    cs.create_gate("count", [cs.query_selector(q) * (cs.query_advice(a, h2.Rotation.next()) - cs.query_advice(a) - 1)])
    k, n = 4, 16
    u = n - (cs.blinding_factors() + 1)
    assert u == 10
    adv = [[i if i < u else 777 for i in range(n)]]                 # whatever the blinding rows hold
    sel = [[1 if i < u - 1 else 0 for i in range(n)]]
    assert MockModel(cs, k, sel, None).verify(adv, []) == []        # q = 0 at row u - 1: 0 * poison = 0
    sel[0][u - 1] = 1
    assert MockModel(cs, k, sel, None).verify(adv, []) == [(GATE_POISONED, 0, u - 1, 0)]
    adv[0][u] = u                                                   # even a value that would satisfy the gate: it will be overwritten
    assert MockModel(cs, k, sel, None).verify(adv, []) == [(GATE_POISONED, 0, u - 1, 0)]
    adv[0][4] = 99                                                  # a plain broken cell: rows 3 and 4 read it
    assert MockModel(cs, k, sel, None).verify(adv, []) == [(GATE, 0, 3, 0), (GATE, 0, 4, 0), (GATE_POISONED, 0, u - 1, 0)]


def test_copy_cycle_across_an_advice_and_an_instance_column():
    cs = h2.ConstraintSystem()
    a, pub = cs.advice_column(), cs.instance_column()
    cs.enable_equality(a)
    cs.enable_equality(pub)
    k, n = 4, 16
    asm = h2.Assembly(n, cs.permutation)
    asm.copy(a, 3, pub, 0)
    asm.copy(a, 5, a, 3)
    adv = [[0] * n]
    adv[0][3] = adv[0][5] = 42
    model = MockModel(cs, k, [], asm.mapping_array())
    assert model.verify(adv, [[42]]) == []
    got = model.verify(adv, [[43]])                                # the instance cell leaves the cycle: it and its predecessor in the cycle differ from their partners
    assert len(got) == 2 and all(f[0] == PERMUTATION for f in got)
    assert {(f[1], f[2]) for f in got} == {(1, 0)} | {(0, r) for r in (3, 5) if tuple(int(v) for v in asm.mapping[0][r]) == (1, 0)}
    adv[0][5] = 41
    assert {(f[1], f[2]) for f in model.verify(adv, [[42]])} == {(0, 5)} | {(j, r) for j, r in ((0, 3), (1, 0)) if tuple(int(v) for v in asm.mapping[j][r]) == (0, 5)}


def test_tuple_lookup_with_one_row_off_the_table():
    cs = h2.ConstraintSystem()
    x, y = cs.advice_column(), cs.advice_column()
    t0, t1 = cs.lookup_table_column(), cs.lookup_table_column()
    cs.lookup("square", [(cs.query_advice(x), t0), (cs.query_advice(y), t1)])
    k, n = 4, 16
    u = n - (cs.blinding_factors() + 1)
    fixed = [[i for i in range(n)], [i * i for i in range(n)]]
    adv = [[(3 * i) % u for i in range(n)], [((3 * i) % u) ** 2 for i in range(n)]]
    model = MockModel(cs, k, fixed, None)
    assert model.verify(adv, []) == []
    adv[1][4] = 17                                                  # (12 % u, 17): 17 is no square
    assert model.verify(adv, []) == [(LOOKUP, 0, 4, 0)]
    adv[1][4] = (u + 1) ** 2                                        # the pair (u + 1, (u + 1)^2) sits in the table COLUMNS, but in a blinding row
    adv[0][4] = u + 1
    assert model.verify(adv, []) == [(LOOKUP, 0, 4, 0)]


@pytest.mark.parametrize("name", [c[0] for c in mc.CIRCUITS])
def test_every_applicable_mutation_class_fails_in_the_model(name):
    """the cap: the clean witness has no failure, and every class that applies to the circuit yields at least one -- with the cells and seeds
    tests/test_gpu_plonk_check.py uses.  Every circuit has gates; the chip and tuple circuits must meet all five classes."""
    case = mc.Case(name)
    assert case.clean == []
    met = 0
    for cls in mc.CLASSES:
        m = case.mutation(cls)
        assert (m is not None) == case.applies(cls)
        if m is not None:
            assert m["failures"], (name, cls)
            met += 1
    assert met >= 2
    if not name.startswith("random"):
        assert met == len(mc.CLASSES)


def test_restricted_evaluation_equals_the_full_one():
    """verify_near (the shortcut the mutation search uses) against the plain full evaluation"""
    case = mc.Case("chips-k7")
    for cls in mc.CLASSES:
        m = case.mutation(cls)
        fixed = case.fixed if m["fixed"] is None else m["fixed"]
        assert MockModel(case.cs, case.k, fixed, case.mapping).verify(m["advice"], m["instances"]) == m["failures"], cls


def test_check_witness_without_a_context_is_an_error_code(gl):
    lib = gl._lib.load()
    cs, k, w = mc.build("random-0")
    desc = h2.export_desc(cs, k, 0)
    total = C.c_uint64(7)
    lens = np.zeros(4, dtype=np.uint32)
    rc = lib.gl355_plonk_check_witness(None, desc.ctypes.data, desc.size, w.fixed.ctypes.data, None, w.advice.ctypes.data, None, lens.ctypes.data, None, 0, C.byref(total), None)
    assert rc == -1
