"""GPU: the quotient kernel's CosetInterpolationGate evaluator (csrc/quotient.hip, the INTERP instances of quotient_kernel) against the
big-integer model (tests/coset_interpolation_model.py inside plonk_verifier.eval_vanishing_poly) at EVERY storage row of a 2^8-point
quotient coset, by the method of test_gpu_quotient_loads.py (degree_bits 5, rate_bits 3; random wires, constants, selectors and Z
columns -- the kernel is one lane per point, so a small domain reaches every path).

Two descriptors: the three interpolation gates {2, 4}, {3, 8}, {4, 6} (no, no and two intermediate pairs; one, two and four groups of
value wires) among Noop, Constant{2}, PublicInput and Arithmetic{3}, with two challenges and with one; and {4, 6} among the 11 gates the
gadget builder emits -- the gate set of a real recursive circuit.  Parameters the evaluator has no tables or wires for are refused at
launch by name."""
import importlib

import pytest

import coset_interpolation_model as cim
from test_gpu_quotient_loads import check_every_row

pytestmark = pytest.mark.gpu


def _lib():
    return importlib.import_module("stark-verifier_amd._lib")


def three_interpolation_gates(nch):
    lib = _lib()
    gates = [(lib.GATE_COSET_INTERPOLATION, cim.param(3, 8)), (lib.GATE_COSET_INTERPOLATION, cim.param(4, 6)),
             (lib.GATE_COSET_INTERPOLATION, cim.param(2, 4)), (lib.GATE_ARITHMETIC, 3), (lib.GATE_CONSTANT, 2), (lib.GATE_PUBLIC_INPUT, 0),
             (lib.GATE_NOOP, 0)]
    return dict(gates=gates, groups=[(0, 1), (1, 4), (4, 7)], routed=40, max_degree=8, npp=4, nch=nch)


def one_gate_among_the_builders_eleven():
    lib = _lib()
    gates = [(lib.GATE_POSEIDON, 0), (lib.GATE_COSET_INTERPOLATION, cim.param(4, 6)), (lib.GATE_RANDOM_ACCESS, 4 | 4 << 8 | 2 << 16),
             (lib.GATE_ARITHMETIC, 20), (lib.GATE_ARITHMETIC_EXT, 10), (lib.GATE_BASE_SUM, 32), (lib.GATE_REDUCING, 43),
             (lib.GATE_REDUCING_EXT, 32), (lib.GATE_POSEIDON_MDS, 0), (lib.GATE_CONSTANT, 2), (lib.GATE_PUBLIC_INPUT, 0), (lib.GATE_NOOP, 0)]
    return dict(gates=gates, groups=[(0, 1), (1, 3), (3, 8), (8, 12)], routed=80, max_degree=8, npp=9, nch=2)


@pytest.mark.parametrize("nch", [2, 1])
def test_every_row_three_interpolation_gates(gl, ctx, monkeypatch, nch):
    cim.install(monkeypatch)
    check_every_row(gl, ctx, three_interpolation_gates(nch), 0xC05 + nch)


def test_every_row_one_gate_among_the_builders_eleven(gl, ctx, monkeypatch):
    cim.install(monkeypatch)
    check_every_row(gl, ctx, one_gate_among_the_builders_eleven(), 0xC08)


@pytest.mark.parametrize("param,routed", [(1 | 2 << 8, 40), (5 | 6 << 8, 80), (2 | 1 << 8, 40), (2 | 5 << 8, 40), (4 | 17 << 8, 40),
                                          (4 | 6 << 8, 36), (4 | 6 << 8 | 1 << 16, 40)],
                         ids=["bits 1", "bits 5", "degree 1", "degree above N at 4 points", "degree above N at 16 points", "36 routed wires",
                              "a third field"])
def test_parameters_without_tables_or_wires_are_refused(gl, ctx, param, routed):
    """an error at launch, not a read of a column the gate does not own or of a table entry that is not there"""
    lib = _lib()
    d = dict(gates=[(lib.GATE_COSET_INTERPOLATION, param), (lib.GATE_NOOP, 0)], groups=[(0, 2)], routed=routed, max_degree=8,
             npp=(routed + 7) // 8 - 1, nch=2)
    with pytest.raises(gl.Gl355Error, match="CosetInterpolationGate"):
        check_every_row(gl, ctx, d, 0xC0F)
