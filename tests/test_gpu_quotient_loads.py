"""GPU: the quotient kernel's grouped column reads (csrc/quotient.hip) against the big-integer evaluation of vanishing_poly.rs
(plonk_verifier.eval_vanishing_poly) at EVERY storage row of a 2^8-point quotient coset (degree_bits 5, rate_bits 3: two
workgroups, four waves -- the kernel is one lane per point with no cross-lane traffic, so a small domain reaches every path).
Inputs are random wires / constants / selectors / Z columns, as in test_gpu_prover.test_gate_set_pointwise.

Three descriptors: that test's gate set unchanged; gate parameters on the edges of the read groups (group size QG: a run-time loop's
last group is clamped and its surplus registers ignored); a routed-wire count that leaves a one-wire last chunk, where the
permutation argument's read-ahead of wire j + 1 has to be clamped because sigma_{routed-1} is the last column of its oracle."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import plonk_verifier as pv
import pymodel as pm
from oracle_lib import P, rand_field

pytestmark = pytest.mark.gpu

DEGREE_BITS, RATE_BITS = 5, 3
# the evaluators' group size, read from the kernel's source so that BaseSum{K}, {K+1} stay on the group edge if it changes
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stark-verifier_amd", "csrc", "quotient.hip")
K = int(re.search(r"constexpr int QG = (\d+);", open(_SRC).read()).group(1))


def _lib():
    return importlib.import_module("stark-verifier_amd._lib")


def gate_set_of_test_gate_set_pointwise():
    lib = _lib()
    gates = [(lib.GATE_POSEIDON, 0), (lib.GATE_ARITHMETIC, 20), (lib.GATE_PUBLIC_INPUT, 0), (lib.GATE_NOOP, 0), (lib.GATE_CONSTANT, 2),
             (lib.GATE_BASE_SUM, 63), (lib.GATE_BASE_SUM, 4), (lib.GATE_BASE_SUM, 20), (lib.GATE_POSEIDON_MDS, 0),
             (lib.GATE_RANDOM_ACCESS, 1 | 20 << 8), (lib.GATE_RANDOM_ACCESS, 4 | 4 << 8 | 2 << 16), (lib.GATE_REDUCING_EXT, 32),
             (lib.GATE_REDUCING, 43), (lib.GATE_ARITHMETIC_EXT, 10), (lib.GATE_MUL_EXT, 13)]
    return dict(gates=gates, groups=[(0, 1), (1, 6), (6, 11), (11, 15)], routed=80, max_degree=8, npp=9, nch=2)


def gate_set_on_group_edges():
    lib = _lib()
    gates = [(lib.GATE_BASE_SUM, 1), (lib.GATE_BASE_SUM, K), (lib.GATE_BASE_SUM, K + 1), (lib.GATE_BASE_SUM, 63),
             (lib.GATE_ARITHMETIC, 1), (lib.GATE_ARITHMETIC_EXT, 1), (lib.GATE_MUL_EXT, 1), (lib.GATE_REDUCING, 1),
             (lib.GATE_REDUCING_EXT, 1), (lib.GATE_CONSTANT, 1), (lib.GATE_RANDOM_ACCESS, 1 | 1 << 8),
             (lib.GATE_RANDOM_ACCESS, 4 | 4 << 8 | 2 << 16), (lib.GATE_POSEIDON_MDS, 0), (lib.GATE_POSEIDON, 0), (lib.GATE_PUBLIC_INPUT, 0)]
    return dict(gates=gates, groups=[(0, 4), (4, 9), (9, 12), (12, 15)], routed=80, max_degree=8, npp=9, nch=2)


def one_wire_last_chunk(nch):
    lib = _lib()
    gates = [(lib.GATE_ARITHMETIC, 3), (lib.GATE_CONSTANT, 2), (lib.GATE_PUBLIC_INPUT, 0), (lib.GATE_NOOP, 0)]
    return dict(gates=gates, groups=[(0, 4)], routed=17, max_degree=8, npp=2, nch=nch)


def check_every_row(gl, ctx, d, seed):
    """gl355_quotient_values == eval_vanishing_poly / Z_H at all N storage rows.  (The big-integer model takes well under 20 s for
    256 points of the largest descriptor, so no row is left out.)"""
    lib = _lib()
    api = importlib.import_module("stark-verifier_amd.api")
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    rng = np.random.default_rng(seed)
    gates, groups, routed, nch, npp = d["gates"], d["groups"], d["routed"], d["nch"], d["npp"]
    assert len(gates) <= 16 and npp == (routed + d["max_degree"] - 1) // d["max_degree"] - 1
    sel_idx = [next(s for s, (lo, hi) in enumerate(groups) if lo <= g < hi) for g in range(len(gates))]
    n, N = 1 << DEGREE_BITS, 1 << (DEGREE_BITS + RATE_BITS)
    n_sel, n_cst, nw = len(groups), d.get("num_constants", 2), d.get("num_wires", 135)
    cs_vals = rand_field(rng, (n_sel + n_cst + routed, n))
    cs_vals[:n_sel] = rng.integers(0, len(gates), size=(n_sel, n)).astype(np.uint64)   # selector-like small values
    cs = gl.PolynomialBatch.from_values(ctx, cs_vals, RATE_BITS, 2)
    wb = gl.PolynomialBatch.from_values(ctx, rand_field(rng, (nw, n)), RATE_BITS, 2)
    zb = gl.PolynomialBatch.from_values(ctx, rand_field(rng, (nch * (1 + npp), n)), RATE_BITS, 2)
    cc = lib.Circuit()
    cc.degree_bits, cc.rate_bits, cc.num_wires, cc.num_routed_wires = DEGREE_BITS, RATE_BITS, nw, routed
    cc.num_constants, cc.num_selectors, cc.num_challenges, cc.max_degree = n_cst, n_sel, nch, d["max_degree"]
    cc.num_partial_products, cc.num_gates = npp, len(gates)
    for i, (t, p) in enumerate(gates):
        cc.gates[i].type, cc.gates[i].param, cc.gates[i].selector_index = t, p, sel_idx[i]
        cc.gates[i].group_start, cc.gates[i].group_end = groups[sel_idx[i]]
    k_is = np.array([pow(7, j, P) for j in range(routed)], dtype=np.uint64)
    betas, gammas, alphas, pi_hash = rand_field(rng, nch), rand_field(rng, nch), rand_field(rng, nch), rand_field(rng, 4)
    vals = np.empty((nch, N), dtype=np.uint64)
    try:
        ctx.check(ctx.lib.gl355_quotient_values(ctx.h, C.byref(cc), cs.h, wb.h, zb.h, api._ptr(k_is), api._ptr(betas), api._ptr(gammas),
                                                api._ptr(alphas), api._ptr(pi_hash), api._ptr(vals)))
    except gl.Gl355Error:
        for o in (cs, wb, zb):
            o.close()
        raise
    cd = dict(degree_bits=DEGREE_BITS, gates=gates, groups=groups, selector_indices=sel_idx, num_selectors=n_sel,
              num_constants=n_cst, num_wires=nw, num_routed_wires=routed, num_challenges=nch, quotient_degree_factor=d["max_degree"],
              num_partial_products=npp, num_gate_constraints=max(plonk._GATE_CONSTRAINTS[t](p) for t, p in gates),
              k_is=[int(k) for k in k_is])
    cs_l, w_l, z_l = cs.leaves(), wb.leaves(), zb.leaves()
    for o in (cs, wb, zb):
        o.close()
    bits = DEGREE_BITS + RATE_BITS
    omega = pm.root_of_unity(bits)
    want = np.empty((nch, N), dtype=np.uint64)
    for t in range(N):
        i = pm.bitrev(t, bits)
        x = 7 * pow(omega, i, P) % P
        t_next = pm.bitrev((i + d["max_degree"]) % N, bits)
        op = dict(constants=[pv.base(v) for v in cs_l[t][:n_sel + n_cst]], plonk_sigmas=[pv.base(v) for v in cs_l[t][n_sel + n_cst:]],
                  wires=[pv.base(v) for v in w_l[t]], plonk_zs=[pv.base(v) for v in z_l[t][:nch]],
                  partial_products=[pv.base(v) for v in z_l[t][nch:]], plonk_zs_next=[pv.base(v) for v in z_l[t_next][:nch]])
        xn = pow(x, n, P)
        van = pv.eval_vanishing_poly(cd, pv.base(x), pv.base(xn), op, [int(v) for v in pi_hash], [int(b) for b in betas],
                                     [int(g) for g in gammas], [int(a) for a in alphas])
        zh_inv = pow((xn - 1) % P, P - 2, P)
        for c in range(nch):
            assert van[c][1] == 0
            want[c][t] = van[c][0] * zh_inv % P
    bad = np.argwhere(vals != want)
    assert bad.size == 0, "%d of %d values differ, first (challenge, storage row) %s" % (len(bad), vals.size, tuple(bad[0]))


def test_every_row_gate_set_of_test_gate_set_pointwise(gl, ctx):
    """the 15 gates of test_gate_set_pointwise (routed 80, 135 wires, 9 partial products), every one of the 256 rows"""
    check_every_row(gl, ctx, gate_set_of_test_gate_set_pointwise(), 0x36A)


def test_every_row_parameters_on_group_edges(gl, ctx):
    """BaseSum{1, K, K+1, 63}, one-operation Arithmetic / ArithmeticExtension / MulExtension / Reducing / ReducingExtension,
    Constant{1}, RandomAccess{bits 1, copies 1} and {bits 4, copies 4, extra 2}, PoseidonMds, Poseidon, PublicInput"""
    check_every_row(gl, ctx, gate_set_on_group_edges(), 0x36B)


@pytest.mark.parametrize("nch", [2, 1])
def test_every_row_one_wire_last_chunk(gl, ctx, nch):
    """17 routed wires in chunks of 8: three chunks, the last holds one wire, and sigma_16 is the last column of the
    constants_sigmas oracle -- the read-ahead past it is clamped; the values must be equal (quotient_kernel<1> shares the code)"""
    check_every_row(gl, ctx, one_wire_last_chunk(nch), 0x36C + nch)


def exact_fit_at_48_wires():
    lib = _lib()
    gates = [(lib.GATE_POSEIDON_MDS, 0), (lib.GATE_ARITHMETIC, 12), (lib.GATE_ARITHMETIC_EXT, 6), (lib.GATE_MUL_EXT, 8), (lib.GATE_REDUCING_EXT, 11),
             (lib.GATE_BASE_SUM, 47), (lib.GATE_RANDOM_ACCESS, 2 | 6 << 8), (lib.GATE_REDUCING, 14), (lib.GATE_CONSTANT, 2),
             (lib.GATE_PUBLIC_INPUT, 0), (lib.GATE_NOOP, 0)]
    return dict(gates=gates, groups=[(0, 3), (3, 7), (7, 11)], routed=40, max_degree=8, npp=4, nch=2, num_wires=48)


def test_every_row_exact_fit_at_48_wires(gl, ctx):
    """a wires oracle of exactly 48 columns: PoseidonMds, Arithmetic{12}, ArithmeticExtension{6}, MulExtension{8}, ReducingExtension{11},
    BaseSum{47} and RandomAccess{bits 2, copies 6} (36 routed wires + 12 bit wires) each read wire 47 and none beyond; Reducing{14}
    reads 46, Constant{2} both gate constants.  The smallest descriptor at which the launcher's check (csrc/gate_shape.h) and the
    evaluators meet: every one of the 256 rows"""
    check_every_row(gl, ctx, exact_fit_at_48_wires(), 0x370)


@pytest.mark.parametrize("gate,num_constants", [("CONSTANT", 2), ("ARITHMETIC", 1)], ids=["Constant{3} with two constants", "Arithmetic{1} with one"])
def test_gates_that_read_more_constants_than_the_circuit_has_are_refused(gl, ctx, gate, num_constants):
    """unchecked, the evaluator would take a sigma column of the same oracle for a gate constant (in bounds, and wrong); the
    descriptor check refuses with GL355_E_INVALID_ARG before anything is launched"""
    lib = _lib()
    gates = [(lib.GATE_CONSTANT, 3) if gate == "CONSTANT" else (lib.GATE_ARITHMETIC, 1), (lib.GATE_NOOP, 0)]
    d = dict(gates=gates, groups=[(0, 2)], routed=17, max_degree=8, npp=2, nch=2, num_constants=num_constants)
    with pytest.raises(gl.Gl355Error, match="does not fit") as ei:
        check_every_row(gl, ctx, d, 0x371)
    assert ei.value.code == -1 and "gate 0" in str(ei.value)


@pytest.mark.parametrize("bits", [0, 5])
def test_random_access_bits_outside_1_to_4_are_refused(gl, ctx, bits):
    """the evaluator holds a copy's bit wires in four registers and its list in sixteen: other parameters are an error at launch,
    not a read of a column the gate does not own"""
    lib = _lib()
    d = dict(gates=[(lib.GATE_RANDOM_ACCESS, bits | 1 << 8), (lib.GATE_NOOP, 0)], groups=[(0, 2)], routed=17, max_degree=8, npp=2, nch=2)
    with pytest.raises(gl.Gl355Error, match="RandomAccessGate"):
        check_every_row(gl, ctx, d, 0x36F)
