"""CPU: GoldilocksExtensionChip (halo2_goldilocks.py) and the tape's INV_EXT operand.  Every method on operands that include 0, 1, p - 1,
(0, y1) and (y0, 0): the eager values equal pymodel's extension arithmetic, the host replay equals the recorder cell for cell with no failing
entry, and the mock model accepts every row and copy constraint.  A division by (0, 0) fails the ASSERT_EQ of y y_inv = 1 with its rows
written; the validator refuses an INV_EXT that reads ahead, names a third component, or sits in a MULADD."""
import numpy as np
import pytest

import halo2_fri_cases as fc
import plonk_verifier as pv
import pymodel as pm
from test_halo2_goldilocks import mock_failures

hg, P, K = fc.hg, fc.P, fc.K
add, sub, mul, base = pv.add, pv.sub, pv.mul, pv.base


def expected(method, args):
    if method == "mul_add":
        return add(mul(args[0], args[1]), args[2])
    if method == "add":
        return add(*args)
    if method == "sub":
        return sub(*args)
    if method == "mul":
        return mul(*args)
    if method == "mul_sub":
        return sub(mul(args[0], args[1]), args[2])
    if method == "square":
        return mul(args[0], args[0])
    if method == "scalar_mul":
        return mul(args[0], base(args[1]))
    if method == "arithmetic":
        c0, c1, a, b, c = args
        return add(mul(base(c0), mul(a, b)), mul(base(c1), c))
    if method == "mul_with_const":
        return mul(base(args[0]), mul(args[1], args[2]))
    if method == "select":
        cond, a, b = args
        return add(mul(cond, sub(a, b)), b)
    if method == "exp2":
        return pv.ext_pow(args[0], 1 << args[1])
    if method == "convert":
        return base(args[0])
    if method == "div":
        return mul(args[0], pm.ext_inv(args[1]))
    if method == "div_add":
        return add(mul(args[0], pm.ext_inv(args[1])), args[2])
    if method == "exp":
        return pv.ext_pow(*args)
    if method == "shift":
        return mul(pv.ext_pow(args[0], args[1]), args[2])
    if method == "mul_many":
        acc = pv.E1
        for t in args:
            acc = mul(acc, t)
        return acc
    if method == "reduce":
        return pv.reduce_with_powers(args[1], args[0])
    if method == "reduce_base_terms":
        return pv.reduce_with_powers([base(t) for t in args[1]], args[0])
    if method == "reduce_base":
        return pv.reduce_with_powers(args[1], base(args[0]))
    return {"zero": (0, 0), "one": (1, 0), "two": (2, 0)}.get(method) or tuple(args[0])


def test_every_method_equals_the_extension_arithmetic():
    rec, out = fc.extension_case()
    seen = set()
    for method, args, cells in out:
        seen.add(method)
        want = expected(method, args)
        assert (cells[0].value, cells[1].value) == (want[0] % P, want[1] % P), (method, args)
    assert len(seen) == 24 and sum(1 for m, a, _ in out if m == "exp") == 4
    assert sorted(len(a[1]) for m, a, _ in out if m == "reduce") == [0, 1, 3]


def test_ext_inverse_is_the_inverse():
    for y in [(1, 0), (0, 1), (P - 1, P - 1), (0, 5), (7, 0), (0x123456789ABCDEF, P - 2)]:
        assert hg.ext_inverse(*y) == pm.ext_inv(y) and mul(y, hg.ext_inverse(*y)) == (1, 0)
    assert hg.ext_inverse(0, 0) == (0, 0)


def test_host_replay_and_mock_model():
    rec, _ = fc.extension_case()
    assert rec.status() == (hg.NO_FAILURE, 0)
    advice, status = hg.synthesize_host(rec.tape(), K, rec.inputs)
    assert status == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert mock_failures(rec, advice) == []


def test_division_by_zero_fails_the_assert_with_its_rows_written():
    rec, q = fc.zero_divisor_case()
    tape = rec.tape().reshape(-1, 8)
    first, count = rec.status()
    assert count >= 1 and int(tape[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    advice, status = hg.synthesize_host(rec.tape(), K, rec.inputs)
    assert status == rec.status()
    assert np.array_equal(advice, rec.advice())
    assert (q[0].value, q[1].value) == (0, 0) and rec.rows_used > q[1].row
    assert mock_failures(rec, advice) != []          # the copy constraint of assert_one is what the circuit refuses


def inv_ext_entry(tape):
    t = tape.reshape(-1, 8)
    return next(i for i in range(len(t)) if int(t[i, 0]) & 0xFF == hg.OP_VALUE and int(t[i, 2]) >> 60 == hg.K_INV_EXT)


def refused(tape, rec):
    from importlib import import_module
    lib = import_module("stark-verifier_amd._lib")
    with pytest.raises(lib.Gl355Error):
        hg.synthesize_host(tape.reshape(-1), K, rec.inputs)


def test_validator_refuses_a_misused_inv_ext():
    rec, _ = fc.zero_divisor_case()
    good = rec.tape().reshape(-1, 8)
    i = inv_ext_entry(good)
    hg.synthesize_host(good.reshape(-1), K, rec.inputs)          # the tape itself loads
    level = int(good[i, 0]) >> 8
    for later in (level, level + 1):                             # the second cell written at the same or a later level
        j = next(j for j in range(len(good)) if int(good[j, 0]) >> 8 == later and int(good[j, 0]) & 0xFF in (hg.OP_MULADD, hg.OP_MULADD_EXT, hg.OP_VALUE) and j != i)
        t = good.copy()
        t[i, 3] = (hg.K_CELL << 60) | (rec.ar.r.index << 40) | int(good[j, 1])
        refused(t, rec)
    t = good.copy()
    t[i, 2] = (int(t[i, 2]) & ~(0xFF << 48)) | (2 << 48)         # aux = 2
    refused(t, rec)
    t = good.copy()
    j = next(j for j in range(len(good)) if int(good[j, 0]) & 0xFF == hg.OP_MULADD and int(good[j, 0]) >> 8 > level)
    t[j, 2] = good[i, 2]                                         # the kind in a MULADD
    refused(t, rec)
    t = good.copy()
    t[i, 3] = (hg.K_INPUT << 60) | 0                             # the second operand must be a cell
    refused(t, rec)
