"""CPU: the plain-integer restatement of the BN254 limb arithmetic (tests/pymodel_bn254_limbs.py) and its operand generators, which
tests/test_gpu_bn254_arith.py drives the device functions with -- the restatement computes what the comments say, the generators reach every
boundary they are there for, and the test hooks refuse without a device or context by an error code."""
import os
import re

import numpy as np
import pytest

import pymodel_bn254_limbs as pl
from pymodel_bn254_limbs import Q, R256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stark-verifier_amd", "csrc")


def header_words(name, path):
    src = open(os.path.join(CSRC, path)).read()
    m = re.search(r"\b%s\b\s*(?:\[\d*\]\s*=\s*\{|,)([^)}]*)" % name, src)
    return [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",") if w.strip()]


@pytest.mark.parametrize("f", ["fr", "fq"])
def test_cios_restatement_is_montgomery_product(f):
    m = pl.MOD[f]
    vals = pl.edge8(f)
    core = [0, 1, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1] + vals[::97]
    st = pl.new_stats()
    n = 0
    for a in core:
        for b in vals[::7]:
            r = pl.cios(a, b, f, st)
            assert r < 2 * m and (r * R256 - a * b) % m == 0                # a b R^-1, below 2m: "4 m < R" needs no final subtraction
            n += 1
    assert n > 5000
    # the rare events: results in [m, 2m) are common at the edges; the ninth-word carry and the top carry of the reduction half-row never
    # fire below 2m (the row sum stays under 2^288 because a < 2m < 2^255), which is why the device form may drop them
    assert st["ge_m"] > 500
    assert st["t9"] == 0 and st["red_top"] == 0
    big = pl.new_stats()
    for a in (R256 - 1, R256 - 2, R256 - (1 << 32)):
        for b in (R256 - 1, R256 - (1 << 224)):
            pl.cios(a, b, f, big)
    assert big["red_top"] > 0                                              # outside the domain the top carry is real: the bound is what matters


@pytest.mark.parametrize("f", ["fr", "fq"])
def test_generators_reach_the_boundaries(f):
    m = pl.MOD[f]
    vals = pl.edge8(f)
    assert all(0 <= v < 2 * m for v in vals) and {0, 1, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1} <= set(vals)
    assert len(vals) > 700
    assert sum(1 for k in range(254) if (1 << k) - 1 in vals and (1 << k) + 1 in vals) >= 250
    assert any(v == 2 * m - 1 for v in vals) and any(v & 0xFFFFFFFF == 0xFFFFFFFF and v > m for v in vals)
    pairs_2m = sum(1 for v in vals if 2 * m - v in vals)
    assert pairs_2m >= 100                                                  # sums of exactly 2m: where >= and > differ
    ints = pl.from_int_edges(f)
    assert max(ints) == R256 - 1
    for k in range(6):
        assert k * m + 1 in ints
    assert sum(1 for v in ints if v >= 5 * m) >= 4                          # inputs that need the fifth conditional subtraction
    for v in ints:
        assert pl.m_from_int(v, f) == pl.cios(v % m, R256 * R256 % m, f)


def test_lent_constants_match_the_header():
    for k in (2, 4, 8, 16):
        assert header_words("FQ29_C%d" % k, "bn254_f29.cuh") == pl.lent(k)
    assert header_words("FQ29_Q", "bn254_f29.cuh") == pl.pack29(Q)
    assert header_words("FR29_R", "bn254_f29.cuh") == pl.pack29(pl.R)


def test_f29_restatement_and_its_columns():
    normal = pl.f29_normal_values()
    assert max(normal) >= 11 * Q and any(pl.below(v, 12) and v > 11 * Q for v in normal)
    lazy = pl.lazy_first_operands()
    assert all(max(x[:8]) < 2 ** 30.6 for x in lazy) and max(max(x[:8]) for x in lazy) > 2 ** 30.4
    worst = 0
    for f in ("fq", "fr"):
        for a in lazy + [pl.pack29(v) for v in normal[::3]]:
            for bv in normal[::5] + [R256 - 1, sum(pl.M29 << (29 * j) for j in range(9))]:
                b = pl.pack29(bv)
                r, top = pl.f29_mul_mod(a, b, f)
                worst = max(worst, top)
                assert pl.f29_mul_ok(a, b, r, f)
    assert worst < 1 << 64                                                   # the 64-bit column accumulators never overflow
    assert worst > 1 << 62                                                   # ... and the operands pushed them near the edge
    for k in (2, 4, 8, 16):
        subs = pl.subtrahends(k)
        assert k * Q - 1 in subs and all(v < k * Q for v in subs)
        assert any(pl.pack29(v)[:8] == [pl.M29] * 8 for v in subs)           # every low limb at 2^29 - 1
        C = pl.lent(k)
        assert all(C[j] >= pl.pack29(v)[j] for v in subs for j in range(8))       # the low limbs never borrow
        # the top limb can: C_k lends 1 from it, so a subtrahend in the last 2^232 below k q has a top limb one above C's, and f29_sub's
        # top limb is then one less than a's -- negative for a top limb of 0 (bn254_f29.cuh states the condition at f29_sub)
        assert any(pl.pack29(v)[8] == C[8] + 1 for v in subs)


def test_hooks_refuse_without_a_context(gl):
    lib = gl._lib.load()
    a = np.zeros((4, 9), dtype=np.uint32)
    out = np.zeros((4, 9), dtype=np.uint32)
    assert lib.gl355_bn254_arith_batch(None, pl.M_MUL, a.ctypes.data, a.ctypes.data, out.ctypes.data, 4) == -1     # GL355_E_INVALID_ARG
    ops = np.zeros((1, pl.OPND_WORDS), dtype=np.uint32)
    steps = np.zeros((1, 2), dtype=np.uint32)
    tr = np.zeros((1, 2, pl.REC_WORDS), dtype=np.uint32)
    assert lib.gl355_bn254_g1_chain(None, pl.CHAIN_XYZZ, ops.ctypes.data, 1, steps.ctypes.data, 1, 2, tr.ctypes.data) == -1
    assert not out.any() and not tr.any()


def test_no_device_is_an_error_code(gl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gl.Gl355Error):
        gl.Context(0)
