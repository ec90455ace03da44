"""CPU: gl355_halo2_synthesize_host (csrc/halo2_synth_host.cpp) against the recorder's eager values, cell for cell, on every shared case
(halo2_synth_cases.py); the status of the failing cases; Merkle proofs under the oracle's BN254-Poseidon hasher; tape validation."""
import importlib

import numpy as np
import pytest

import halo2_synth_cases as cs
from halo2_mock_model import PERMUTATION
from oracle_lib import Bn254Oracle
from test_halo2_goldilocks import mock_failures

hg, P, K = cs.hg, cs.P, cs.K


def replay(rec):
    advice, status = hg.synthesize_host(rec.tape(), K, rec.inputs)
    assert status == rec.status()
    want = rec.advice()
    if not np.array_equal(advice, want):
        col, row = np.argwhere((advice != want).any(axis=2))[0]
        raise AssertionError("host replay differs from the recorder at advice column %d row %d" % (col, row))
    return status


@pytest.mark.parametrize("case", ["arithmetic_case", "permute_case", "deep_case", "wide_case"])
def test_host_replay_equals_recorder(case):
    rec = getattr(cs, case)()[0]
    assert replay(rec) == (hg.NO_FAILURE, 0)


def test_host_replay_failing_value():
    rec = cs.failing_value_case()
    first, count = replay(rec)
    assert (first, count) == (1, 2)
    tape = rec.tape().reshape(-1, 8)
    assert int(tape[first, 0]) & 0xFF == hg.OP_VALUE and int(tape[first, 2]) == (hg.K_INPUT << 60) | 1


def test_host_replay_failing_assert():
    rec = cs.failing_assert_case()
    first, count = replay(rec)
    assert count == 2 and int(rec.tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


@pytest.fixture(scope="module")
def bn(orc):
    return Bn254Oracle(orc)


@pytest.mark.parametrize("depth,leaf_len,index", [(3, 9, 5), (3, 4, 2), (0, 4, 1)])
def test_merkle_proof_valid(bn, depth, leaf_len, index):
    rec = cs.merkle_case(bn, depth, leaf_len, index)
    assert replay(rec) == (hg.NO_FAILURE, 0)
    assert mock_failures(rec) == []


@pytest.mark.parametrize("depth,leaf_len,index,mutate", [(3, 9, 5, "sibling"), (3, 9, 5, "cap_index"), (0, 4, 1, "sibling"), (0, 4, 1, "cap_index")])
def test_merkle_proof_invalid(bn, depth, leaf_len, index, mutate):
    rec = cs.merkle_case(bn, depth, leaf_len, index, mutate)
    first, count = replay(rec)
    assert count >= 1
    tape = rec.tape().reshape(-1, 8)
    assert int(tape[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    # the failing entries are exactly the final comparisons of the cap entry with the computed root; the mock model names the same cells' copy constraints
    bad = [i for i, e in enumerate(rec._sorted()) if e[5]]
    cells = set()
    for i in bad:
        for w in tape[i, 2:4]:
            cells.add(((int(w) >> 40) & 0xFF, int(w) & 0xFFFFFFFFFF))
    fails = mock_failures(rec)
    assert fails and all(f[0] == PERMUTATION for f in fails)
    perm = rec.cs.permutation
    named = {(perm[f[1]].index, f[2]) for f in fails if perm[f[1]].kind == cs.h2.ADVICE}
    assert cells <= named


def _tape_of_two():
    rec = hg.Recorder(K, [3, 4])
    g = hg.GoldilocksChip(rec)
    a = g.assign_value(hg.Input(0))
    b = g.assign_value(hg.Input(1))
    g.mul_add(a, b, a)
    return rec


def _rc(tape, n_inputs, inputs):
    lib = importlib.import_module("stark-verifier_amd")._lib.load()
    tape = np.ascontiguousarray(tape, dtype=np.uint64)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
    advice = np.zeros((hg.N_ADVICE, 1 << K, 4), dtype=np.uint64)
    status = np.zeros(2, dtype=np.uint64)
    return lib.gl355_halo2_synthesize_host(tape.ctypes.data, tape.size, n_inputs, K, hg.N_ADVICE, inputs.ctypes.data, advice.ctypes.data, status.ctypes.data)


def test_tape_validation():
    rec = _tape_of_two()
    good = rec.tape()
    assert _rc(good, 2, rec.inputs) == 0
    t = good.reshape(-1, 8).copy()
    # a forward reference: the first VALUE takes the MULADD's r cell (a later level) as its operand
    fwd = t.copy()
    fwd[0, 2] = (hg.K_CELL << 60) | (rec.ar.r.index << 40) | 2
    assert _rc(fwd.reshape(-1), 2, rec.inputs) == -1
    # a row out of range, an operand row out of range, an input index out of range
    for (i, j, v) in ((2, 1, 1 << K), (2, 2, (hg.K_CELL << 60) | (rec.ar.r.index << 40) | (1 << K)), (1, 2, (hg.K_INPUT << 60) | 2)):
        bad = t.copy()
        bad[i, j] = v
        assert _rc(bad.reshape(-1), 2, rec.inputs) == -1
    # truncated, an unknown op, the same cell written twice, a level that is not above its operand's
    assert _rc(good[:-3], 2, rec.inputs) == -1
    bad = t.copy(); bad[2, 0] = 99 | (2 << 8)
    assert _rc(bad.reshape(-1), 2, rec.inputs) == -1
    bad = t.copy(); bad[1, 1] = 0
    assert _rc(bad.reshape(-1), 2, rec.inputs) == -1
    bad = t.copy(); bad[2, 0] = hg.OP_MULADD | (1 << 8)
    assert _rc(bad.reshape(-1), 2, rec.inputs) == -1
    with pytest.raises(Exception):
        hg.synthesize_host(good[:-3], K, rec.inputs)
