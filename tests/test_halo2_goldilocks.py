"""CPU: the recorder of the reference's Goldilocks chips (stark-verifier_amd/halo2_goldilocks.py) -- eager values against plain arithmetic and the
BN254-Poseidon model, the recorded (layout, witness) against the tree-evaluating MockProver model, the offset logic of AllChip::permute, and
the artifact round trip.

The mock model is run on every row with a selector on and the rows whose gates read them (all other rows have every selector off, every gate
polynomial identically zero and every lookup input zero: unassigned advice is zero and 0 is in the table); copy constraints are checked in
full.  At k = 17 that is a few hundred of 131 072 rows per case; the fraction is printed."""
import numpy as np
import pytest

import halo2_synth_cases as cs
import pymodel_bn254 as pm
from halo2_mock_model import GATE, PERMUTATION, MockModel

hg, h2, P, K = cs.hg, cs.h2, cs.P, cs.K
RANGE_TABLE = {(v,) for v in range(1 << 16)}


def mock_failures(rec, advice=None, model_copies=False):
    """the mock model's complete list.  Gates and lookups: the model itself on the rows named above.  Copy constraints: the model's rule
    vectorised (cs.copy_failures; the model's own loop over all 7 x 2^17 cells takes seconds), or the model's loop with model_copies=True --
    test_mock_model_sees_a_changed_cell holds the two against each other."""
    lay = rec.layout()
    fixed, mapping = lay.fixed_array(), lay.mapping_array()
    advice = rec.advice() if advice is None else advice
    model = MockModel(lay.cs, K, cs.LazyColumns(fixed), mapping if model_copies else None)
    rows = model.readers(cs.selector_rows(rec))
    print("mock model: %d of %d rows evaluated (every row with a selector on, and their readers)" % (len(rows), model.usable))
    out = model.verify(cs.LazyColumns(advice), [rec.instance], rows=rows, tables=[RANGE_TABLE] * len(lay.cs.lookups))
    return out if model_copies else sorted(out + cs.copy_failures(lay.cs, mapping, advice, fixed, rec.instance))


def test_arithmetic_values_and_mock_model():
    rec, out = cs.arithmetic_case()
    x, m2 = rec.inputs[3], rec.inputs[4]
    v = lambda c: c.value        # noqa: E731
    assert v(out["add"]) == (2 * (P - 1)) % P and v(out["sub"]) == P - 1
    assert v(out["mul_max"]) == ((P - 1) ** 2 + P - 1) % P and v(out["mul"]) == x * m2 % P
    assert v(out["mul_with_constant"]) == x * 2 * (P - 1) % P and v(out["add_constant"]) == 0
    q_ext = (8 * (P - 1) ** 2 + P - 1) // P
    assert q_ext >> 64, "the case is meant to need q's fifth limb"
    assert [v(c) for c in out["ext_max"]] == [(8 * (P - 1) ** 2 + P - 1) % P, (2 * (P - 1) ** 2 + P - 1) % P]
    assert rec.values[(rec.ar.q_limbs[4].index, out["ext_max"][0].row)] == q_ext >> 64
    assert [v(c) for c in out["ext"]] == [(x * 3 + 7 * 2 * 5 + 1) % P, (x * 5 + 2 * 3) % P]
    assert v(out["select1"]) == x and v(out["select0"]) == m2
    assert (v(out["is_zero_0"]), v(out["is_zero_x"]), v(out["is_equal"]), v(out["is_not_equal"])) == (1, 0, 1, 0)
    assert [v(b) for b in out["bits"]] == [((P - 1) >> i) & 1 for i in range(64)]
    assert v(out["from_bits"]) == (P - 1) & ((1 << 40) - 1)
    assert v(out["exp2"]) == pow(x, 32, P) and v(out["exp_bits"]) == pow(7, 5, P)
    assert v(out["compose"]) == (11 + x * 3 + (P - 1) * (P - 1)) % P
    assert v(out["packed"]) == 1 * P + (P - 1) * P * P and [v(c) for c in out["unpacked"]] == [0, 1, P - 1]
    # unpack works in base p (goldilocks_decompose, utils.rs:25-36): a scalar whose 64-bit pieces include one >= p has three digits below p like any
    # other and never fails; the fourth digit is assigned and range-checked but not returned
    assert [v(c) for c in out["unpacked_wide"]] == [cs.WIDE_FR % P, cs.WIDE_FR // P % P, cs.WIDE_FR // P ** 2 % P]
    assert v(out["access_first"]) == x and v(out["access_last"]) == 3
    assert rec.instance == [x * m2 % P, 3]
    assert rec.status() == (hg.NO_FAILURE, 0)
    assert mock_failures(rec) == []


def test_mock_model_sees_a_changed_cell():
    """the restricted model is not vacuous: one r cell changed breaks its row's gates and its copy constraints"""
    rec, out = cs.arithmetic_case()
    adv = rec.advice()
    cell = out["mul"]
    adv[cell.col, cell.row, 0] ^= np.uint64(1)
    fails = mock_failures(rec, adv)
    assert any(f[0] == GATE and f[2] == cell.row for f in fails) and any(f[0] == PERMUTATION for f in fails)
    assert fails == mock_failures(rec, adv, model_copies=True)


def test_value_not_below_p_fails_at_its_entry():
    rec = cs.failing_value_case()
    first, count = rec.status()
    assert count == 2 and rec.entry_rows(first) == (1, 1)       # the second assign_value row
    fails = mock_failures(rec)
    # row 1 (r = 2^64 - 1): q = p - r holds in the scalar field, but q is then not the sum of its five 16-bit limbs: "limb decomposition" fails.
    # row 2 (r = p exactly): q = 0 and every constraint of the reference's gate set holds (it admits r <= p); the tape's status still names it
    assert sorted({f[2] for f in fails if f[0] == GATE}) == [1]


def test_assert_equal_on_differing_values():
    rec = cs.failing_assert_case()
    first, count = rec.status()
    assert count == 2
    tape = rec.tape().reshape(-1, 8)
    assert int(tape[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    fails = mock_failures(rec)
    assert fails and all(f[0] == PERMUTATION for f in fails)


def test_permute_values_and_offsets():
    rec, runs = cs.permute_case()
    for state, out, before, after in runs:
        assert [c.value for c in out] == pm.permute(state)
        # all_chip.rs:74-87: the 69 Poseidon rows start where the pack rows start; the arithmetic rows are 4 packs of 3 rows and 4 unpacks of 8
        # (every constant is registered by then), so the offset continues at the larger of the two ends
        assert after - before == max(4 * 3 + 4 * 8, 69)
    assert mock_failures(rec) == []


def test_permute_offset_with_constants_assigned_inside():
    """the first permute of a region also assigns its constants (0, 1, p, p^2, p^3) among the pack / unpack rows: the same max(), other numbers"""
    rec = hg.Recorder(K, list(range(12)))
    g = hg.GoldilocksChip(rec)
    cells = [g.assign_value(hg.Input(i)) for i in range(12)]
    before = rec.offset
    g.all_chip.permute(cells)
    n_const = len(rec.constants)
    assert n_const == 5 and rec.offset - before == max(1 + 4 * 3 + 4 + 4 * 8, 1 + 69)     # the zero is assigned before the Poseidon rows start


def test_level_major_tape():
    rec, _ = cs.arithmetic_case()
    tape = rec.tape().reshape(-1, 8)
    levels = (tape[:, 0] >> np.uint64(8)).astype(np.int64)
    assert levels[0] == 1 and (np.diff(levels) >= 0).all() and set(np.diff(levels)) <= {0, 1}
    assert sum(rec.level_widths()) == len(tape)


def test_artifact_round_trip(tmp_path):
    rec, _ = cs.permute_case()
    art = rec.artifact()
    path = str(tmp_path / "layout.npz")
    art.save(path)
    back = hg.Artifact.load(path)
    assert back.digest() == art.digest()
    assert np.array_equal(back.tape, art.tape) and back.layout.rows_used == rec.rows_used
    assert np.array_equal(back.layout.fixed_array(), art.layout.fixed_array()) and np.array_equal(back.layout.mapping_array(), art.layout.mapping_array())
    raw = bytearray(open(path, "rb").read())
    # a byte inside the stored tape (np.savez stores uncompressed): the digest no longer matches, or the container itself is refused
    pos = raw.find(art.tape.tobytes()[:64])
    assert pos > 0
    raw[pos + 9] ^= 0x40
    bad = str(tmp_path / "bad.npz")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        hg.Artifact.load(bad)
