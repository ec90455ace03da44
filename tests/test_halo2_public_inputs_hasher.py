"""CPU: PublicInputsHasherChip (halo2_plonk_chips.py) and the constants poseidon_spec.py derives for it.  The chip's hash must be plonky2's
hash_no_pad, one permutation the oracle's permutation, and the sparse form of the partial rounds must agree with the 30 dense rounds (which
locates a wrong constant: the dense rounds use the round constants and the MDS matrix only)."""
import numpy as np
import pytest

import halo2_verifier_cases as hv

hg, hp, ps, P, K = hv.hg, hv.hp, hv.ps, hv.P, hv.K


@pytest.mark.parametrize("n", hv.HASH_LENGTHS)
def test_hash_equals_hash_no_pad(orc, n):
    rec, out, marks = hv.hasher_case(n)
    words = hv.hasher_inputs(n)
    assert n < 3 or (0 in words and P - 1 in words)
    assert [c.value for c in out] == [int(v) for v in orc.hash_no_pad(np.array(words, dtype=np.uint64))]
    assert len(marks) == (n + 7) // 8
    if n:
        hv.accepted(rec)
    else:                                                            # no input, no permutation: four constant zeros and no row for the mock model to visit
        advice, status = hg.synthesize_host(rec.tape(), rec.k, np.zeros(0, dtype=np.uint64))
        assert status == rec.status() == (hg.NO_FAILURE, 0) and np.array_equal(advice, rec.advice())


def test_one_permutation_equals_the_oracle(orc):
    rng = np.random.default_rng(0x9E2)
    state = [int(v) for v in hv.rand_field(rng, 12)]
    state[3], state[7] = 0, P - 1
    rec = hg.Recorder(K, state)
    g = hg.GoldilocksChip(rec)
    g.load_table()
    chip = hp.PublicInputsHasherChip(rec)
    out = chip.permute([g.assign_value(hg.Input(i)) for i in range(12)], 8)
    want = [int(v) for v in orc.permute(np.array(state, dtype=np.uint64))]
    assert [c.value for c in chip.state] == want and [c.value for c in out] == want[:8]
    hv.accepted(rec)


def test_sparse_form_equals_the_dense_rounds():
    rng = np.random.default_rng(0x5BA)
    for state in ([int(v) for v in hv.rand_field(rng, 12)], [0] * 12, [P - 1] * 12):
        assert ps.permute_optimized(state) == ps.permute_dense(state)
    sp = ps.optimized_spec()
    assert len(sp["start"]) == 5 and len(sp["partial"]) == 22 == len(sp["sparse"]) and len(sp["end"]) == 3
    assert all(len(row) == 12 and len(col_hat) == 11 for row, col_hat in sp["sparse"])


def test_fast_partial_tables_equal_the_golden_file():
    """PoseidonGate's constants come from the package: they are the numbers tests/golden holds"""
    import json
    import os
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon_fast_partial_tables.json")))
    tb = ps.fast_partial_tables()
    num = lambda name: [int(x, 16) for x in golden[name]]      # noqa: E731
    flat = lambda rows: [x for row in rows for x in row]      # noqa: E731
    assert num("FAST_PARTIAL_FIRST_ROUND_CONSTANT") == tb["first"] and num("FAST_PARTIAL_ROUND_CONSTANTS") == tb["post"]
    assert num("FAST_PARTIAL_ROUND_VS") == flat(tb["vs"]) and num("FAST_PARTIAL_ROUND_W_HATS") == flat(tb["w_hats"])
    assert num("FAST_PARTIAL_ROUND_INITIAL_MATRIX") == flat(tb["init"])


def test_only_the_first_permutation_interleaves_constants():
    """rows and levels of the second and the third permutation are the same; the first has the constant rows (assign_constant caches) on top.
    24 inputs, so that the second and the third permutation both take eight fresh words: a word's level is 1 + its operands', and
    compose walks its 12 terms in order, so a permutation that overwrites only ONE word (the third of 17 inputs) is a few levels deeper
    than one that overwrites eight -- the figures of both are printed"""
    for n in (17, 24):
        rec, _, marks = hv.hasher_case(n)
        assert len(marks) == 3
        (r1, l1), (r2, l2), (r3, l3) = marks
        start = next(e[3] for e in rec.entries if e[2] == hg.OP_MULADD)
        print("%d inputs: rows per permutation %d, %d, %d; levels per permutation %d, %d, %d" % (n, r1 - start, r2 - r1, r3 - r2, l1 - 1, l2 - l1, l3 - l2))
        assert r3 - r2 == r2 - r1 < r1 - start
    assert l3 - l2 == l2 - l1
