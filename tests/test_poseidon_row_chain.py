"""CPU: the chained MDS / block rows (csrc/poseidon.cuh psd_mds_rows, psd_b3_dot; tools/gen_poseidon_tables.py chained_row): the high chain starts
from (al >> 32) + c_hi as one 32-bit word, so the row's value is al_0 + ah' 2^32 and no add-with-carry joins the chains.  Checked here: the
precondition c_hi + (worst al >> 32) < 2^32 for all 360 + 98 constants, the chained row against the naive row on all-ones words and non-canonical
inputs, and the accumulator bounds after the change."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_tables as gpt  # noqa: E402

P = gpt.P
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
EPS = M32


@pytest.fixture(scope="module")
def rc():
    return gpt.load_rc()


@pytest.fixture(scope="module")
def bt(rc):
    return gpt.b3_tables(rc)


def test_start_word_fits_32_bits_for_every_constant(rc, bt):
    assert sum(len(r) for r in rc) == 360 and len(bt["add"]) == 98
    assert gpt.DENSE_ROW_SUM == 264 == max(sum(r) for r in gpt.mds_matrix())
    # restated from the definition, not through the generator's helper: every constant under the worst low chain of its own row
    for row in rc:
        for c in row:
            assert (c >> 32) + (((c & M32) + 264 * M32) >> 32) <= M32
    worst = None
    for blk in range(gpt.B3_BLOCKS):
        for j, coef in enumerate(bt["rows"]):
            c = bt["add"][14 * blk + j]
            room = (1 << 32) - ((c >> 32) + (((c & M32) + sum(coef) * M32) >> 32))
            assert room >= 1, (blk, j)
            worst = min(worst, (room, blk, j)) if worst else (room, blk, j)
    dense_room, block_room, where = gpt.chain_preconditions(rc, bt)
    assert max(c >> 32 for row in rc for c in row) == 0xfeed4db6 and dense_room == (1 << 32) - 0xfeed4db6 - 264
    assert (block_room,) + where == worst
    print("room left in the start word: dense %d, block rows %d (block %d, row %d)" % ((dense_room, block_room) + where))


def test_block_row_accumulator_bound(bt):
    # ah' = start + sum coef hi_j with start < 2^32: below 2^57 for the block rows, below 2^44 + 2^32 for the dense rows
    assert gpt.B3_CHAIN_BOUND == 1 << 57
    assert M32 + bt["max_row_sum"] * M32 < (1 << 57)
    assert M32 + 264 * M32 < (1 << 44) + (1 << 32)
    # and the fold's contract: the top word times EPS plus any 64-bit word wraps at most once, the repayment never
    top = (M32 + bt["max_row_sum"] * M32) >> 32
    assert M64 + top * EPS - (1 << 64) + EPS < (1 << 64)


def word_states():
    rnd = random.Random(0xC4A1)
    fixed = [0, M64, P - 1, P, EPS, EPS << 32, M32 << 32 | M32, 1 << 32, (1 << 32) - 1]
    out = [[v] * 12 for v in fixed]
    for _ in range(400):
        out.append([rnd.choice(fixed) if rnd.random() < 0.5 else rnd.randrange(1 << 64) for _ in range(12)])
    return out


def test_chained_dense_row_equals_naive_row(rc):
    m = gpt.mds_matrix()
    n = 0
    for st in word_states():
        for r in range(12):
            for c in (rc[1][r], rc[13][r], rc[29][r], 0, max(x for row in rc for x in row)):
                got, carry, ahp = gpt.chained_row(m[r], st, c, (1 << 44) + (1 << 32))
                assert carry <= 264
                assert got % P == (c + sum(k * v for k, v in zip(m[r], st))) % P
                n += 1
    assert n > 20000


def test_chained_block_row_equals_naive_row(rc, bt):
    rnd = random.Random(0xC4A2)
    for st in word_states()[:120]:
        blk = rnd.randrange(gpt.B3_BLOCKS)
        for j, coef in enumerate(bt["rows"]):
            terms = (st + [rnd.randrange(1 << 64) for _ in range(3)])[:len(coef)]
            c = bt["add"][14 * blk + j]
            got, _, ahp = gpt.chained_row(coef, terms, c, gpt.B3_CHAIN_BOUND)
            assert got % P == (c + sum(k * v for k, v in zip(coef, terms))) % P
    # the tightest row under all-ones words: the start word reaches its largest value
    _, _, (blk, j) = gpt.chain_preconditions(rc, bt)
    coef, c = bt["rows"][j], bt["add"][14 * blk + j]
    got, carry, _ = gpt.chained_row(coef, [M64] * len(coef), c, gpt.B3_CHAIN_BOUND)
    assert carry == ((c & M32) + sum(coef) * M32) >> 32
    assert got % P == (c + sum(coef) * M64) % P


def test_permutation_model_runs_on_the_chained_rows(rc, bt):
    for st in ([0] * 12, [P - 1] * 12, [M64] * 12):
        want = gpt.permute_naive(st, rc)
        assert gpt.permute_b3(st, rc, bt) == want
        assert gpt.permute_b3(st, rc, bt, noncanonical=True) == want
