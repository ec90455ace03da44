"""CPU: the tables of the partial rounds in blocks of three (tools/gen_poseidon_tables.py b3_tables; csrc/poseidon.cuh psd_partial_rounds_b3) and the
half-exact model of the device algorithm: 32-bit halves, two 64-bit accumulators per dot product, the high one chained behind the low one
(chained_row: the start word asserted to fit 32 bits, the high chain asserted below 2^57; tests/test_poseidon_row_chain.py restates the
precondition row by row)."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_tables as gpt  # noqa: E402

P = gpt.P


@pytest.fixture(scope="module")
def rc():
    return gpt.load_rc()


@pytest.fixture(scope="module")
def bt(rc):
    return gpt.b3_tables(rc)


def states():
    rnd = random.Random(13)
    return [[0] * 12, [P - 1] * 12, [(1 << 32) - 1] * 12, list(range(12))] + [[rnd.randrange(P) for _ in range(12)] for _ in range(20)]


def test_model_equals_naive(rc, bt):
    for st in states():
        want = gpt.permute_naive(st, rc)
        assert gpt.permute_b3(st, rc, bt) == want
        assert gpt.permute_b3(st, rc, bt, noncanonical=True) == want
    assert gpt.permute_b3([0] * 12, rc, bt)[0] == 0x3c18a9786cb0b359            # plonky2's test vector for the all-zero state


def test_partial_rounds_take_any_u64(rc, bt):
    """the rounds alone on raw words, as the test hook runs them: both halves of every term at their maximum meet the accumulator bounds"""
    m = gpt.mds_matrix()
    mul = lambda a, b: a * b % P
    for st in ([(1 << 64) - 1] * 12, [1 << 32] * 12, [P - 1] * 12):
        s = [v % P for v in st]
        for r in range(gpt.HALF_F, gpt.HALF_F + gpt.R_P):
            s[0] = pow(s[0], 7, P)
            s = [(v + c) % P for v, c in zip(gpt.mat_vec(m, s), rc[r + 1])]
        assert gpt.b3_partial_rounds(st, rc, bt, mul) == s


def test_table_shape_and_bounds(bt):
    assert len(bt["mac"]) == 193 and len(bt["add"]) == 98
    assert [len(r) for r in bt["rows"]] == [12, 13] + [14] * 12
    assert [c for r in bt["rows"] for c in r] == bt["mac"]
    # a change of either figure means the derivation changed
    assert bt["max_coeff"] == max(bt["mac"]) == 1367024
    assert bt["max_row_sum"] == max(sum(r) for r in bt["rows"]) == 15068206
    assert 15068206 * ((1 << 32) - 1) + (1 << 32) - 1 < (1 << 56)
    assert all(0 <= c < P for c in bt["add"])


def test_header_is_current(bt):
    hdr = open(os.path.join(ROOT, "stark-verifier_amd", "csrc", "poseidon_b3tables.h")).read()
    _, mac_txt, add_txt = re.split(r"^PSD_TABLE_QUAL uint(?:32|64)_t PSD_B3_(?:MAC|ADD)\[\d+\] = \{$", hdr, flags=re.M)
    mac = [int(x, 16) for x in re.findall(r"\b(0x[0-9a-f]+)u,", mac_txt)]
    add = [int(x, 16) for x in re.findall(r"UINT64_C\((0x[0-9a-f]+)\)", add_txt)]
    want_mac, want_add = gpt.b3_header_words(bt)
    assert mac == want_mac and add == want_add
    w = gpt.B3_ROW_WORDS
    assert len(mac) == 14 * w and "#define PSD_B3_ROW_WORDS %d\n" % w in hdr and "#define PSD_B3_BLOCKS %d\n" % gpt.B3_BLOCKS in hdr
    # the rows without their zero padding are the 193 coefficients
    assert [v for i, r in enumerate(bt["rows"]) for v in mac[w * i: w * i + len(r)]] == bt["mac"]
    assert all(v == 0 for i, r in enumerate(bt["rows"]) for v in mac[w * i + len(r): w * (i + 1)])
    assert "__constant__ const" not in hdr and re.search(r"^PSD_TABLE_QUAL uint32_t PSD_B3_MAC\[", hdr, re.M)
