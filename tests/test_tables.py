"""CPU: the derived Poseidon fast-partial-round tables (tools/gen_poseidon_tables.py)."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_tables as gpt  # noqa: E402


def test_fast_equals_naive_and_header_is_current():
    rc = gpt.load_rc()
    tb = gpt.derive(rc)
    rnd = random.Random(11)
    for _ in range(5):
        st = [rnd.randrange(gpt.P) for _ in range(12)]
        assert gpt.permute_fast(st, rc, tb) == gpt.permute_naive(st, rc)
    assert tb["post"][21] == 0 and tb["first"][0] == rc[4][0]
    hdr = open(os.path.join(ROOT, "stark-verifier_amd", "csrc", "poseidon_fast_tables.h")).read()
    for v in (tb["first"][5], tb["post"][7], tb["vs"][3][4], tb["w_hats"][20][10], tb["init"][10][10]):
        assert "0x%016x" % v in hdr


def test_tables_equal_reference_literals():
    # the reference's literal tables, transcribed into tests/golden/ (make_golden.py poseidon-fast-tables)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_fast_partial_tables.json")))
    grab = lambda name: [int(x, 16) for x in ref[name]]
    tb = gpt.derive(gpt.load_rc())
    assert grab("FAST_PARTIAL_FIRST_ROUND_CONSTANT") == tb["first"]
    assert grab("FAST_PARTIAL_ROUND_CONSTANTS") == tb["post"]
    assert grab("FAST_PARTIAL_ROUND_VS") == [x for row in tb["vs"] for x in row]
    assert grab("FAST_PARTIAL_ROUND_W_HATS") == [x for row in tb["w_hats"] for x in row]
    assert grab("FAST_PARTIAL_ROUND_INITIAL_MATRIX") == [x for row in tb["init"] for x in row]
