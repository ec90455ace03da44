"""CPU: the pass plan of the BN254 Fr transform (stark-verifier_amd/csrc/bn254_fr_route.h) under host sanitizers.

tests/fr_route_check.cpp -- a program with its own main that includes the header and nothing else of the library -- is compiled with the host
compiler of csrc/Makefile under AddressSanitizer and UBSan, as tests/test_ntt_route_host.py does for the Goldilocks route table, and run directly.
It prints, for an order, a size and whether input and output are one array, the split of the stages into passes and every pass in launch order with
its first / last marks and the buffers it reads and writes.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

from test_host_field import CSRC, FLAGS, ROOT, host_compiler

GATHER, DIF, FROM_BITREV = 0, 1, 2

# the split of log_n stages into passes, written out (not recomputed by the formula under test)
SPLIT = {k: [k] for k in range(11)}
SPLIT.update({k: [10, k - 10] for k in range(11, 18)})
SPLIT.update({18: [10, 4, 4], 19: [10, 5, 4], 20: [10, 5, 5], 21: [10, 6, 5], 22: [10, 6, 6], 23: [10, 7, 6], 24: [10, 7, 7], 25: [10, 5, 5, 5],
              26: [10, 6, 5, 5]})


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """(order, log_n, in_place) -> the parsed answer, for every size 0 .. 26, order and aliasing; a run under ASan and UBSan that reports anything
    does not exit 0"""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fr_route") / "fr_route_check")
    subprocess.run([cxx] + FLAGS + ["-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "fr_route_check.cpp"), "-o", exe], check=True)
    cases = [(order, log_n, in_place) for order in (GATHER, DIF, FROM_BITREV) for log_n in range(27) for in_place in (0, 1)]
    res = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases)
    return {c: parse(g) for c, g in zip(cases, lines)}


def parse(line):
    head, *steps = line.split(" | ")
    f = dict(w.split("=") for w in head.split())
    out = dict(ns=[int(x) for x in f["ns"].split(",")], s0=[int(x) for x in f["s0"].split(",")], flags=set(filter(None, f["flags"].split(","))),
               tail=int(f["tail"]), steps=[])
    for text in steps:
        where, marks, bufs = text.split(":")
        s0, ns = where.split("+")
        src, dst = bufs.split(">")
        out["steps"].append(dict(s0=int(s0), ns=int(ns), first=marks[0] == "f", last=marks[1] == "l", src=src, dst=dst))
    return out


def test_split_is_the_written_table(routes):
    assert sorted(SPLIT) == list(range(27))
    for (order, log_n, in_place), r in routes.items():
        assert r["ns"] == SPLIT[log_n], (log_n, r)
        assert sum(r["ns"]) == log_n
        assert r["s0"] == [sum(r["ns"][:k]) for k in range(len(r["ns"]))]
        # at least 8 adjacent columns in a 1024-element tile of every pass after the first
        assert r["ns"][0] <= 10 and all(ns <= 7 for ns in r["ns"][1:]), (log_n, r)


def test_gather_routes(routes):
    for log_n in range(27):
        for in_place in (0, 1):
            r = routes[(GATHER, log_n, in_place)]
            st, p = r["steps"], len(SPLIT[log_n])
            assert r["flags"] == set()
            assert [(s["s0"], s["ns"]) for s in st] == list(zip(r["s0"], r["ns"]))                  # ascending s0
            assert [s["first"] for s in st] == [True] + [False] * (p - 1) and [s["last"] for s in st] == [False] * (p - 1) + [True]
            assert [s["src"] for s in st] == ["in"] + ["work"] * (p - 1)
            one_pass_in_place = p == 1 and in_place == 1
            assert [s["dst"] for s in st] == ["work"] * (p - 1) + ["work" if one_pass_in_place else "out"]
            assert r["tail"] == int(one_pass_in_place), (log_n, in_place, r)
    # written out by hand
    assert routes[(GATHER, 10, 1)]["steps"] == [dict(s0=0, ns=10, first=True, last=True, src="in", dst="work")] and routes[(GATHER, 10, 1)]["tail"] == 1
    assert routes[(GATHER, 10, 0)]["steps"] == [dict(s0=0, ns=10, first=True, last=True, src="in", dst="out")] and routes[(GATHER, 10, 0)]["tail"] == 0
    for in_place in (0, 1):
        assert routes[(GATHER, 11, in_place)]["steps"] == [dict(s0=0, ns=10, first=True, last=False, src="in", dst="work"),
                                                           dict(s0=10, ns=1, first=False, last=True, src="work", dst="out")]
        assert routes[(GATHER, 23, in_place)]["steps"] == [dict(s0=0, ns=10, first=True, last=False, src="in", dst="work"),
                                                           dict(s0=10, ns=7, first=False, last=False, src="work", dst="work"),
                                                           dict(s0=17, ns=6, first=False, last=True, src="work", dst="out")]


def test_dif_routes(routes):
    for log_n in range(27):
        for in_place in (0, 1):
            r = routes[(DIF, log_n, in_place)]
            st, p = r["steps"], len(SPLIT[log_n])
            assert r["flags"] == {"no_gather", "dif"} and r["tail"] == 0
            assert [(s["s0"], s["ns"]) for s in st] == list(zip(r["s0"], r["ns"]))[::-1]            # from the highest s0 down
            assert [s["first"] for s in st] == [True] + [False] * (p - 1)                            # the highest pass reads the input
            assert [s["last"] for s in st] == [False] * (p - 1) + [True] and st[-1]["s0"] == 0       # the s0 = 0 pass finishes
            assert [s["src"] for s in st] == ["in"] + ["out"] * (p - 1) and all(s["dst"] == "out" for s in st)      # no WORK buffer
    assert routes[(DIF, 23, 0)]["steps"] == [dict(s0=17, ns=6, first=True, last=False, src="in", dst="out"),
                                             dict(s0=10, ns=7, first=False, last=False, src="out", dst="out"),
                                             dict(s0=0, ns=10, first=False, last=True, src="out", dst="out")]


def test_from_bitrev_routes(routes):
    for log_n in range(27):
        for in_place in (0, 1):
            r = routes[(FROM_BITREV, log_n, in_place)]
            st, p = r["steps"], len(SPLIT[log_n])
            assert r["flags"] == {"no_gather"} and r["tail"] == 0
            assert [(s["s0"], s["ns"]) for s in st] == list(zip(r["s0"], r["ns"]))
            assert [s["first"] for s in st] == [True] + [False] * (p - 1) and [s["last"] for s in st] == [False] * (p - 1) + [True]
            assert [s["src"] for s in st] == ["in"] + ["out"] * (p - 1) and all(s["dst"] == "out" for s in st)
    assert routes[(FROM_BITREV, 25, 1)]["steps"] == [dict(s0=0, ns=10, first=True, last=False, src="in", dst="out"),
                                                     dict(s0=10, ns=5, first=False, last=False, src="out", dst="out"),
                                                     dict(s0=15, ns=5, first=False, last=False, src="out", dst="out"),
                                                     dict(s0=20, ns=5, first=False, last=True, src="out", dst="out")]


def test_tail_copy_only_for_one_gathering_pass_in_place(routes):
    with_tail = sorted(c for c, r in routes.items() if r["tail"])
    assert with_tail == [(GATHER, log_n, 1) for log_n in range(11)]
    # a pass never reads a buffer that no earlier pass wrote, and only the tail copy reads WORK after the last pass
    for c, r in routes.items():
        written = {"in"}
        for s in r["steps"]:
            assert s["src"] in written, (c, r)
            written.add(s["dst"])
        assert ("out" in written) != bool(r["tail"]), (c, r)
