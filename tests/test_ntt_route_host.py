"""CPU: the route table of the Goldilocks NTT (stark-verifier_amd/csrc/ntt_route.h) under host sanitizers.

tests/ntt_route_check.cpp -- a program with its own main that includes the header and nothing else of the library -- is compiled with the host
compiler of csrc/Makefile under AddressSanitizer and UBSan, as tests/test_merkle_update_plan_host.py does for the Merkle update plan, and run
directly.  It prints the route of every shape it is given: the kernel instance of each pass with its tables, flags, profile scope and grid.
The hand-written routes are the rows of docs/history/ntt_shapes.md; the sweep is over every shape the three callers in capi.hip (ntt_dev,
intt_from_bitrev_dev, lde_dev) can build.  Nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

from test_host_field import CSRC, FLAGS, ROOT, host_compiler

FIELDS = ("log_n", "n_cosets", "inverse", "in_bitrev", "out_bitrev", "pre", "post", "scale", "ratio", "out_contig", "cosets_contig", "slot0_zero",
          "batch_fits_y", "opt")


def shape(log_n, **kw):
    s = dict(log_n=log_n, n_cosets=1, inverse=0, in_bitrev=0, out_bitrev=0, pre=0, post=0, scale=0, ratio=0, out_contig=1, cosets_contig=0,
             slot0_zero=1, batch_fits_y=1, opt=12)
    s.update(kw)
    return tuple(int(s[f]) for f in FIELDS)


# the shapes the three callers build (capi.hip)
def ntt_dev(log_n, inverse=False, coset=False, **kw):
    """gl355_ntt / gl355_coset_ntt: natural order in and out; an inverse above 2^14 arrives bit-reversed (the caller permutes first)"""
    if not inverse:
        return shape(log_n, pre=coset, **kw)
    return shape(log_n, inverse=1, in_bitrev=log_n > 14, post=coset, scale=log_n > 0, **kw)


def intt_from_bitrev(log_n, coset=False, **kw):
    return shape(log_n, inverse=1, in_bitrev=1, post=coset, scale=log_n > 0, **kw)


def lde(log_n, rate_bits, **kw):
    """gl355_lde / gl355_lde_bitrev: 2^rate_bits cosets in contiguous blocks, bit-reversed out (natural order is the caller's extra pass)"""
    return shape(log_n, n_cosets=1 << rate_bits, out_bitrev=1, pre=1, ratio=1, cosets_contig=1, **kw)


def domain():
    out = []
    for opt in (12, 13, 14):
        for fits in (1, 0):
            for contig in (1, 0):
                kw = dict(opt=opt, batch_fits_y=fits, out_contig=contig)
                for log_n in range(25):
                    for coset in (False, True):
                        out.append(ntt_dev(log_n, False, coset, **kw))
                        out.append(ntt_dev(log_n, True, coset, **kw))
                        out.append(intt_from_bitrev(log_n, coset, **kw))
                    for rate_bits in range(5):
                        if log_n:
                            out.append(lde(log_n, rate_bits, **kw))
    return out


STEP = re.compile(r"^(\w+)<(\d+),(\d+),(\d+),(\d+),(\d+)>\[([^;\]]*);([^\]]*)\] rows=(\d+) xf=(\d+) shift=(\d+) (\w+)>(\w+) (\w+)\*(\d+) grid=(\d+),(\d+)$")


def parse(line):
    """a route line -> list of steps (dicts), or ('refused', code, message)"""
    if line.startswith("refused "):
        _, code, msg = line.split(" ", 2)
        return ("refused", int(code), msg)
    steps = []
    for text in line.split(" | "):
        m = STEP.match(text)
        assert m, "cannot read the step %r" % text
        g = m.groups()
        steps.append(dict(form=g[0], lt=int(g[1]), log_t=int(g[2]), pre=int(g[3]), inv=int(g[4]), pass_=int(g[5]), inst=text.split("[")[0],
                          tabs=set(filter(None, g[6].split(","))), flags=set(filter(None, g[7].split(","))), rows=int(g[8]), xf=int(g[9]),
                          shift=int(g[10]), src=g[11], dst=g[12], scope=g[13], bytes=int(g[14]), grid=(int(g[15]), int(g[16]))))
    return steps


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ntt_route") / "ntt_route_check")
    subprocess.run([cxx] + FLAGS + ["-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "ntt_route_check.cpp"), "-o", exe], check=True)

    def ask(shapes):
        """the answer lines; a run under ASan and UBSan that reports anything does not exit 0"""
        lines = ["instances\n" if s == "instances" else " ".join(map(str, s)) + "\n" for s in shapes]
        res = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        got = res.stdout.splitlines()
        assert len(got) == len(shapes)
        return got
    return ask


@pytest.fixture(scope="module")
def sweep(ask):
    shapes = domain()
    return shapes, [parse(g) for g in ask(shapes)]


def route(ask, s):
    r = parse(ask([s])[0])
    assert isinstance(r, list), r
    return r


def insts(r):
    return [st["inst"] for st in r]


# ---- 1. the routes written out by hand ----------------------------------------------------------------------------------------------------------------
def test_single_pass_routes(ask):
    for log_n in range(1, 12):
        for s, inv in ((ntt_dev(log_n), 0), (ntt_dev(log_n, coset=True), 0), (ntt_dev(log_n, True), 1), (ntt_dev(log_n, True, True), 1),
                       (intt_from_bitrev(log_n), 1), (lde(log_n, 3), 0)):
            r = route(ask, s)
            assert insts(r) == ["rows16<12,%d,0,%d,0>" % (log_n, inv)], (log_n, s, r)
            assert r[0]["scope"] == "ntt_rows_single_pass" and r[0]["rows"] == 0 and "canon" in r[0]["flags"]
    for log_n in (12, 14):
        for coset in (False, True):
            r = route(ask, ntt_dev(log_n, coset=coset))
            assert insts(r) == ["rows16<%d,%d,0,0,0>" % (log_n, log_n)] and "natural_out" in r[0]["flags"]
            assert r[0]["tabs"] == (set() if not coset else {"pre:1"} if log_n == 12 else {"pre:full"})
        r = route(ask, ntt_dev(log_n, True))
        assert insts(r) == ["rows8<%d,%d,0,1,0>" % (log_n, log_n)] and r[0]["tabs"] == {"scale"} and "natural_out" in r[0]["flags"]
        r = route(ask, ntt_dev(log_n, True, True))
        assert insts(r) == ["rows16<%d,%d,0,1,0>" % (log_n, log_n)] and r[0]["tabs"] == {"scale", "post:1" if log_n == 12 else "post:2"}
    r = route(ask, ntt_dev(0))
    assert insts(r) == ["points<12,0,0,0,0>"] and r[0]["scope"] == "ntt_single_points" and r[0]["bytes"] == 16


def test_two_pass_routes_up_to_2p20(ask):
    for contig in (1, 0):
        r = route(ask, ntt_dev(15, out_contig=contig))
        assert insts(r) == ["cols8_nat<12,8,0,0,0>", "cols8_nat<12,7,0,0,1>"]
        assert [st["scope"] for st in r] == ["ntt_cols_pass1", "ntt_cols_pass2"] and [(st["src"], st["dst"]) for st in r] == [("in", "mid"), ("mid", "out")]
        assert r[0]["tabs"] == {"root", "step:nat"} and r[1]["tabs"] == set() and (r[0]["rows"], r[1]["rows"]) == (7, 8)
    assert insts(route(ask, ntt_dev(20))) == ["cols8_nat<13,10,0,0,0>", "cols8_nat<13,10,0,0,1>"]
    r = route(ask, ntt_dev(15, coset=True))
    assert insts(r) == ["cols8<12,3,1,0,0>", "rows_l24<12,12,0,0,0>", "bitrev<12,0,0,0,0>"]
    assert r[0]["tabs"] == {"root", "pre:full", "step:full"} and r[1]["tabs"] == {"mid"} and r[1]["flags"] == {"canon"}
    r = route(ask, ntt_dev(15, True))
    assert insts(r) == ["rows16<12,12,0,1,0>", "cols16<12,3,0,1,0>"]
    assert [st["scope"] for st in r] == ["ntt_bitrev_in_rows_pass1", "ntt_bitrev_in_cols_pass2"]
    assert r[0]["flags"] == {"bitrev_in", "natural_out"} and r[1]["flags"] == {"bitrev_in", "natural_out", "canon"}
    assert r[0]["tabs"] == {"root"} and r[1]["tabs"] == {"step:2", "scale"}
    assert route(ask, ntt_dev(15, True, True))[1]["tabs"] == {"step:2", "post:2", "scale"}


def test_routes_above_2p20(ask):
    limb, rev = "rows_l24<12,12,0,0,0>", "bitrev<12,0,0,0,0>"
    assert insts(route(ask, ntt_dev(21))) == ["cols8_big<13,9,0,0,0>", limb, rev]
    assert insts(route(ask, ntt_dev(22))) == ["cols8_big<13,10,0,0,0>", limb, rev]
    r = route(ask, ntt_dev(21, out_contig=0))
    assert insts(r) == ["cols16<12,9,0,0,0>", limb, rev] and r[0]["tabs"] == {"root", "step:2"}
    r = route(ask, ntt_dev(22, out_contig=0))
    assert insts(r) == ["cols16<12,8,0,0,0>", "rows8<14,14,0,0,0>", rev] and r[0]["tabs"] == {"root", "step:2"}
    for log_n in (23, 24):
        r = route(ask, ntt_dev(log_n))
        assert insts(r) == ["cols8<12,%d,0,0,0>" % (log_n - 17), "cols8<12,5,0,0,0>", limb, rev]
        assert [st["scope"] for st in r] == ["ntt_cols_pass1", "ntt_cols_pass1", "ntt_rows_pass2", "bitrev_permute"]
        assert [(st["xf"], st["shift"], st["rows"]) for st in r[:3]] == [(log_n, 0, 17), (17, log_n - 17, 12), (17, log_n - 17, 5)]
        assert "root" in r[0]["tabs"] and "root" in r[1]["tabs"] and all(st["tabs"] >= {"step:full"} for st in r[:2])
    r = route(ask, ntt_dev(22, True))
    assert insts(r) == ["rows16<14,14,0,1,0>", "cols16<12,8,0,1,0>"]


def test_lde_routes(ask):
    limb = "rows_l24<12,12,0,0,0>"
    assert insts(route(ask, lde(5, 3))) == ["rows16<12,5,0,0,0>"]
    r = route(ask, lde(12, 3))
    assert insts(r) == ["rows8<12,12,1,0,0>"] and r[0]["tabs"] == {"pre:1full"}
    assert insts(route(ask, lde(13, 3, opt=12))) == ["cols_small_cosets<12,1,0,0,0>", limb]
    r = route(ask, lde(13, 3, opt=13))
    assert insts(r) == ["rows8<13,13,1,0,0>"] and r[0]["tabs"] == {"pre:full"}
    assert insts(route(ask, lde(14, 1, opt=12))) == ["cols_small_cosets<12,2,0,0,0>", limb]
    assert insts(route(ask, lde(14, 1, opt=14))) == ["rows8<14,14,1,0,0>"]
    assert insts(route(ask, lde(15, 3))) == ["cols_small_cosets<12,3,0,0,0>", limb]
    assert insts(route(ask, lde(16, 3))) == ["cols8_cosets<12,4,0,0,0>", limb]
    r = route(ask, lde(17, 3))                   # the benchmark's shape
    assert insts(r) == ["cols_l24_cosets<12,5,0,0,0>", limb]
    assert r[0]["tabs"] == {"root", "pre:full", "step:full", "ratio"} and r[1]["tabs"] == {"mid"} and r[1]["flags"] == {"canon", "collapse"}
    assert (r[1]["rows"], r[1]["bytes"]) == (5 + 3, 64) and [st["scope"] for st in r] == ["ntt_cols_pass1", "ntt_rows_pass2"]
    assert insts(route(ask, lde(17, 0))) == ["cols8<12,5,1,0,0>", limb]
    assert insts(route(ask, lde(18, 3))) == ["cols8_cosets<12,6,0,0,0>", limb]
    for log_n, rate in ((18, 4), (19, 3)):
        r = route(ask, lde(log_n, rate))
        assert insts(r) == ["cols16<12,%d,0,0,0>" % (log_n - 12), limb] and r[0]["tabs"] == {"root", "pre:2", "step:full"}
    assert insts(route(ask, lde(21, 2))) == ["cols16<12,9,0,0,0>", limb]
    assert insts(route(ask, lde(22, 1))) == ["cols16<12,8,0,0,0>", "rows8<14,14,0,0,0>"]


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ask):
    cases = [
        (shape(25), -5, "ntt: log_n > 24"),
        (shape(10, n_cosets=0), -1, "ntt: bad coset count"),
        (shape(10, n_cosets=17), -1, "ntt: bad coset count"),
        (shape(16, n_cosets=4, pre=1, out_bitrev=1, cosets_contig=0), -1, "ntt: multi-coset two-pass needs contiguous coset blocks"),
        (shape(16, inverse=1, in_bitrev=1, out_bitrev=1), -5, "ntt: bitrev -> bitrev not provided"),
        (shape(16, n_cosets=4, in_bitrev=1, cosets_contig=1), -5, "ntt: bitrev-input flow is single-coset"),
        (shape(16, n_cosets=4, pre=1, cosets_contig=1), -5, "ntt: natural-order multi-coset output"),
        (shape(16, post=1, out_bitrev=1), -5, "ntt: post-multiplier needs natural-order output"),
    ]
    for (s, code, prefix), g in zip(cases, ask([c[0] for c in cases])):
        r = parse(g)
        assert r[0] == "refused" and r[1] == code and r[2].startswith(prefix), (s, g)


# ---- 3. the callers' whole domain -----------------------------------------------------------------------------------------------------------------------
def test_sweep_names_listed_instances_and_reaches_each(ask, sweep):
    shapes, routes = sweep
    listed = ask(["instances"])[0].split()
    assert len(listed) == len(set(listed))
    reached = set()
    for s, r in zip(shapes, routes):
        assert isinstance(r, list), "a shape of the callers' domain is refused: %r %r" % (dict(zip(FIELDS, s)), r)
        reached.update(insts(r))
    assert reached <= set(listed), "routes name instances that are not compiled: %s" % sorted(reached - set(listed))
    assert set(listed) <= reached, "compiled instances that no shape of the callers reaches (dead kernels): %s" % sorted(set(listed) - reached)


# the kernels' own static bounds (ntt_kernels.cuh, ntt_l24.cuh): form -> predicate on a step
BOUNDS = {
    "points": lambda st: st["log_t"] == 0,
    "rows16": lambda st: 1 <= st["log_t"] <= st["lt"] and st["lt"] == max(12, st["log_t"]) <= 14,
    "rows8": lambda st: st["log_t"] == st["lt"] and 12 <= st["lt"] <= 14,
    "rows_l24": lambda st: st["log_t"] == 12,
    "cols16": lambda st: st["lt"] == 12 and 1 <= st["log_t"] <= 12 and st["rows"] >= 12 - st["log_t"],
    "cols8": lambda st: st["lt"] == 12 and 1 <= st["log_t"] <= 12 and st["rows"] >= 12 - st["log_t"],
    "cols8_big": lambda st: st["lt"] == 13 and 1 <= st["log_t"] <= 13 and st["rows"] >= 13 - st["log_t"],
    "cols8_cosets": lambda st: st["lt"] == 12 and 1 <= st["log_t"] <= 12 and st["rows"] >= 12 - st["log_t"],
    "cols8_nat": lambda st: st["lt"] in (12, 13) and 3 <= st["log_t"] <= st["lt"] - 3 and st["rows"] >= st["lt"] - st["log_t"],   # LOG_TC >= 3
    "cols_l24_cosets": lambda st: st["log_t"] == 5 and st["rows"] >= 6,                # tiles of 64 columns
    "cols_small_cosets": lambda st: 1 <= st["log_t"] <= 3 and st["rows"] >= 8,         # 256 columns per block
    "bitrev": lambda st: True,
}


def test_sweep_static_bounds_and_grids(sweep):
    shapes, routes = sweep
    for s, r in zip(shapes, routes):
        d = dict(zip(FIELDS, s))
        assert 1 <= len(r) <= 4
        for st in r:
            assert BOUNDS[st["form"]](st), (d, st)
            if st["form"] == "bitrev":
                assert st["grid"] == (0, 0)
            else:
                assert all(0 < g < 1 << 31 for g in st["grid"]), (d, st)
            # a pass covers its transform: 2^log_t points per row or column, 2^rows of them, the collapsed cosets among the rows
            lc = d["n_cosets"].bit_length() - 1 if "collapse" in st["flags"] else 0
            if st["form"] not in ("bitrev", "points"):
                assert st["log_t"] + st["rows"] - lc == st["xf"], (d, st)
            assert st["xf"] + st["shift"] == d["log_n"]
        assert r[0]["src"] == "in" and r[-1]["dst"] == "out" and all(a["dst"] == b["src"] for a, b in zip(r, r[1:]))
        assert ("root" in r[0]["tabs"]) == (len(r) > 1)


# ---- 4. the cosets collapse into rows only where their blocks tile the column ---------------------------------------------------------------------------
def test_multi_coset_two_pass_needs_contiguous_blocks(ask, sweep):
    shapes, routes = sweep
    seen = 0
    for s, r in zip(shapes, routes):
        d = dict(zip(FIELDS, s))
        if d["n_cosets"] > 1 and len(r) > 1:
            assert d["cosets_contig"] and "collapse" in r[-1]["flags"], (d, r)
            seen += 1
            g = parse(ask([shape(**dict(d, cosets_contig=0))])[0]) if seen <= 40 else None
            if g is not None and d["log_n"] > 14:
                assert g[0] == "refused" and g[1] == -1, (d, g)
    assert seen > 100


# ---- 5. the whole sweep under the sanitizers: `ask` asserts exit status 0 of the ASan + UBSan build -----------------------------------------------------
def test_sweep_is_clean_under_sanitizers(sweep):
    shapes, routes = sweep
    assert len(shapes) == len(routes) > 2000
