"""CPU: the one host statement of the Halo2 descriptor (stark-verifier_amd/csrc/plonk_desc.h) under host sanitizers.

tests/plonk_desc_check.cpp -- a program with its own main that includes plonk_desc.h and is linked with host_keccak.cpp only -- is
compiled with the host compiler of csrc/Makefile under AddressSanitizer and UBSan, as tests/test_gate_shape_host.py does for the gate
table.  It parses each descriptor it is given with plk_parse_desc, prints the refusal or the header, the derived shape, the emit counts
and plk_perm_queries, and runs every program through plk_run_program over heap arrays of exactly the query counts and the constant
pool (a read outside them is a sanitizer report, which aborts the program); on request it prints plk_pinned_digest.  Nothing is loaded
into Python.

Accepted descriptors are compared with the ConstraintSystem they were exported from (shape, Horner folds of the expression trees in
Python integers, halo2.vk_digest); the mutation list of tests/plonk_desc_cases.py and a seeded sweep of single-word corruptions with that
file's statement of the bounds in Python integers."""
import importlib
import os
import random
import subprocess

import numpy as np
import pytest

import halo2_verifier as hv
import plonk_desc_cases as pdc
from halo2_circuits import plonk_with_tuple_lookup, random_circuit
from test_host_field import CSRC, FLAGS, ROOT, host_compiler

h2 = importlib.import_module("stark-verifier_amd.halo2")
ch = importlib.import_module("stark-verifier_amd.halo2_chips")
R = h2.R
M64 = (1 << 64) - 1
CIRCUITS = {
    "chip_shape": lambda: (7, ch.synthetic_circuit(7, table_bits=5, n_permutations=1)[0]),
    "tuple_lookup": lambda: (7, plonk_with_tuple_lookup(7, 5)[0]),
    "random0": lambda: (6, random_circuit(6, 0)[0]),
    "random1": lambda: (7, random_circuit(7, 1)[0]),
    "random2": lambda: (6, random_circuit(6, 2)[0]),
    "random3": lambda: (7, random_circuit(7, 3)[0]),
}
_cache = {}


def circuit(name):
    """(k, cs, the descriptor with a zero digest field as Python integers)"""
    if name not in _cache:
        k, cs = CIRCUITS[name]()
        _cache[name] = (k, cs, [int(x) for x in h2.export_desc(cs, k, 0)])
    return _cache[name]


def seeded(a, b):
    """plonk_desc_check.cpp's scalars: four splitmix64 words from the state 0x355 + (a << 32) + b, little-endian, mod r"""
    s, v = 0x355 + (a << 32) + b, 0
    for i in range(4):
        s = (s + 0x9E3779B97F4A7C15) & M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        v |= (z ^ (z >> 31)) << (64 * i)
    return v % R


def line(w, max_k, commitments=()):
    return "%d %d %s" % (max_k, len(w), " ".join("%x" % x for x in list(w) + list(commitments)))


def shape_of(w):
    """the first four fields of the answer to an accepted descriptor, from its words alone"""
    k, deg, bf, n_perm = w[2], w[8], w[9], w[6]
    progs, _ = pdc.programs(w)
    emits = [sum(1 for i in range(n) if w[at + 2 * i] & 0xFFFFFFFF == 3) for at, n in progs]
    pq = pdc.perm_queries(w)
    return "ok %s %d %d | %d %d %d %d %d %d | %s | %s |" % (
        " ".join("%d" % x for x in w[2:10] + [w[15]]), 2 ** k, 2 ** k - bf - 1, w[3], w[4], w[5], deg - 1, deg - 2, -(-n_perm // (deg - 2)),
        " ".join(["%d" % emits[0]] + ["%d/%d" % (emits[1 + 2 * l], emits[2 + 2 * l]) for l in range(w[7])]),
        "none" if pq is None else " ".join("%d" % q for q in pq))


def want(w, max_k):
    """(exact answer or None, prefix the answer must start with)"""
    why = pdc.refusal(w, max_k)
    return ("refused " + why, "") if why else (None, shape_of(w))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("plonk_desc") / "plonk_desc_check")
    subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "plonk_desc_check.cpp"), os.path.join(CSRC, "host_keccak.cpp"), "-o", exe], check=True)

    def ask(lines):
        res = subprocess.run([exe], input="".join(c + "\n" for c in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        got = res.stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return ask


def check(ask, cases, max_k):
    """cases: (what, descriptor); every answer is the refusal this file expects, or starts with the shape it expects"""
    got = ask([line(w, max_k) for _, w in cases])
    bad = []
    for (what, w), g in zip(cases, got):
        exact, prefix = want(w, max_k)
        if g != exact if exact is not None else not g.startswith(prefix):
            bad.append((what, exact or prefix, g))
    assert not bad, "%d of %d descriptors differ, the first (what, expected, answer): %r" % (len(bad), len(cases), bad[0])
    return got


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_shape_programs_and_digest_equal_the_constraint_system(ask, name):
    k, cs, w = circuit(name)
    rng = np.random.default_rng(0x355)
    fc = rng.integers(0, 1 << 63, (cs.num_fixed, 8), dtype=np.uint64)
    sc = rng.integers(0, 1 << 63, (len(cs.permutation), 8), dtype=np.uint64)
    got, = ask([line(w, pdc.MAX_K_DEVICE, [int(x) for x in fc.reshape(-1)] + [int(x) for x in sc.reshape(-1)])])
    deg, bf, n_perm = cs.degree(), cs.blinding_factors(), len(cs.permutation)
    head = [k, cs.num_advice, cs.num_fixed, cs.num_instance, n_perm, len(cs.lookups), deg, bf, len(cs.all_gate_polys()), 2 ** k, 2 ** k - bf - 1]
    shape = [cs.num_advice, cs.num_fixed, cs.num_instance, deg - 1, deg - 2, -(-n_perm // (deg - 2))]
    emits = ["%d" % len(cs.all_gate_polys())] + ["%d/%d" % (len(ins), len(tabs)) for _, ins, tabs in cs.lookups]
    pq = [cs.queries[c.kind].index((c.index, 0)) for c in cs.permutation]

    def fold(exprs, by):
        acc = 0
        for e in exprs:
            acc = (acc * by + e.evaluate(seeded)) % R
        return "%064x" % acc
    y, theta = seeded(7, 0), seeded(8, 0)
    values = [fold(cs.all_gate_polys(), y)] + ["%s/%s" % (fold(ins, theta), fold(tabs, theta)) for _, ins, tabs in cs.lookups]
    digest = "%064x" % h2.vk_digest(cs, k, fc, sc, hv.keccak256)
    expected = "ok " + " | ".join(" ".join(str(x) for x in part) for part in (head, shape, emits, pq, values, [digest]))
    assert got == expected
    assert got.startswith(shape_of(w))
    # a non-zero digest field is the digest, whatever the commitments
    given = list(w)
    given[16:20] = [5, 6, 7, 8]
    got, = ask([line(given, pdc.MAX_K_DEVICE, [1] * (8 * (cs.num_fixed + n_perm)))])
    assert got.endswith("| %064x" % ((5 | 6 << 64 | 7 << 128 | 8 << 192) % R))


@pytest.mark.parametrize("name", ["random0", "tuple_lookup"])
@pytest.mark.parametrize("max_k", [pdc.MAX_K_DEVICE, pdc.MAX_K_VERIFIER])
def test_mutation_list(ask, name, max_k):
    k, cs, w = circuit(name)
    cases = pdc.mutations(w, max_k)
    got = check(ask, cases, max_k)
    by_answer = {}
    for (what, _), g in zip(cases, got):
        by_answer.setdefault(g.split(" |")[0] if g.startswith("ok") else g, []).append(what)
    refusals = {g[len("refused "):] for g in by_answer if g.startswith("refused")}
    wanted = {"null or truncated descriptor", "not a version-1 gl355 PLONK descriptor", "implausible circuit shape", "fewer rows than the blinding needs",
              "truncated descriptor", "bad permutation column", "bad query", "bad gate program", "descriptor length does not match its header"}
    assert refusals >= wanted | ({"bad lookup program"} if cs.lookups else set()), wanted - refusals
    answers = dict(zip((what for what, _ in cases), got))
    assert answers["header word 2 = %d" % max_k].startswith("ok %d " % max_k) and answers["header word 2 = %d" % (max_k + 1)] == "refused implausible circuit shape"
    assert answers["header word 15 = %d" % (1 << 20)].startswith("ok") and answers["header word 15 = %d" % ((1 << 20) + 1)] == "refused implausible circuit shape"
    assert " | none | " in answers["the first permutation column is not queried at rotation 0"]
    assert sum(1 for g in got if g.startswith("ok")) > 100                         # the inner side of the operand bounds: evaluated without a report


def test_seeded_sweep_of_single_word_corruptions(ask):
    k, cs, w = circuit("random0")
    rng = random.Random(0x9D5C)
    cases = []
    for _ in range(2000):
        at = rng.randrange(len(w))
        how = rng.randrange(6)
        old = w[at]
        new = (old ^ 1 << rng.randrange(64), rng.getrandbits(64), rng.randrange(20), (old + rng.choice((-1, 1))) & M64,
               old & ~0xFFFFFFFF | rng.randrange(1 << 12), old & 0xFFFFFFFF | rng.randrange(1 << 12) << 32)[how]
        cases.append(("word %d: %x -> %x" % (at, old, new), pdc._with(w, at, new)))
    got = check(ask, cases, pdc.MAX_K_DEVICE)
    n_ok = sum(1 for g in got if g.startswith("ok"))
    assert 200 < n_ok < 1800, n_ok                                                 # the sweep sees both verdicts often
