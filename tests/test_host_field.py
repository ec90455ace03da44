"""CPU: the host's one BN254 field class (stark-verifier_amd/csrc/host_mont.h) for both moduli, against Python integers.

tests/host_field_check.cpp -- a stand-alone program that includes nothing of the project but that header -- is compiled with the host
compiler of csrc/Makefile under AddressSanitizer and UBSan (any report aborts it); the cases go in as hex lines, the answers come back the
same way.  Nothing is loaded into Python.  Operands per modulus m: the edge values 0, 1, 2, m-2, m-1, (m-1)/2, (m+1)/2, R mod m, R^2 mod m,
2^253 and 200 seeded random values.  Binary operations (* + - less_than ==) run on every ordered pair of edge values and on each random
value with its successor (cyclically); unary ones (neg, inv, is_zero, the word round trip, pow by 0, 1, m-2 and 2^256-1) on every value.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stark-verifier_amd", "csrc")
FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MODULI = {"r": FR, "q": FQ}
RADIX = 1 << 256
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def host_compiler():
    """HOSTCXX of csrc/Makefile (the environment's, else the Makefile's default), else the system's C++ compiler"""
    default = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("HOSTCXX ?="):
            default = line.split("=", 1)[1].strip()
    for cand in (os.environ.get("HOSTCXX"), default, "g++", "c++"):
        path = cand and shutil.which(cand)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_field") / "host_field_check")
    subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "host_field_check.cpp"), "-o", exe], check=True)

    def ask(lines):
        res = subprocess.run([exe], input="".join(c + "\n" for c in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        got = res.stdout.split()
        assert len(got) == len(lines)
        return got
    return ask


def check(ask, cases):
    """cases: (line, expected answer); every answer is compared"""
    got = ask([c for c, _ in cases])
    bad = [(c, want, g) for (c, want), g in zip(cases, got) if g != want]
    assert not bad, "%d of %d cases differ, the first: %r" % (len(bad), len(cases), bad[0])


def hx(v):
    assert 0 <= v < RADIX
    return "%064x" % v


def operands(m, seed):
    edge = [0, 1, 2, m - 2, m - 1, (m - 1) // 2, (m + 1) // 2, RADIX % m, RADIX * RADIX % m, (1 << 253) % m]
    rng = random.Random(seed)
    return edge, [rng.randrange(m) for _ in range(200)]


@pytest.mark.parametrize("f", ["r", "q"])
def test_binary_ops(ask, f):
    m = MODULI[f]
    edge, rnd = operands(m, 0x355 + ord(f))
    pairs = [(a, b) for a in edge for b in edge] + [(rnd[i], rnd[(i + 1) % len(rnd)]) for i in range(len(rnd))]
    cases = []
    for a, b in pairs:
        args = "%s %s" % (hx(a), hx(b))
        cases.append(("%s mul %s" % (f, args), hx(a * b % m)))
        cases.append(("%s add %s" % (f, args), hx((a + b) % m)))
        cases.append(("%s sub %s" % (f, args), hx((a - b) % m)))
        cases.append(("%s lt %s" % (f, args), "1" if a < b else "0"))
        cases.append(("%s eq %s" % (f, args), "1" if a == b else "2"))       # bit 0: ==, bit 1: !=
    check(ask, cases)


@pytest.mark.parametrize("f", ["r", "q"])
def test_unary_ops_and_pow(ask, f):
    m = MODULI[f]
    edge, rnd = operands(m, 0x355 + ord(f))
    cases = []
    for a in edge + rnd:
        cases.append(("%s neg %s" % (f, hx(a)), hx(-a % m)))
        cases.append(("%s inv %s" % (f, hx(a)), hx(pow(a, m - 2, m))))
        cases.append(("%s zero %s" % (f, hx(a)), "1" if a == 0 else "0"))
        cases.append(("%s words %s" % (f, hx(a)), hx(a)))
        for e in (0, 1, m - 2, RADIX - 1):
            cases.append(("%s pow %s %s" % (f, hx(a), hx(e)), hx(pow(a, e, m))))
    assert pow(0, m - 2, m) == 0                                             # inv(0) == 0 is among the cases
    check(ask, cases)


@pytest.mark.parametrize("f", ["r", "q"])
def test_raw_words_are_reduced(ask, f):
    """from_words and from_mont_words accept any 256-bit word string; what comes out is the canonical residue"""
    m = MODULI[f]
    cases = []
    for w in (m, m + 1, 2 * m - 1, 2 * m, RADIX - 1, 0, m - 1):
        cases.append(("%s words %s" % (f, hx(w)), hx(w % m)))
        cases.append(("%s mont %s" % (f, hx(w)), hx(w % m)))
    check(ask, cases)


def test_root_of_unity_order(ask):
    ks = (0, 1, 28)
    for k, ans in zip(ks, ask(["r root %d" % k for k in ks])):
        w = int(ans, 16)
        assert w < FR and pow(w, 1 << k, FR) == 1
        assert k == 0 or pow(w, 1 << (k - 1), FR) != 1, "the order of root_of_unity(%d) is below 2^%d" % (k, k)
