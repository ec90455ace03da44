"""CPU: the host BN254 pairing behind the native Halo2 verifier (include/gl355.h: gl355_bn254_g2_mul, gl355_bn254_pairing_check;
the check verify_proof ends in, chip/native_chip/test_utils.rs:82-93).  No second pairing implementation: the pairing is tested through
bilinearity, prod_i e(a_i G1, b_i G2) = 1 exactly when sum a_i b_i = 0 mod r, with the G1 multiples from tests/pymodel_bn254_curve.py and
the G2 arithmetic checked against an affine big-integer model of the twist written here."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pymodel_bn254_curve as pm  # noqa: E402

h2 = importlib.import_module("stark-verifier_amd.halo2")
_lib = importlib.import_module("stark-verifier_amd._lib")
Q, R = pm.Q, pm.R
E_INVALID_ARG = -1


# ---- Fq2 = Fq[u] / (u^2 + 1) and the twist y^2 = x^3 + 3 / (9 + u), affine, on Python integers ----------------------------------------
def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def f2_sqrt(a):
    """a square root of a in Fq2, or None (q = 3 mod 4: through the norm)"""
    if a == (0, 0):
        return (0, 0)
    norm = (a[0] * a[0] + a[1] * a[1]) % Q
    s = pow(norm, (Q + 1) // 4, Q)
    if s * s % Q != norm:
        return None
    for sign in (1, -1):
        t = (a[0] + sign * s) * pow(2, -1, Q) % Q
        x0 = pow(t, (Q + 1) // 4, Q)
        if x0 * x0 % Q == t and x0:
            r = (x0, a[1] * pow(2 * x0, -1, Q) % Q)
            if f2_mul(r, r) == a:
                return r
    return None


B_TWIST = f2_mul((3, 0), f2_inv((9, 1)))


def on_twist(p):
    return p is None or f2_sub(f2_mul(p[1], p[1]), f2_add(f2_mul(f2_mul(p[0], p[0]), p[0]), B_TWIST)) == (0, 0)


def g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if f2_add(p[1], q[1]) == (0, 0):
            return None
        lam = f2_mul(f2_mul((3, 0), f2_mul(p[0], p[0])), f2_inv(f2_add(p[1], p[1])))
    else:
        lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), p[0]), q[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(p[0], x3)), p[1]))


def g2_mul_model(p, k):
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, p)
        p = g2_add(p, p)
        k >>= 1
    return acc


def test_generator_is_on_the_twist_and_has_order_r():
    g = h2.G2_GENERATOR
    assert on_twist(g)
    assert g2_mul_model(g, R) is None                       # big-integer model
    assert h2.g2_mul(R) is None                             # the library
    assert h2.g2_mul(1) == g and h2.g2_mul(R + 1) == g
    assert h2.g2_mul(0) is None
    # include/gl355.h states the same four coordinates
    hdr = open(os.path.join(ROOT, "include", "gl355.h")).read()
    for c in (g[0][0], g[0][1], g[1][0], g[1][1]):
        assert "0x%064x" % c in hdr


def test_g2_mul_agrees_with_repeated_addition_and_composes():
    g = h2.G2_GENERATOR
    acc = None
    for k in range(1, 20):
        acc = g2_add(acc, g)
        assert h2.g2_mul(k) == acc, k
        assert on_twist(acc)
    rng = np.random.default_rng(21)
    for _ in range(6):
        a, b = (int.from_bytes(rng.bytes(32), "little") % R for _ in range(2))
        assert h2.g2_mul(a, h2.g2_mul(b)) == h2.g2_mul(a * b % R)
    a = int.from_bytes(rng.bytes(32), "little") % R
    assert h2.g2_mul(a) == g2_mul_model(g, a)
    assert h2.g2_mul(5, None) == h2.g2_mul(5) and h2.g2_mul(7, h2.g2_mul(R - 1)) == h2.g2_mul(R - 7)


def test_bilinearity():
    """20 tuples of length 1..4: the product of pairings is 1 exactly when sum a_i b_i = 0 (mod r); half are built to satisfy it"""
    rng = np.random.default_rng(0xB11)
    rnd = lambda: 1 + int.from_bytes(rng.bytes(32), "little") % (R - 1)      # noqa: E731
    for t in range(20):
        m = 1 + t % 4
        a = [rnd() for _ in range(m)]
        b = [rnd() for _ in range(m)]
        if t % 2 == 0:                                       # satisfy the relation
            if m == 1:
                b[0] = R                                     # the only way with one pair: a zero factor
            else:
                b[-1] = -sum(x * y for x, y in zip(a[:-1], b[:-1])) * pow(a[-1], -1, R) % R
        want = sum(x * y for x, y in zip(a, b)) % R == 0
        assert want == (t % 2 == 0)
        got = h2.pairing_check([pm.mul(pm.G, x) for x in a], [h2.g2_mul(y) for y in b])
        assert got == want, (t, m)
    # e(a G1, b G2) = e(ab G1, G2) = e(G1, ab G2), as two-pair products with one side negated
    a, b = rnd(), rnd()
    assert h2.pairing_check([pm.mul(pm.G, a), pm.mul(pm.G, (-a * b) % R)], [h2.g2_mul(b), h2.G2_GENERATOR])
    assert h2.pairing_check([pm.mul(pm.G, a), pm.G], [h2.g2_mul(b), h2.g2_mul((-a * b) % R)])
    assert not h2.pairing_check([pm.mul(pm.G, a), pm.G], [h2.g2_mul(b), h2.g2_mul((-a * b + 1) % R)])


def test_non_degeneracy_and_identities():
    assert not h2.pairing_check([pm.G], [h2.G2_GENERATOR])                  # e(G1, G2) != 1
    assert h2.pairing_check([], [])
    assert h2.pairing_check([None], [h2.G2_GENERATOR])                      # an identity on either side contributes 1
    assert h2.pairing_check([pm.G], [None])
    assert h2.pairing_check([None, pm.G, pm.mul(pm.G, 5), pm.mul(pm.G, R - 5)], [h2.g2_mul(3), None, h2.g2_mul(9), h2.g2_mul(9)])
    assert not h2.pairing_check([None, pm.G], [h2.g2_mul(3), h2.g2_mul(4)])


def twist_point_outside_the_subgroup():
    """the twist has cofactor 2q - r > 1: a point with a small x is (almost surely) not of order r"""
    for x0 in range(1, 200):
        x = (x0, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), B_TWIST))
        if y is None:
            continue
        p = (x, y)
        assert on_twist(p)
        if g2_mul_model(p, R) is not None:
            return p
    raise AssertionError("no such point found")


def test_rejections_are_error_codes():
    g1, g2 = pm.G, h2.G2_GENERATOR
    off_subgroup = twist_point_outside_the_subgroup()
    cases = {
        "G1 coordinate >= q": ([(g1[0] + Q, g1[1])], [g2]),
        "G1 y >= q": ([(g1[0], g1[1] + Q)], [g2]),
        "G1 off the curve": ([(1, 3)], [g2]),
        "G2 coordinate >= q": ([g1], [((g2[0][0] + Q, g2[0][1]), g2[1])]),
        "G2 coordinate (y.c1) >= q": ([g1], [(g2[0], (g2[1][0], g2[1][1] + Q))]),
        "G2 off the twist": ([g1], [(g2[0], ((g2[1][0] + 1) % Q, g2[1][1]))]),
        "twist point outside the subgroup": ([g1], [off_subgroup]),
        "second pair bad": ([g1, (1, 3)], [g2, g2]),
    }
    for name, (a, b) in cases.items():
        with pytest.raises(_lib.Gl355Error) as ei:
            h2.pairing_check(a, b)
        assert ei.value.code == E_INVALID_ARG, name
    with pytest.raises(_lib.Gl355Error) as ei:
        h2.pairing_check([g1, (1, 3)], [g2, g2])
    assert "pair 1" in str(ei.value)
    # g2_mul wants a point of the twist (any subgroup), and says so without crashing
    assert on_twist(h2.g2_mul(3, off_subgroup))
    with pytest.raises(_lib.Gl355Error) as ei:
        h2.g2_mul(3, (g2[0], ((g2[1][0] + 1) % Q, g2[1][1])))
    assert ei.value.code == E_INVALID_ARG
    # null arguments are codes too
    lib = _lib.load()
    assert lib.gl355_bn254_pairing_check(None, None, 1, None) == E_INVALID_ARG
    assert lib.gl355_bn254_g2_mul(None, None, None) == E_INVALID_ARG
