"""CPU: the G1 FFT entries (gl355_bn254_g1_fft, gl355_kzg_lagrange_from_powers) are declared, exported and bound, refuse without a
context by an error code, and the kernels' schedule -- bit-reversed load, decimation-in-time stages with twiddle w_n^(j n / 2^s), the
4-bit signed-digit recoding of each twiddle, the 1/n of the inverse -- restated over Fr scalars equals the DFT by its definition.  The map
s -> [s] G is a homomorphism, so a schedule that is right on scalars is right on points."""
import os
import re

import numpy as np
import pytest

import pymodel_bn254_curve as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gl355_bn254_g1_fft", "gl355_kzg_lagrange_from_powers")


def test_entries_declared_exported_and_bound(gl):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gl355.h")).read(), flags=re.S)
    lib = gl._lib.load()
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in gl._lib.SIGNATURES, name
    full = open(os.path.join(ROOT, "include", "gl355.h")).read()
    assert "gl355_kzg_lagrange_from_powers" in full and "verifier_api.rs:77" in full


def test_refusals_without_a_context_are_error_codes(gl):
    lib = gl._lib.load()
    pts = np.zeros((8, 8), dtype=np.uint64)
    out = np.zeros((8, 8), dtype=np.uint64)
    assert lib.gl355_bn254_g1_fft(None, pts.ctypes.data, 3, 0) == -1                        # GL355_E_INVALID_ARG
    assert lib.gl355_bn254_g1_fft(None, pts.ctypes.data, 3, 1) == -1
    assert lib.gl355_kzg_lagrange_from_powers(None, pts.ctypes.data, 8, 3, out.ctypes.data) == -1
    assert not out.any()


def test_no_device_is_an_error_code(gl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gl.Gl355Error):
        gl.Context(0)
    h2 = __import__("importlib").import_module("stark-verifier_amd.halo2")
    assert callable(h2.g1_fft) and callable(h2.kzg_lagrange_from_powers)


# ---- the kernels' schedule over scalars (bn254_g1_fft.hip) -------------------------------------------------------------------------
WIN, WINDOWS = 4, 64


def signed_digits(k):
    """g1_mul_signed_window's recoding: (top digit, [(magnitude, negative)] for windows 63 .. 0)"""
    neg, c = [], 0
    for i in range(WINDOWS):
        raw = ((k >> (4 * i)) & 15) + c
        c = 1 if raw >= 8 else 0
        neg.append(c)
    digits = []
    for i in range(WINDOWS - 1, -1, -1):
        cin = neg[i - 1] if i else 0
        raw = ((k >> (4 * i)) & 15) + cin
        digits.append((16 - raw if neg[i] else raw, bool(neg[i])))
    return c, digits


def mul_by_schedule(p, k):
    """[k] p in the additive group Z_r, step by step as the kernel does it: the table d p (d <= 8), four doublings and one addition of
    +-table[d] per window"""
    tab = [d * p % pm.R for d in range(9)]
    top, digits = signed_digits(k)
    acc = p if top else 0
    for mag, negative in digits:
        assert 0 <= mag <= 8
        for _ in range(WIN):
            acc = 2 * acc % pm.R
        acc = (acc + (-tab[mag] if negative else tab[mag])) % pm.R
    return acc


def g1_fft_by_schedule(vals, inverse):
    n = len(vals)
    log_n = n.bit_length() - 1
    w = pm.omega(log_n, inverse) if log_n else 1
    tw = [pow(w, i, pm.R) for i in range(max(1, n // 2))]
    data = [vals[int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0] for i in range(n)]       # load pass
    for s in range(1, log_n + 1):                                                                  # stage kernels
        half = 1 << (s - 1)
        for t in range(n // 2):
            j, base = t & (half - 1), (t >> (s - 1)) << s
            u, v = data[base + j], data[base + j + half]
            if j:
                v = mul_by_schedule(v, tw[j << (log_n - s)])
            data[base + j], data[base + j + half] = (u + v) % pm.R, (u - v) % pm.R
    if inverse and log_n:                                                                          # store pass
        ninv = pow(n, -1, pm.R)
        data = [mul_by_schedule(x, ninv) for x in data]
    return data


def test_signed_digits_reconstruct_the_scalar():
    rng = np.random.default_rng(7)
    cases = [0, 1, 7, 8, 15, 16, (1 << 256) - 1, 0x8888 << 200, pm.R - 1, pm.Q - 1]
    cases += [int.from_bytes(rng.bytes(32), "little") for _ in range(200)]
    for k in cases:
        top, digits = signed_digits(k)
        v = top
        for mag, negative in digits:
            assert 0 <= mag <= 8
            v = 16 * v + (-mag if negative else mag)
        assert v == k, hex(k)
        assert mul_by_schedule(3, k % (1 << 256)) == 3 * k % pm.R


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 8])
@pytest.mark.parametrize("inverse", [False, True])
def test_schedule_over_scalars_equals_the_dft(log_n, inverse):
    rng = np.random.default_rng(100 + log_n)
    vals = [int.from_bytes(rng.bytes(32), "little") % pm.R for _ in range(1 << log_n)]
    assert g1_fft_by_schedule(vals, inverse) == pm.dft(vals, inverse)


def test_inverse_of_the_powers_is_the_lagrange_basis():
    """what gl355_kzg_lagrange_from_powers relies on: inverse DFT of (tau^i) = (L_i(tau)) as gl355_kzg_setup evaluates them"""
    log_n, tau = 4, 0x1234567890ABCDEF % pm.R
    n, w = 1 << log_n, pm.omega(4)
    got = g1_fft_by_schedule([pow(tau, i, pm.R) for i in range(n)], True)
    c = (pow(tau, n, pm.R) - 1) * pow(n, -1, pm.R) % pm.R
    assert got == [c * pow(w, i, pm.R) * pow(tau - pow(w, i, pm.R), -1, pm.R) % pm.R for i in range(n)]
