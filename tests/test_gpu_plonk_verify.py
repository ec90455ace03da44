"""GPU: the native Halo2 verifier through the C ABI (gl355_plonk_vk_from_pk / gl355_plonk_verify / _verify_batch, gl355_kzg_params_check:
verify_proof with VerifierSHPLONK as chip/native_chip/test_utils.rs:82-93 runs it on every proof) on proofs gl355_plonk_prove makes --
accepted under [tau] G2 with and without a context, one verdict with the restated verifier on bad inputs, the ceremony case (nobody keeps the
secret) end to end, batches with the combined MSM on the host and on the device, and the parameter-set check at k = 16.  Bad inputs here
are ordinary malformed data the code rejects with a verdict."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import halo2_model as hm  # noqa: E402
import halo2_verifier as hv  # noqa: E402
from halo2_circuits import plonk_with_tuple_lookup, random_circuit  # noqa: E402
from halo2_mutations import mutations  # noqa: E402

pytestmark = pytest.mark.gpu
h2 = importlib.import_module("stark-verifier_amd.halo2")
ch = importlib.import_module("stark-verifier_amd.halo2_chips")
TAU = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF % hm.R
R = hm.R


def pt(a):
    x, y = h2.from_limbs(a[:4])[0], h2.from_limbs(a[4:])[0]
    return None if (x, y) == (0, 0) else (x, y)


@pytest.fixture(scope="module")
def s_g2():
    return h2.kzg_setup_g2(TAU)


def circuit(kind, k):
    if kind == "chip":
        cs, cfg, w = ch.synthetic_circuit(k, table_bits=min(k - 2, 9), n_permutations=1)
        return cs, w
    if kind == "tuple":
        return plonk_with_tuple_lookup(k, 5, seed=100)
    return random_circuit(k, k)


class Keyed:
    """one circuit keyed under gl355_kzg_setup(TAU): the prover, its verifying key under [TAU] G2 and one proof"""

    def __init__(self, ctx, s_g2, srs, kind, k):
        self.cs, self.w = circuit(kind, k)
        self.prover = h2.PlonkProver(ctx, self.cs, k, srs[0], srs[1], self.w.fixed, self.w.assembly.mapping_array())
        self.vk = self.prover.verifying_key(s_g2)
        self.proof = self.prover.prove(self.w.advice, self.w.instance, bytes(range(32)))

    def close(self):
        self.vk.close()
        self.prover.close()


@pytest.fixture(scope="module")
def keys(ctx, s_g2):
    """keys(kind, k) -> Keyed, made on first use and kept for the module (one parameter set per k)"""
    srs, made = {}, {}

    def get(kind, k):
        if k not in srs:
            srs[k] = h2.kzg_setup(ctx, k, TAU)
        if (kind, k) not in made:
            made[kind, k] = Keyed(ctx, s_g2, srs[k], kind, k)
        return made[kind, k]
    yield get
    for key in made.values():
        key.close()


@pytest.fixture
def device_msm(monkeypatch):
    """the batch verifier's MSMs on the device whatever their size (include/gl355.h: GL355_PLONK_VERIFY_DEVICE_MSM_MIN)"""
    monkeypatch.setenv("GL355_PLONK_VERIFY_DEVICE_MSM_MIN", "0")


@pytest.mark.parametrize("k", range(7, 13))
@pytest.mark.parametrize("kind", ["chip", "random"])
def test_product_proofs_verify(ctx, s_g2, keys, kind, k):
    key = keys(kind, k)
    cs, w, prover, vk, proof = key.cs, key.w, key.prover, key.vk, key.proof
    assert vk.verify(w.instance, proof, ctx=ctx), vk.last_error
    assert vk.verify(w.instance, proof, ctx=None), vk.last_error
    # the key rebuilt from its public parts (descriptor, commitments; the digest by keygen's rule) is the same key
    again = h2.PlonkVerifier(cs, k, prover.fixed_commitments, prover.sigma_commitments, s_g2)
    assert again.verify(w.instance, proof)
    again.close()
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 4
    assert vk.verify(w.instance, bytes(bad), ctx=ctx) is False and vk.verify(w.instance, bytes(bad), ctx=None) is False
    assert vk.last_error


@pytest.mark.parametrize("kind", ["chip", "tuple"])
def test_keygen_and_vk_create_derive_one_digest(ctx, s_g2, keys, kind):
    """a zero digest field: gl355_plonk_pk_digest after keygen == vk_digest over the key's own commitments == what gl355_plonk_vk_create
    derives from the same descriptor and commitments (one rule, csrc/plonk_desc.h).  The verifying key keeps its digest to itself, so the
    last is read off its verdicts: the proof verifies under the key from the proving key, under the key made with no digest argument and
    under the one given vk_digest, and not under the one given another digest"""
    k = 7
    key = keys(kind, k)
    cs, w, prover, proof = key.cs, key.w, key.prover, key.proof
    assert not prover.desc[16:20].any()
    digest = h2.vk_digest(cs, k, prover.fixed_commitments, prover.sigma_commitments, hv.keccak256)
    assert prover.digest == digest
    assert key.vk.verify(w.instance, proof), key.vk.last_error                       # gl355_plonk_vk_from_pk
    for given, want in ((None, True), (digest, True), ((digest + 1) % R, False)):
        made = h2.PlonkVerifier(cs, k, prover.fixed_commitments, prover.sigma_commitments, s_g2, digest=given)      # gl355_plonk_vk_create
        assert made.verify(w.instance, proof) is want, (given, made.last_error)
        made.close()


def test_verdicts_equal_the_restated_verifier(ctx, keys):
    k = 7
    key = keys("random", k)
    cs, w, prover, vk, proof = key.cs, key.w, key.prover, key.vk, key.proof
    pvk = dict(digest=prover.digest, fixed_commitments=[pt(c) for c in prover.fixed_commitments], sigma_commitments=[pt(c) for c in prover.sigma_commitments])
    rejected = 0
    for what, inst, bad in [("valid", w.instance, proof)] + mutations(cs, w.instance, proof):
        try:
            want = hv.verify(k, cs, pvk, inst, bad, TAU)
        except hv.VerifyError:
            want = False
        got = vk.verify(inst, bad, ctx=ctx)
        assert got == want, (what, vk.last_error)
        rejected += not got
    assert rejected >= 7


def test_noncanonical_instance_is_a_malformed_call(ctx, keys):
    """public values are canonical integers like every scalar of the ABI: r itself in an instance cell is an error code, not a verdict"""
    import ctypes as C
    key = keys("tuple", 7)
    flat, lens = key.vk._instances(key.w.instance)
    assert len(flat) >= 1
    flat = flat.copy()
    flat[:4] = h2._raw_limbs([R])
    lens = np.array(lens + [0], dtype=np.uint32)
    ok = C.c_int32(1)
    rc = key.vk.lib.gl355_plonk_verify(ctx.h, key.vk.h, flat.ctypes.data, lens.ctypes.data, key.proof, len(key.proof), C.byref(ok))
    assert rc == -1 and ok.value == 0 and "instance" in key.vk.last_error
    ptrs = (C.c_char_p * 1)(key.proof)
    plens = np.array([len(key.proof)], dtype=np.uint64)
    ok = C.c_int32(1)
    rc = key.vk.lib.gl355_plonk_verify_batch(ctx.h, key.vk.h, 1, flat.ctypes.data, lens.ctypes.data, ptrs, plens.ctypes.data, bytes(32), C.byref(ok), None)
    assert rc == -1 and ok.value == 0


def test_ceremony_parameters_end_to_end(ctx):
    """powers of tau whose secret is thrown away: Lagrange bases by the G1 FFT, the set checked, a proof made and verified under [tau] G2"""
    k = 10
    tau = int.from_bytes(os.urandom(32), "little") % R
    g, _ = h2.kzg_setup(ctx, k, tau, lagrange=False)
    s_g2 = h2.kzg_setup_g2(tau)
    other_s_g2 = h2.kzg_setup_g2((tau + 1) % R)
    del tau
    g_lagrange = h2.kzg_lagrange_from_powers(ctx, g, k)
    assert h2.kzg_params_check(ctx, g, s_g2, k, g_lagrange=g_lagrange)
    cs, w = circuit("chip", k)
    prover = h2.PlonkProver(ctx, cs, k, g, g_lagrange, w.fixed, w.assembly.mapping_array())
    proof = prover.prove(w.advice, w.instance, bytes(range(32)))
    vk = prover.verifying_key(s_g2)
    assert vk.verify(w.instance, proof), vk.last_error
    assert vk.verify(w.instance, proof, ctx=ctx)
    wrong = prover.verifying_key(other_s_g2)
    assert wrong.verify(w.instance, proof) is False
    assert not h2.kzg_params_check(ctx, g, other_s_g2, k, g_lagrange=g_lagrange)
    prover.close()


@pytest.fixture(scope="module")
def batch_of_32(keys):
    """32 proofs under one key (fixed columns, copy constraints), each with its own witness, instances and blinding seed"""
    key = keys("tuple", 7)
    insts, proofs = [], []
    for b in range(32):
        _, w = plonk_with_tuple_lookup(7, 5, seed=100 + b)
        assert np.array_equal(w.fixed, key.w.fixed)
        insts.append(w.instance)
        proofs.append(key.prover.prove(w.advice, w.instance, bytes([b]) * 32))
    assert len({tuple(i[0]) for i in insts}) == 32 and len(set(proofs)) == 32
    return key.vk, insts, proofs


SEEDS = (bytes(32), bytes([0xA5]) * 32)


def check_batch(ctx, vk, insts, proofs, bad_index):
    """true as it stands; false with first_bad = bad_index once that proof has one evaluation changed (still well-formed, so it is the pairing
    product that fails and the fallback that finds it); the same with a context, without one, and for two seeds"""
    for seed in SEEDS:
        assert vk.verify_batch(ctx, insts, proofs, seed=seed, want_first_bad=True) == (True, -1), vk.last_error
        assert vk.verify_batch(None, insts, proofs, seed=seed, want_first_bad=True) == (True, -1), vk.last_error
    assert vk.verify_batch(ctx, insts, proofs) is True                  # weights from the OS's generator
    bad = bytearray(proofs[bad_index])
    bad[-129] ^= 1
    mixed = proofs[:bad_index] + [bytes(bad)] + proofs[bad_index + 1:]
    for seed in SEEDS:
        assert vk.verify_batch(ctx, insts, mixed, seed=seed, want_first_bad=True) == (False, bad_index)
        assert vk.verify_batch(None, insts, mixed, seed=seed, want_first_bad=True) == (False, bad_index)
        assert vk.verify_batch(ctx, insts, mixed, seed=seed) is False
    assert "pairing" in vk.last_error


def test_verify_batch_of_32(ctx, batch_of_32):
    """about 500 terms in the combined MSM: on the device with a context (on the host without one), the 32-term h2 sum on the host"""
    check_batch(ctx, *batch_of_32, bad_index=17)


def test_verify_batch_of_32_device_msm(ctx, batch_of_32, device_msm):
    """the same batch with both MSMs (about 500 terms with 128-bit-weighted scalars and the key's points; 32 terms of 128 bits) on the device:
    verdict and first_bad as on the host (ctx = None takes the host sum whatever the threshold)"""
    check_batch(ctx, *batch_of_32, bad_index=17)
    vk, insts, proofs = batch_of_32
    assert vk.verify_batch(ctx, insts[:1], proofs[:1], seed=SEEDS[1], want_first_bad=True) == (True, -1)        # a one-term h2 sum
    assert vk.verify_batch(ctx, insts[:2], proofs[:2][::-1], seed=SEEDS[1], want_first_bad=True) == (False, 0)   # proofs against the other's instances


def test_verify_batch_chip_shape_reaches_the_device(ctx, keys):
    """enough proofs of the reference's chip shape (57 points each, other blinding seeds) to pass PLONK_VERIFY_DEVICE_MSM_MIN, read from
    csrc/plonk_verifier.cpp: with a context the combined MSM runs on the device without any override"""
    src = open(os.path.join(ROOT, "stark-verifier_amd", "csrc", "plonk_verifier.cpp")).read()
    device_min = int(re.search(r"constexpr uint64_t PLONK_VERIFY_DEVICE_MSM_MIN = (\d+);", src).group(1))
    key = keys("chip", 7)
    cl = key.cs.chunk_len()
    per_proof = key.cs.num_advice + 3 * len(key.cs.lookups) + (len(key.cs.permutation) + cl - 1) // cl + 1 + (key.cs.degree() - 1) + 2
    n = max(8, -(-device_min // per_proof) + 2)
    assert n <= 128, "the device threshold has outgrown this test"
    proofs = [key.prover.prove(key.w.advice, key.w.instance, bytes([b, 0x5A]) * 16) for b in range(n)]
    assert len(set(proofs)) == n
    check_batch(ctx, key.vk, [key.w.instance] * n, proofs, bad_index=n - 3)


def test_kzg_params_check_k16(ctx, s_g2):
    k = 16
    g, gl_ = h2.kzg_setup(ctx, k, TAU)
    seed = bytes(range(32))
    assert h2.kzg_params_check(ctx, g, s_g2, k, g_lagrange=gl_, seed=seed)
    assert h2.kzg_params_check(ctx, g, s_g2, k, seed=seed)               # the powers alone
    assert h2.kzg_params_check(ctx, g, s_g2, k - 2, g_lagrange=h2.kzg_lagrange_from_powers(ctx, g, k - 2))        # a downsized set
    import pymodel_bn254_curve as pm
    doubled = g.copy()
    doubled[5] = h2.g1_words(pm.add(pt(g[5]), pt(g[5])))
    swapped = g.copy()
    swapped[[9, 10]] = swapped[[10, 9]]
    lag_swapped = gl_.copy()
    lag_swapped[[3, 4]] = lag_swapped[[4, 3]]
    off_curve = g.copy()
    off_curve[7, 4] += 1
    cases = {
        "g[5] doubled": (doubled, gl_, s_g2),
        "two powers swapped": (swapped, gl_, s_g2),
        "two Lagrange bases swapped": (g, lag_swapped, s_g2),
        "s_g2 of another tau": (g, gl_, h2.kzg_setup_g2(TAU + 1)),
        "a point off the curve": (off_curve, gl_, s_g2),
        "g[0] the identity": (np.concatenate([np.zeros((1, 8), dtype=np.uint64), g[1:]]), gl_, s_g2),
    }
    for name, (gg, ll, s2) in cases.items():
        assert h2.kzg_params_check(ctx, gg, s2, k, g_lagrange=ll, seed=seed) is False, name
