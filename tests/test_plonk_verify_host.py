"""CPU: the native Halo2 verifier (gl355_plonk_vk_create / gl355_plonk_verify, csrc/plonk_verifier.cpp: verify_proof with VerifierSHPLONK
as chip/native_chip/test_utils.rs:82-93 runs it) against the restated one (tests/halo2_verifier.py).  Proofs and keys come from the CPU
prover restatement (oracle/halo2_model.py) over the circuits of tests/halo2_circuits.py; the native verifier gets [tau] G2 and never tau."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import halo2_model as hm  # noqa: E402
import halo2_verifier as hv  # noqa: E402
from halo2_circuits import oracle_vk_digest, plonk_with_tuple_lookup, points_to_words, random_circuit  # noqa: E402
from halo2_mutations import mutations  # noqa: E402

h2 = importlib.import_module("stark-verifier_amd.halo2")
ch = importlib.import_module("stark-verifier_amd.halo2_chips")
TAU = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF % hm.R


def chip_shape(k):
    cs, cfg, w = ch.synthetic_circuit(k, table_bits=5, n_permutations=1)
    return cs, w


CIRCUITS = {
    "chip_shape": lambda: (7, chip_shape(7)),
    "tuple_lookup": lambda: (7, plonk_with_tuple_lookup(7, 5)),
    "random0": lambda: (6, random_circuit(6, 0)),
    "random1": lambda: (7, random_circuit(7, 1)),
    "random2": lambda: (6, random_circuit(6, 2)),
    "random3": lambda: (7, random_circuit(7, 3)),
}
_cache = {}


def case(name):
    """(k, cs, witness, vk dict of the restated verifier, proof, native verifier under [tau] G2)"""
    if name not in _cache:
        k, (cs, w) = CIRCUITS[name]()
        params = hm.Params(k, TAU)
        pk = hm.keygen(params, cs, w.fixed_ints(), w.assembly)
        digest = oracle_vk_digest(cs, k, pk)
        proof = hm.create_proof(params, pk, w.advice_ints(), w.instance, bytes(range(32)), digest)
        vk = dict(digest=digest, fixed_commitments=pk.fixed_commitments, sigma_commitments=pk.sigma_commitments)
        native = h2.PlonkVerifier(cs, k, points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments), h2.kzg_setup_g2(TAU))
        _cache[name] = (k, cs, w, vk, proof, native, pk)
    return _cache[name]


def restated(k, cs, vk, instances, proof):
    try:
        return hv.verify(k, cs, vk, instances, proof, TAU)
    except hv.VerifyError:
        return False


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_every_proof_verifies_on_the_host(name):
    k, cs, w, vk, proof, native, pk = case(name)
    assert native.verify(w.instance, proof, ctx=None), native.last_error
    assert native.last_error == ""
    assert restated(k, cs, vk, w.instance, proof)
    # the digest the key derives itself (pinned-key Keccak rule) is the checker's; given explicitly it is the same key
    explicit = h2.PlonkVerifier(cs, k, points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments), h2.kzg_setup_g2(TAU), digest=vk["digest"])
    assert explicit.verify(w.instance, proof)
    other = h2.PlonkVerifier(cs, k, points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments), h2.kzg_setup_g2(TAU), digest=vk["digest"] + 1)
    assert not other.verify(w.instance, proof)


@pytest.mark.parametrize("name,every", [("random0", 1), ("tuple_lookup", 1), ("chip_shape", 8)])
def test_verdict_equals_the_restated_verifier(name, every):
    """the valid proof and every mutation of tests/halo2_mutations.py: one verdict from both verifiers, and the native one names a step"""
    k, cs, w, vk, proof, native, pk = case(name)
    rejected = 0
    for what, inst, bad in [("valid", w.instance, proof)] + mutations(cs, w.instance, proof, every):
        want = restated(k, cs, vk, inst, bad)
        got = native.verify(inst, bad)
        assert got == want, (what, native.last_error)
        assert (native.last_error == "") == got
        rejected += not got
    assert rejected >= 7


def test_wrong_s_g2_rejects_a_valid_proof():
    k, cs, w, vk, proof, native, pk = case("random0")
    wrong = h2.PlonkVerifier(cs, k, points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments), h2.kzg_setup_g2(TAU + 1))
    assert not wrong.verify(w.instance, proof)
    assert "pairing" in wrong.last_error
    assert native.verify(w.instance, proof)


def test_batch_on_the_host():
    """verify_batch with ctx=None: the same code path as on the device but for where the MSM runs"""
    k, cs, w, vk, proof, native, pk = case("random0")
    params = hm.Params(k, TAU)
    proofs = [proof] + [hm.create_proof(params, pk, w.advice_ints(), w.instance, bytes([s]) * 32, vk["digest"]) for s in (1, 2, 3)]
    insts = [w.instance] * 4
    assert native.verify_batch(None, insts, proofs, seed=bytes(32))
    assert native.verify_batch(None, insts, proofs, seed=bytes([7]) * 32, want_first_bad=True) == (True, -1)
    assert native.verify_batch(None, insts, proofs)                     # seed from the OS
    assert native.verify_batch(None, [], [])
    bad = bytearray(proofs[2])
    bad[-70] ^= 1                                                       # a bit of h1: off the curve or another point, proof 2 is the bad one either way
    for seed in (bytes(32), bytes([9]) * 32):
        assert native.verify_batch(None, insts, proofs[:2] + [bytes(bad)] + proofs[3:], seed=seed, want_first_bad=True) == (False, 2)
    # a proof that is valid for other instances fails the pairing, not the parsing
    if w.instance and w.instance[0]:
        changed = [list(c) for c in w.instance]
        changed[0][0] = (changed[0][0] + 1) % hm.R
        assert native.verify_batch(None, [w.instance, changed, w.instance, w.instance], proofs, seed=bytes(32), want_first_bad=True) == (False, 1)
        assert "proof 1" in native.last_error


def test_malformed_calls_are_error_codes():
    _lib = importlib.import_module("stark-verifier_amd._lib")
    k, cs, w, vk, proof, native, pk = case("random0")
    fc, sc = points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments)
    with pytest.raises(_lib.Gl355Error):                                 # s_g2 off the twist
        g = h2.G2_GENERATOR
        h2.PlonkVerifier(cs, k, fc, sc, (g[0], (g[1][0] + 1, g[1][1])))
    with pytest.raises(_lib.Gl355Error):                                 # the identity is no parameter set
        h2.PlonkVerifier(cs, k, fc, sc, None)
    bad_fc = fc.copy()
    bad_fc[0, 4] += 1
    with pytest.raises(_lib.Gl355Error):                                 # a key commitment off the curve
        h2.PlonkVerifier(cs, k, bad_fc, sc, h2.kzg_setup_g2(TAU))
    lib = _lib.load()
    assert lib.gl355_plonk_verify(None, None, None, None, None, 0, None) == -1
    assert lib.gl355_plonk_vk_create(None, 0, None, None, None, None, None) == -1
    # public values are canonical integers like every scalar of the ABI: r in an instance cell is a malformed call, r - 1 is not
    import ctypes as C
    k, cs, w, vk, proof, native, pk = case("tuple_lookup")
    cols = [len(c) for c in w.instance]
    assert sum(cols)
    lens = np.array(cols + [0], dtype=np.uint32)
    for value, want_rc in ((hm.R, -1), (hm.R - 1, 0)):
        flat = h2._raw_limbs([value] + [0] * (sum(cols) - 1))
        ok = C.c_int32(1)
        assert lib.gl355_plonk_verify(None, native.h, flat.ctypes.data, lens.ctypes.data, proof, len(proof), C.byref(ok)) == want_rc
        assert ok.value == 0
    assert not native.verify(w.instance, proof[:100]) and native.stage_ms() == dict(host=0.0, msm=0.0, pairing=0.0)       # nothing stale
    # an empty and a truncated proof are verdicts
    k, cs, w, vk, proof, native, pk = case("random0")
    assert not native.verify(w.instance, b"")
    assert not native.verify(w.instance, proof[:100])


def test_malformed_descriptors_are_error_codes():
    """the mutation list of tests/plonk_desc_cases.py through gl355_plonk_vk_create: -1 and the parser's text (csrc/plonk_desc.h) for every
    refusal, a key for everything else; k = 28 is a verifier's circuit, k = 29 is not; the digest the key derives is vk_digest"""
    import ctypes as C
    import plonk_desc_cases as pdc
    _lib = importlib.import_module("stark-verifier_amd._lib")
    lib = _lib.load()
    s_g2 = h2.g2_words(h2.kzg_setup_g2(TAU))
    for name in ("random0", "tuple_lookup"):
        k, cs, w, vk, proof, native, pk = case(name)
        desc = [int(x) for x in h2.export_desc(cs, k, 0)]
        # a mutated header may claim up to 256 columns of either kind: the identity stands for the ones the key does not have
        fc, sc = np.zeros((256, 8), dtype=np.uint64), np.zeros((256, 8), dtype=np.uint64)
        fc[:cs.num_fixed], sc[:len(cs.permutation)] = points_to_words(pk.fixed_commitments), points_to_words(pk.sigma_commitments)

        def create(words, digest=None):
            a, h = np.array(list(words) + [0], dtype=np.uint64), C.c_void_p()
            d = None if digest is None else h2.to_limbs([digest])[0]
            rc = lib.gl355_plonk_vk_create(a.ctypes.data, len(words), fc.ctypes.data, sc.ctypes.data, None if d is None else d.ctypes.data, s_g2.ctypes.data, C.byref(h))
            assert (rc == 0) == bool(h.value)
            return rc, (lib.gl355_plonk_verify_last_error() or b"").decode(), h
        answers = {}
        for what, m in pdc.mutations(desc, pdc.MAX_K_VERIFIER):
            want = "null or truncated argument" if len(m) < pdc.HDR else pdc.verdict(m, pdc.MAX_K_VERIFIER)      # the entry's own pre-check comes first
            rc, msg, h = create(m)
            if rc == 0:
                lib.gl355_plonk_vk_destroy(h)
            assert (rc, msg) == ((-1, "plonk_vk_create: " + want) if want else (0, msg)), what
            answers[what] = rc
        assert answers["header word 2 = 28"] == 0 and answers["header word 2 = 29"] == -1
        assert sum(1 for rc in answers.values() if rc == 0) > 200 and sum(1 for rc in answers.values() if rc) > 300
        # no digest argument and a zero digest field: the transcript starts from vk_digest -- the proof made under it verifies, as it does
        # under the key that is given that digest, and no longer under a key that is given another
        digest = h2.vk_digest(cs, k, fc[:cs.num_fixed], sc[:len(cs.permutation)], hv.keccak256)
        assert digest == vk["digest"]
        for given, want in ((None, True), (digest, True), (digest + 1, False)):
            rc, msg, h = create(desc, given)
            assert rc == 0, msg
            key = h2.PlonkVerifier(cs, k, None, None, None, _handle=h)
            assert key.verify(w.instance, proof) == want, given
            key.close()


def test_no_new_export_takes_the_secret():
    """the verifier's exports see [s] G2 only: no parameter of a new entry is called tau (or secret), and the new sources never name one"""
    hdr = open(os.path.join(ROOT, "include", "gl355.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    new = ["gl355_bn254_g2_mul", "gl355_bn254_pairing_check", "gl355_plonk_vk_create", "gl355_plonk_vk_from_pk", "gl355_plonk_vk_destroy", "gl355_plonk_verify",
           "gl355_plonk_verify_batch", "gl355_plonk_verify_last_error", "gl355_plonk_verify_stage_ms", "gl355_kzg_params_check"]
    for name in new:
        m = re.search(r"\b%s\s*\(([^;]*)\);" % name, code)
        assert m, name
        assert not re.search(r"\b(tau|secret|toxic)\b", m.group(1), flags=re.I), name
    for src in ("plonk_verifier.cpp", "host_bn254_pairing.cpp"):
        text = open(os.path.join(ROOT, "stark-verifier_amd", "csrc", src)).read()
        assert not re.search(r"\btau\b", text), src
