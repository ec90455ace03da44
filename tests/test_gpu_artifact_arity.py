"""GPU: circuit artifacts that carry their FRI arities (versions 4 / 5: export_blob(..., wide_arity=True) -> gl355_circuit_load).  The
small gate-zoo circuit (fri_arity_cases.small_circuit, degree 2^6, 3 queries, cap height 1) at own arities [3], [2, 3], [1, 3] and [4]:
the loaded circuit reports the arities and the proof length of its CircuitData, its proofs are byte-identical to gl355_prove_sparse
of the same data and seed, single and in lock-step, and gl355_circuit_verify, CircuitData.verify and the model verifier agree on
them and on their mutations.  The loader refuses every malformed table by name and leaves the context usable."""
import importlib

import numpy as np
import pytest

import fri_arity_cases as fc

pytestmark = pytest.mark.gpu

ARITIES = [[3], [2, 3], [1, 3], [4]]
HDR = 112
INVALID_ARG, UNSUPPORTED, VERIFY = -1, -5, -7
_cases = {}


def case(ctx, arities):
    """the circuit built on the device, three witnesses of it, its version-4 artifact loaded"""
    key = str(arities)
    if key not in _cases:
        plonk = importlib.import_module("stark-verifier_amd.plonk")
        cfg = fc.config_of(plonk, reduction_arity_bits=arities, zero_knowledge=False, cap_height=1)
        builders = [fc.small_circuit(cfg, 0xB50 + u) for u in range(3)]
        data = builders[0][0].cb.build(ctx, np.random.default_rng(0xB5), min_degree_bits=6)
        wit = [b.sparse_witness() for b, _ in builders]
        idx = wit[0][0]
        assert all(np.array_equal(w[0], idx) for w in wit)
        blob = data.export_blob(idx, wide_arity=True)
        _cases[key] = dict(plonk=plonk, data=data, idx=idx, rows=np.stack([w[1] for w in wit]), pis=np.stack([pi for _, pi in builders]),
                           blob=blob, nat=plonk.NativeCircuit(ctx, blob))
    return _cases[key]


@pytest.mark.parametrize("arities", ARITIES, ids=str)
def test_the_loaded_circuit_reports_its_arities_and_proves_the_same_bytes(gl, ctx, arities):
    c = case(ctx, arities)
    plonk, data, nat = c["plonk"], c["data"], c["nat"]
    assert data.fri_arity_bits == arities and data.degree_bits == 6
    assert int(c["blob"][1]) == 4 and [int(a) for a in c["blob"][HDR:HDR + len(arities)]] == arities
    assert nat.fri_arity_bits == arities
    flat = plonk.prove_sparse(ctx, data, c["idx"], c["rows"][0], c["pis"][0], 0xB60, flat_only=True)
    assert nat.proof_words == flat.size == int(flat[0])
    assert np.array_equal(nat.prove_rows(ctx, c["rows"][0], c["pis"][0], 0xB60), flat)


@pytest.mark.parametrize("arities", ARITIES, ids=str)
def test_three_lock_step_units_equal_three_single_proofs(gl, ctx, arities):
    c = case(ctx, arities)
    plonk, nat = c["plonk"], c["nat"]
    seeds = [0xB60, 0xB61, 0xB62]
    flats = np.empty((3, nat.proof_words), dtype=np.uint64)
    keys = b"".join(plonk.key_bytes(s) for s in seeds)
    rows, pis = np.ascontiguousarray(c["rows"]), np.ascontiguousarray(c["pis"])
    ctx.check(ctx.lib.gl355_circuit_prove_rows_units(ctx.h, nat.h, 3, rows.ctypes.data, pis.ctypes.data, pis.shape[1], keys, flats.ctypes.data))
    for u in range(3):
        assert np.array_equal(flats[u], nat.prove_rows(ctx, rows[u], pis[u], seeds[u])), u
        assert np.array_equal(flats[u], plonk.prove_sparse(ctx, c["data"], c["idx"], rows[u], pis[u], seeds[u], flat_only=True)), u


@pytest.mark.parametrize("arities", ARITIES, ids=str)
def test_the_three_verifiers_agree_on_the_proof_and_its_mutations(gl, ctx, orc, arities):
    c = case(ctx, arities)
    plonk, data, nat = c["plonk"], c["data"], c["nat"]
    pi = np.ascontiguousarray(c["pis"][0])
    flat = nat.prove_rows(ctx, c["rows"][0], pi, 0xB60)

    def native_verify(f):
        f = np.ascontiguousarray(f, dtype=np.uint64)
        return ctx.lib.gl355_circuit_verify(nat.h, f.ctypes.data, f.size, pi.ctypes.data, pi.size)
    assert native_verify(flat) == 0
    assert fc.verdicts(orc, gl, plonk, data, flat, pi) == (None, None)
    seen = 0
    for name, bad, want in fc.mutations(data.common(), flat):
        assert native_verify(bad) == VERIFY, name
        assert (ctx.lib.gl355_verify_last_error() or b"").decode().endswith(fc.C_CHECKS[want.split()[0]]), name
        c_check, m_check = fc.verdicts(orc, gl, plonk, data, bad, pi)
        assert m_check == want and c_check == want.split()[0], name
        seen += 1
    assert seen == 4


def test_blinding_rows_follow_the_artifact_too(gl, ctx):
    """zero-knowledge on: the blinding-row counts depend on the arities and travel in the header; the salted proof is the same bytes"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=3, zero_knowledge=True)
    b, pi = fc.small_circuit(cfg, 0xB50)
    data = b.cb.build(ctx, np.random.default_rng(0xB5))
    idx, rows = b.sparse_witness()
    assert any(a > 1 for a in data.fri_arity_bits) and data.blind_rows[1] > 0
    nat = plonk.NativeCircuit(ctx, data.export_blob(idx, wide_arity=True))
    assert nat.fri_arity_bits == data.fri_arity_bits
    flat = nat.prove_rows(ctx, rows, pi, 0xB80)
    assert np.array_equal(flat, plonk.prove_sparse(ctx, data, idx, rows, pi, 0xB80, flat_only=True))
    assert ctx.lib.gl355_circuit_verify(nat.h, flat.ctypes.data, flat.size, pi.ctypes.data, pi.size) == 0


def _refused(gl, ctx, plonk, blob, code):
    with pytest.raises(gl.Gl355Error) as ei:
        plonk.NativeCircuit(ctx, blob)
    assert ei.value.code == code and "circuit_load" in str(ei.value), str(ei.value)
    # the refusal freed what it had allocated and the context goes on working
    x = np.arange(16, dtype=np.uint64).reshape(2, 8)
    got = ctx.hash_no_pad(x)
    assert all(np.array_equal(got[i], plonk.host_hash_no_pad(x[i])) for i in range(2))


def test_the_loader_refuses_a_malformed_table_by_name(gl, ctx):
    c = case(ctx, [2, 3])
    plonk, blob = c["plonk"], c["blob"]
    assert int(blob[2]) == 6 and int(blob[3]) == 3 and int(blob[92]) == 1      # degree 2^6, rate 3, cap height 1

    def with_table(*words):
        bad = blob.copy()
        bad[HDR:HDR + 2] = np.array(words, dtype=np.uint64)
        return bad
    _refused(gl, ctx, plonk, with_table(0, 3), INVALID_ARG)               # an arity word 0
    _refused(gl, ctx, plonk, with_table(2, 5), UNSUPPORTED)               # an arity word 5
    _refused(gl, ctx, plonk, with_table(1 << 32, 3), INVALID_ARG)         # an arity word 2^32 (not its low 32 bits)
    _refused(gl, ctx, plonk, with_table(4, 3), INVALID_ARG)               # 7 bits folded out of a degree-2^6 polynomial
    _refused(gl, ctx, plonk, blob[:-1], INVALID_ARG)                      # one word short
    _refused(gl, ctx, plonk, np.concatenate([blob, blob[-1:]]), INVALID_ARG)   # one word long
    bad = blob.copy()
    bad[1] = 6
    _refused(gl, ctx, plonk, bad, INVALID_ARG)                            # version 6
    # the untouched blob still loads, with a handle of its own
    assert plonk.NativeCircuit(ctx, blob).fri_arity_bits == [2, 3]


def test_the_loader_refuses_a_layer_narrower_than_the_cap(gl, ctx):
    """cap height 6 at degree 2^6, rate 3: the LDE has 2^9 points, layers [2, 2] stay within the degree and the second (2^5 leaves) is
    narrower than the 2^6 cap"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=[2, 1], zero_knowledge=False, cap_height=6)
    b, _ = fc.small_circuit(cfg, 0xB50)
    data = b.cb.build(ctx, np.random.default_rng(0xB5), min_degree_bits=6)
    assert data.degree_bits == 6 and data.fri_arity_bits == [2, 1]
    blob = data.export_blob(b.sparse_witness()[0], wide_arity=True)
    assert plonk.NativeCircuit(ctx, blob).fri_arity_bits == [2, 1]        # 2^6 leaves: exactly as wide as the cap
    bad = blob.copy()
    bad[HDR + 1] = 2
    _refused(gl, ctx, plonk, bad, INVALID_ARG)


def test_version_words_must_match_the_body(gl, ctx):
    """a version-4 word on a version-2 body, and an arity-2 circuit under versions 2 and 4"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cfg = fc.config_of(plonk, reduction_arity_bits=1, zero_knowledge=False, cap_height=1)
    b, pi = fc.small_circuit(cfg, 0xB50)
    data = b.cb.build(ctx, np.random.default_rng(0xB5), min_degree_bits=6)
    idx, rows = b.sparse_witness()
    L = len(data.fri_arity_bits)
    assert L >= 1 and all(a == 1 for a in data.fri_arity_bits)
    v2 = data.export_blob(idx)
    assert int(v2[1]) == 2
    nat2 = plonk.NativeCircuit(ctx, v2)
    assert nat2.fri_arity_bits == [1] * L                                 # no table: all ones
    bad = v2.copy()
    bad[1] = 4
    _refused(gl, ctx, plonk, bad, INVALID_ARG)
    # the same circuit with a table of ones proves the same bytes
    nat4 = plonk.NativeCircuit(ctx, data.export_blob(idx, wide_arity=True))
    assert nat4.fri_arity_bits == [1] * L and nat4.proof_words == nat2.proof_words
    assert np.array_equal(nat4.prove_rows(ctx, rows, pi, 0xB70), nat2.prove_rows(ctx, rows, pi, 0xB70))


def test_version_5_carries_the_table_and_the_cap(gl, ctx):
    c = case(ctx, [2, 3])
    plonk, data = c["plonk"], c["data"]
    ext = np.array([11, 12, 13, 14], dtype=np.uint64)
    blob = data.export_blob(c["idx"], external_digest=ext, wide_arity=True)
    assert int(blob[1]) == 5
    nat = plonk.NativeCircuit(ctx, blob)
    assert nat.fri_arity_bits == [2, 3] and nat.proof_words == c["nat"].proof_words
    pi = np.ascontiguousarray(c["pis"][0])
    flat = nat.prove_rows(ctx, c["rows"][0], pi, 0xB60)
    assert ctx.lib.gl355_circuit_verify(nat.h, flat.ctypes.data, flat.size, pi.ctypes.data, pi.size) == 0
    assert ctx.lib.gl355_circuit_verify(c["nat"].h, flat.ctypes.data, flat.size, pi.ctypes.data, pi.size) == VERIFY     # another digest, another transcript
    bad = blob.copy()
    bad[-1] ^= np.uint64(1)                                               # the carried cap
    _refused(gl, ctx, plonk, bad, INVALID_ARG)
