"""GPU: the native flow (artifacts with an arity table -> gl355_circuit_prove_tape(_units), gl355_semaphore_units, gl355_aggregate_units)
at FRI arities above 2.  Shapes as in the other arity tests: the small gate-zoo circuit at degree 2^6, a depth-2 access set, 3 queries,
cap height 1, no blinding rows; every outer circuit is built with CircuitConfig.use_interpolation_gate and a Fixed reduction list, so
that each circuit of a flow -- the Semaphore circuit ([3] at degree 2^4), the recursive circuit and both aggregation levels ([3, 2]) --
has a layer wider than 2.  Everything native is held byte for byte against the host-orchestrated path of the same data and seed."""
import ctypes as C
import importlib
import os
import tempfile

import numpy as np
import pytest

import coset_interpolation_model as cim
import fri_arity_cases as fc
from oracle_lib import rand_field
from test_gpu_prover import make_access_set

pytestmark = pytest.mark.gpu

OUTER_ARITIES = [3, 2]
WITNESS = -6
_rec, _sem = {}, {}


def _mod(name):
    return importlib.import_module("stark-verifier_amd." + name)


def wide_config(plonk, **kw):
    kw.setdefault("reduction_arity_bits", OUTER_ARITIES)
    return plonk.CircuitConfig(use_interpolation_gate=True, zero_knowledge=False, cap_height=1, num_query_rounds=3, **kw)


def is_wide(arities):
    return any(a > 1 for a in arities)


def recursion_case(ctx):
    """two [2, 3] inner proofs of the small circuit, the outer circuit at [3, 2] built from the first, its artifact"""
    if not _rec:
        plonk, rec = _mod("plonk"), _mod("recursion")
        cfg = fc.config_of(plonk, reduction_arity_bits=[2, 3], zero_knowledge=False, cap_height=1)
        inner = []
        for u in range(2):
            b, pi = fc.small_circuit(cfg, 0xC50 + u)
            if u == 0:
                data = b.cb.build(ctx, np.random.default_rng(0xC5), min_degree_bits=6)
            idx, rows = b.sparse_witness()
            inner.append((plonk.prove_sparse(ctx, data, idx, rows, pi, 0xC60 + u, flat_only=True), pi))
        rc = rec.RecursiveCircuit(ctx, data.common(), k=1, config=wide_config(plonk)).build([inner[0]], np.random.default_rng(0xC6))
        _rec.update(plonk=plonk, rec=rec, data=data, inner=inner, rc=rc, nat=rc.native())
    return _rec


def native_verify(ctx, nat, flat, pis):
    flat, pis = np.ascontiguousarray(flat, dtype=np.uint64), np.ascontiguousarray(pis, dtype=np.uint64)
    return ctx.lib.gl355_circuit_verify(nat.h, flat.ctypes.data, flat.size, pis.ctypes.data, pis.size)


def test_a_wide_outer_circuit_goes_native_without_a_keyword(gl, ctx):
    c = recursion_case(ctx)
    plonk, rc, nat, inner = c["plonk"], c["rc"], c["nat"], c["inner"]
    outer = rc.data
    assert outer.fri_arity_bits == OUTER_ARITIES and outer.degree_bits <= 11
    assert int(nat.blob[1]) == 4 and nat.fri_arity_bits == OUTER_ARITIES
    assert nat.proof_words == ctx.lib.gl355_proof_words(C.byref(outer.prover_data(ctx)))
    # one proof: the tape inside gl355_circuit_prove_tape against the Python-side replay + gl355_prove_sparse
    flat_py, pis_py = rc.prove_flat([inner[0]], seed=0xC70)
    assert flat_py.size == nat.proof_words
    flat_nat, pis_nat = nat.prove_tape(ctx, np.concatenate(inner[0]), 0xC70)
    assert np.array_equal(flat_nat, flat_py) and np.array_equal(pis_nat, pis_py)
    outer.verify(flat_nat, pis_nat)
    assert native_verify(ctx, nat, flat_nat, pis_nat) == 0
    # host and device witness generation agree, two units in lock-step equal two single proofs
    inputs = np.stack([np.concatenate([f, p]) for f, p in inner])
    d_rows, d_pis = nat.witness_rows(ctx, inputs, on_device=True)
    h_rows, h_pis = nat.witness_rows(ctx, inputs, on_device=False)
    assert np.array_equal(d_rows, h_rows) and np.array_equal(d_pis, h_pis)
    flats, pis = nat.prove_tape_units(ctx, inputs, [0xC70, 0xC71])
    assert np.array_equal(flats[0], flat_py) and np.array_equal(pis, d_pis)
    single, _ = nat.prove_tape(ctx, inputs[1], 0xC71)
    assert np.array_equal(flats[1], single)
    assert native_verify(ctx, nat, flats[1], pis[1]) == 0


def test_a_second_level_verifies_the_wide_outer_proof_natively(gl, ctx):
    c = recursion_case(ctx)
    plonk, rec, rc, nat = c["plonk"], c["rec"], c["rc"], c["nat"]
    flat1, pis1 = nat.prove_tape(ctx, np.concatenate(c["inner"][0]), 0xC80)
    rc2 = rec.RecursiveCircuit(ctx, rc.data.common(), k=1, config=wide_config(plonk)).build([(flat1, pis1)], np.random.default_rng(0xC8))
    # level 1 folds by 8 and 4: level 2 has interpolation rows for both sizes
    want = {(12, plonk.coset_interpolation_param(a, 8)) for a in OUTER_ARITIES}
    assert {g for g in rc2.data.gates if g[0] == cim.COSET_INTERPOLATION} == want
    nat2 = rc2.native()
    assert int(nat2.blob[1]) == 4 and nat2.fri_arity_bits == rc2.data.fri_arity_bits and is_wide(nat2.fri_arity_bits)
    flat2, pis2 = nat2.prove_tape(ctx, np.concatenate([flat1, pis1]), 0xC81)
    assert np.array_equal(flat2, rc2.prove_flat([(flat1, pis1)], seed=0xC81)[0])
    rc2.data.verify(flat2, pis2)
    assert native_verify(ctx, nat2, flat2, pis2) == 0
    assert np.array_equal(pis2, c["inner"][0][1])
    print("recursion at wide arities: level 1 degree 2^%d %r, level 2 degree 2^%d %r" % (
        rc.data.degree_bits, rc.data.fri_arity_bits, rc2.data.degree_bits, rc2.data.fri_arity_bits))


def test_a_mutated_inner_fri_layer_fails_at_the_entry_the_host_replay_names(gl, ctx):
    c = recursion_case(ctx)
    gad, nat, rc = _mod("gadgets"), c["nat"], c["rc"]
    flat, pi = c["inner"][0]
    for name, bad, _ in fc.mutations(c["data"].common(), flat):
        inputs = np.concatenate([bad, pi])
        rows = np.empty((rc.row_idx.size, 135), dtype=np.uint64)
        failed = C.c_uint64(0)
        rcode = ctx.lib.gl355_witness_replay(rc.tape.ctypes.data, rc.tape.shape[0], inputs.ctypes.data, inputs.size, rows.ctypes.data,
                                             rows.size, 135, C.byref(failed))
        assert rcode == WITNESS and rc.tape[failed.value][0] == gad.TAPE_ASSERT_EQ, name
        with pytest.raises(gl.Gl355Error) as ei:
            nat.witness_rows(ctx, inputs[None, :], on_device=True)
        assert ei.value.code == WITNESS and ei.value.failed_entry == failed.value, name
        with pytest.raises(gl.Gl355Error) as ei:
            nat.prove_tape(ctx, inputs, 0xC90)
        assert ei.value.code == WITNESS and ("tape entry %d" % failed.value) in str(ei.value), name


# ---- Semaphore: four signals of a depth-2 access set at [3], aggregated and proven in batches ----------------------------------------------

def semaphore_case(gl, ctx):
    if not _sem:
        plonk = _mod("plonk")
        aset, sks, rng = make_access_set(gl, ctx, 2, 0xCA0)
        cfg = plonk.CircuitConfig(zero_knowledge=False, cap_height=1, num_query_rounds=3, reduction_arity_bits=[3])
        data, rows = aset.build(rng, config=cfg)
        assert data.fri_arity_bits == [3]
        members = [2, 3, 0, 1]
        topics = [rand_field(rng, 4) for _ in members]
        sigs = []
        for k, (m, t) in enumerate(zip(members, topics)):
            sig, _ = aset.make_signal_fast(sks[m], t, m, 0xCB0 + k, flat_only=True)
            sigs.append((sig.proof, np.concatenate([aset.tree.cap[0], sig.nullifier[0], sig.topics[0]])))
            data.verify(*sigs[-1])
        _sem.update(plonk=plonk, aset=aset, sks=sks, rng=rng, data=data, rows=rows, members=members, topics=topics, sigs=sigs)
    return _sem


def test_aggregate_four_wide_signals_through_every_path(gl, ctx):
    s = semaphore_case(gl, ctx)
    plonk, rec, sigs = s["plonk"], _mod("recursion"), s["sigs"]
    # without the flag the in-circuit verifier refuses by its own name, at the first level
    plain = plonk.CircuitConfig(zero_knowledge=False, cap_height=1, num_query_rounds=3, reduction_arity_bits=OUTER_ARITIES)
    with pytest.raises(ValueError, match="the in-circuit verifier supports arity-2 FRI only"):
        rec.Aggregator(ctx, s["data"].common(), config=plain).aggregate(sigs, seed=100, rng=np.random.default_rng(0xCC))
    agg = rec.Aggregator(ctx, s["data"].common(), config=wide_config(plonk))
    proof, pis, cd = agg.aggregate(sigs, seed=100, rng=np.random.default_rng(0xCC))
    assert len(agg.levels) == 2
    for lvl in agg.levels:
        assert lvl.data.fri_arity_bits == OUTER_ARITIES and int(lvl.native().blob[1]) == 4 and lvl.native().fri_arity_bits == OUTER_ARITIES
    agg.levels[1].data.verify(proof, pis)
    assert pis.size == 4 + 16 + 16
    assert np.array_equal(pis[:4], s["aset"].tree.cap[0])
    assert np.array_equal(pis[4:20], np.concatenate([sg[1][4:8] for sg in sigs]))
    assert np.array_equal(pis[20:36], np.concatenate(s["topics"]))
    ctx2 = gl.Context(0)
    try:
        for cs in ([ctx], [ctx, ctx2]):
            n_proof, n_pis, _ = agg.aggregate_native(sigs, seed=100, ctxs=cs)
            assert np.array_equal(n_proof, proof) and np.array_equal(n_pis, pis), len(cs)
        p_proof, p_pis, _ = agg.aggregate(sigs, seed=100, ctxs=[ctx, ctx2])
        assert np.array_equal(p_proof, proof) and np.array_equal(p_pis, pis)
        with tempfile.TemporaryDirectory() as d:
            agg.save(d)
            for l in range(2):
                assert int(np.load(os.path.join(d, "level%d.npy" % l))[1]) == 4
            agg2 = rec.Aggregator.load(ctx, d)
            l_proof, l_pis, _ = agg2.aggregate_native(sigs, seed=100, ctxs=[ctx, ctx2])
            assert np.array_equal(l_proof, proof) and np.array_equal(l_pis, pis)
    finally:
        ctx2.close()
    bad = (sigs[1][0].copy(), sigs[1][1])
    bad[0][40] ^= np.uint64(1)
    with pytest.raises(gl.Gl355Error) as ei:
        agg.aggregate_native([sigs[0], bad, sigs[2], sigs[3]], seed=1)
    assert ei.value.code == WITNESS
    print("aggregation at wide arities: level degrees 2^%d, 2^%d" % (agg.levels[0].data.degree_bits, agg.levels[1].data.degree_bits))


@pytest.mark.parametrize("device_replay", [0, 1])
def test_the_batch_runtime_equals_the_calls_one_by_one(gl, ctx, device_replay):
    """gl355_semaphore_units over five members with both artifacts wide, on three contexts, as test_gpu_native.py::test_native_batch_runtime
    does at arity 2"""
    s = semaphore_case(gl, ctx)
    plonk, rec, aset, sks = s["plonk"], _mod("recursion"), s["aset"], s["sks"]
    topic = s["topics"][0]
    if "sem_nat" not in s:
        idx, vals, pi = aset.witness_rows(s["rows"], sks[0], topic, 0)
        s["sem_nat"] = plonk.NativeCircuit(ctx, s["data"].export_blob(idx, wide_arity=True))
        flat0, pis0 = s["sem_nat"].semaphore_prove(ctx, sks[0], topic, 0, aset.tree.prove_host(0), 1)
        assert np.array_equal(flat0, plonk.prove_sparse(ctx, s["data"], idx, vals, pi, 1, flat_only=True)) and np.array_equal(pis0, pi)
        s["rec_rc"] = rec.RecursiveCircuit(ctx, s["data"].common(), k=1, config=wide_config(plonk)).build([(flat0, pis0)], np.random.default_rng(0xCD))
    sem, nat = s["sem_nat"], s["rec_rc"].native()
    assert sem.fri_arity_bits == [3] and nat.fri_arity_bits == OUTER_ARITIES and int(sem.blob[1]) == 4 and int(nat.blob[1]) == 4
    ctxs = [gl.Context(0) for _ in range(3)]
    try:
        for cx in ctxs:
            cx.set_option(6, device_replay)          # GL355_OPT_DEVICE_REPLAY
        members = np.array([3, 1, 0, 2, 1], dtype=np.uint64)
        leaves, proofs, per = plonk.semaphore_units(ctxs, sem, nat, sks, topic, aset.tree.digests, members, 1000, want_proofs=True)
        assert sum(per) == members.size and proofs.shape[1] == nat.proof_words
        for j, m in enumerate(members):
            f, p = sem.semaphore_prove(ctx, sks[m], topic, int(m), aset.tree.prove_host(int(m)), plonk.derive_key(1000, 2 * j))
            o, op = nat.prove_tape(ctx, np.concatenate([f, p]), plonk.derive_key(1000, 2 * j + 1))
            assert np.array_equal(proofs[j], o) and np.array_equal(leaves[j], op[4:12]), j
            assert native_verify(ctx, nat, proofs[j], op) == 0
        leaves2, proofs2, _ = plonk.semaphore_units(ctxs, sem, None, sks, topic, aset.tree.digests, members[:2], 1000, want_proofs=True)
        assert np.array_equal(leaves2, leaves[:2]) and proofs2.shape[1] == sem.proof_words
    finally:
        for cx in ctxs:
            cx.close()
