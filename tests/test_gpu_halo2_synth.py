"""GPU: gl355_halo2_synthesize (csrc/halo2_synth.hip) against the host replay and the recorder's eager values, word for word, on the shared
cases (halo2_synth_cases.py) -- the failing ones included: same status, and the witness still written -- plus a level 4 096 + 37 entries wide
(the lane-per-entry path with a partial last wave), 40 chained permutations (121 levels: one launch each), Merkle proofs, determinism, and
the columns left resident for gl355_plonk_check_witness; then the real circuit: FriOpeningsCircuit over a wrap proof, synthesised on the device,
checked, proven, and verified natively and by the restated Python verifier."""
import importlib

import numpy as np
import pytest

import halo2_synth_cases as cs

pytestmark = pytest.mark.gpu
hg, h2, K = cs.hg, cs.h2, cs.K


def device_replay(ctx, rec):
    tape = hg.DeviceTape(ctx, rec.tape(), K, len(rec.inputs))
    try:
        return tape.synthesize(np.array(rec.inputs, dtype=np.uint64))
    finally:
        tape.close()


def check(ctx, rec):
    advice, status = device_replay(ctx, rec)
    host, host_status = hg.synthesize_host(rec.tape(), K, rec.inputs)
    assert status == host_status == rec.status()
    for name, want in (("the host replay", host), ("the recorder", rec.advice())):
        if not np.array_equal(advice, want):
            col, row = np.argwhere((advice != want).any(axis=2))[0]
            raise AssertionError("device synthesis differs from %s at advice column %d row %d" % (name, col, row))
    return status


@pytest.mark.parametrize("case", ["arithmetic_case", "permute_case", "wide_case", "deep_case"])
def test_device_equals_host_equals_recorder(ctx, case):
    rec = getattr(cs, case)()[0]
    if case == "wide_case":
        assert rec.level_widths() == [4096 + 37]
    if case == "deep_case":
        assert len(rec.level_widths()) == 1 + 3 * 40
    assert check(ctx, rec) == (hg.NO_FAILURE, 0)


def test_failing_cases_same_status_and_witness_written(ctx):
    assert check(ctx, cs.failing_value_case()) == (1, 2)
    first, count = check(ctx, cs.failing_assert_case())
    assert count == 2 and int(cs.failing_assert_case().tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


@pytest.mark.parametrize("depth,leaf_len,index,mutate", [(3, 9, 5, None), (3, 9, 5, "sibling"), (3, 9, 5, "cap_index"), (0, 4, 1, None), (0, 4, 1, "cap_index")])
def test_merkle_proofs(ctx, orc, depth, leaf_len, index, mutate):
    from oracle_lib import Bn254Oracle
    rec = cs.merkle_case(Bn254Oracle(orc), depth, leaf_len, index, mutate)
    first, count = check(ctx, rec)
    if mutate is None:
        assert count == 0
    else:
        assert count >= 1 and int(rec.tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


def test_deterministic_and_resident_columns(ctx):
    """two syntheses are byte-equal; synthesis into device memory equals synthesis into host memory; the resident columns are what
    gl355_plonk_check_witness takes: zero failures for the satisfied case, the failing VALUE's row for the other"""
    import torch
    rec, _ = cs.arithmetic_case()
    tape = hg.DeviceTape(ctx, rec.tape(), K, len(rec.inputs))
    inputs = np.array(rec.inputs, dtype=np.uint64)
    a1, s1 = tape.synthesize(inputs)
    a2, s2 = tape.synthesize(inputs)
    assert s1 == s2 and np.array_equal(a1, a2)
    dev = torch.full((hg.N_ADVICE, 1 << K, 4), -1, dtype=torch.int64, device="cuda")      # stale contents: the call must zero what it does not write
    d_in = torch.from_numpy(inputs.view(np.int64)).cuda()
    _, s3 = tape.synthesize(d_in.data_ptr(), out=dev.data_ptr())
    torch.cuda.synchronize()
    assert s3 == s1 and np.array_equal(dev.cpu().numpy().view(np.uint64), a1)
    lay = rec.layout()
    mock = h2.MockProver(ctx, lay.cs, K, lay.fixed_array(), lay.mapping_array())
    recs, total = mock.check(dev.data_ptr(), [rec.instance])
    assert total == 0, [mock._resolve(r) for r in recs[:4]]
    tape.close()
    bad = cs.failing_value_case()
    tape = hg.DeviceTape(ctx, bad.tape(), K, len(bad.inputs))
    _, status = tape.synthesize(np.array(bad.inputs, dtype=np.uint64), out=dev.data_ptr())
    tape.close()
    assert status == (1, 2)
    lay = bad.layout()
    mock = h2.MockProver(ctx, lay.cs, K, lay.fixed_array(), lay.mapping_array())
    fails = mock.verify(dev.data_ptr(), [bad.instance])
    assert fails and {f.row for f in fails if f.kind == h2.FAIL_GATE} == {bad.entry_rows(status[0])[0]}


def test_tape_load_rejects_an_invalid_tape(ctx, gl):
    rec = cs.failing_assert_case()
    t = rec.tape().reshape(-1, 8).copy()
    t[0, 1] = 1 << K
    with pytest.raises(gl.Gl355Error):
        hg.DeviceTape(ctx, t.reshape(-1), K, len(rec.inputs))


def test_prove_from_inputs_and_native_verify(ctx):
    """a recorded circuit end to end: artifact -> keygen -> gl355_halo2_synthesize into device memory -> gl355_plonk_prove on the resident
    columns -> gl355_plonk_verify accepts with the exposed values as instances and rejects a changed instance"""
    tau = 0x1F2E3D4C5B6A79880123456789ABCDEF
    rec, _ = cs.arithmetic_case()
    art = rec.artifact()
    g, g_lagrange = h2.kzg_setup(ctx, K, tau)
    prover = h2.PlonkProver.from_artifact(ctx, art, g, g_lagrange)
    proof, status = prover.prove_from_inputs(np.array(rec.inputs, dtype=np.uint64), [rec.instance], bytes(range(32)))
    assert status == (hg.NO_FAILURE, 0)
    vk = prover.verifying_key(h2.kzg_setup_g2(tau))
    assert vk.verify([rec.instance], proof), vk.last_error
    assert vk.verify([[rec.instance[0], rec.instance[1] ^ 1]], proof) is False
    prover.close()


TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF


@pytest.fixture(scope="module")
def wrap(gl, ctx):
    """a wrap proof made as test_gpu_bn254.py::test_wrap_proof_with_bn254_hasher makes one (a Semaphore proof wrapped under the BN254-Poseidon
    config), FriOpeningsCircuit recorded from it, and its prover: shared by the tests below, none of which changes it"""
    from oracle_lib import rand_field
    from test_gpu_prover import make_access_set
    rcn = importlib.import_module("stark-verifier_amd.recursion")
    vc = importlib.import_module("stark-verifier_amd.halo2_verifier_circuit")
    aset, sks, rng = make_access_set(gl, ctx, 3, 0x2542)
    topic = rand_field(rng, 4)
    sig, data = aset.make_signal_fast(sks[4], topic, 4, 3, flat_only=True)
    inner = (sig.proof, np.concatenate([aset.tree.cap[0], sig.nullifier[0], sig.topics[0]]))
    wc = rcn.WrapperCircuit(ctx, data.common()).build([inner], rng)
    flat, _ = wc.prove_flat([inner], seed=17)
    circuit = vc.FriOpeningsCircuit(wc.data.common())
    inputs = circuit.inputs(flat)
    rec = circuit.record(inputs)
    print("FriOpeningsCircuit of the wrap proof: %d rows, k = %d, %d tape entries on %d levels, %d inputs, %d instances"
          % (rec.rows_used, rec.k, len(rec.entries), len(rec.level_widths()), inputs.size, len(rec.instance)))
    g, g_lagrange = h2.kzg_setup(ctx, rec.k, TAU)
    prover = h2.PlonkProver.from_artifact(ctx, rec.artifact(), g, g_lagrange, checkable=True)
    yield circuit, inputs, rec, prover
    prover.close()


def test_wrap_proof_openings_synthesised_proven_and_verified(ctx, wrap):
    """the real circuit: every Merkle opening of a wrap proof's FRI query rounds.  The device synthesis reports no failing entry and equals
    the recorder's values; gl355_plonk_check_witness finds nothing; the proof of prove_from_inputs is accepted by gl355_plonk_verify and by
    the restated verifier (halo2_verifier.py) with the caps and the indices as instances, and refused with one instance changed"""
    import torch
    import halo2_verifier as hv
    circuit, inputs, rec, prover = wrap
    assert 18 <= rec.k <= 19
    assert rec.status() == (hg.NO_FAILURE, 0)
    dev = torch.empty((hg.N_ADVICE, 1 << rec.k, 4), dtype=torch.int64, device="cuda")
    _, status = prover.tape.synthesize(inputs, out=dev.data_ptr())
    torch.cuda.synchronize()
    assert status == (hg.NO_FAILURE, 0)
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), rec.advice())
    del dev
    proof, status = prover.prove_from_inputs(inputs, [rec.instance], bytes(range(32)), check=True)      # check: MockProver.assert_satisfied on the resident columns
    assert status == (hg.NO_FAILURE, 0)
    vk = prover.verifying_key(h2.kzg_setup_g2(TAU))
    assert vk.verify([rec.instance], proof), vk.last_error
    changed = list(rec.instance)
    changed[-1] ^= 1                                               # the last query round's index
    assert vk.verify([changed], proof) is False
    changed = list(rec.instance)
    changed[5] ^= 1                                                # a word of the wires cap
    assert vk.verify([changed], proof) is False
    pt = lambda a: (lambda x, y: None if (x, y) == (0, 0) else (x, y))(h2.from_limbs(a[:4])[0], h2.from_limbs(a[4:])[0])      # noqa: E731
    pvk = dict(digest=prover.digest, fixed_commitments=[pt(c) for c in prover.fixed_commitments], sigma_commitments=[pt(c) for c in prover.sigma_commitments])
    assert hv.verify(rec.k, rec.cs, pvk, [rec.instance], proof, TAU)


def test_wrap_proof_flipped_sibling_names_its_round(ctx, wrap):
    """one sibling word of one query round flipped in the input vector: status names an ASSERT_EQ entry, the witness is still written, and
    gl355_plonk_check_witness names rows inside that round's rows only"""
    import torch
    circuit, inputs, rec, prover = wrap
    query = len(circuit.queries) // 2
    _, initial, _ = circuit.queries[query]
    bad = inputs.copy()
    bad[initial[1][1][3][2]] ^= 1                                  # the wires tree's fourth sibling, its third word
    dev = torch.empty((hg.N_ADVICE, 1 << rec.k, 4), dtype=torch.int64, device="cuda")
    _, (first, count) = prover.tape.synthesize(bad, out=dev.data_ptr())
    assert count >= 1 and int(rec.tape().reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ
    fails = prover.mock_prover().verify(dev.data_ptr(), [rec.instance])
    lo, hi = circuit.round_rows[query]
    assert fails and all(lo <= f.row < hi for f in fails), [h2.describe_failure(f) for f in fails[:4]]
