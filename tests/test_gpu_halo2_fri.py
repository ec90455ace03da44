"""GPU: part 2 of the Halo2 verifier circuit on the device.  gl355_halo2_synthesize against the host replay, word for word and with the same
status, on the GoldilocksExtensionChip cases (the INV_EXT operand, the (0, 0) divisor included), on FriVerifierCircuit over two real proofs of
the CPU prover and on their four mutations; one circuit end to end at k = 17 (keygen, synthesis, gl355_plonk_check_witness, create_proof, the
native verifier with the public-inputs hash as instances); and part-1 tapes, whose columns must not change: these small circuits consist of
narrow levels with PERMUTE entries, which is where the kernel spreads a permutation over the lanes of a group."""
import numpy as np
import pytest

import halo2_fri_cases as fc
import halo2_synth_cases as cs

pytestmark = pytest.mark.gpu
hg, h2, K = cs.hg, cs.h2, cs.K
TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF


@pytest.fixture(scope="module")
def cases():
    return fc.synth_cases()


def device_equals_host(ctx, tape, k, inputs):
    dt = hg.DeviceTape(ctx, tape, k, len(inputs))
    try:
        advice, status = dt.synthesize(np.asarray(inputs, dtype=np.uint64))
    finally:
        dt.close()
    host, host_status = hg.synthesize_host(tape, k, inputs)
    assert status == host_status
    if not np.array_equal(advice, host):
        col, row = np.argwhere((advice != host).any(axis=2))[0]
        raise AssertionError("device synthesis differs from the host replay at advice column %d row %d" % (col, row))
    return status


@pytest.mark.parametrize("name", ["extension", "fri_zk", "fri_plain"])
def test_device_equals_host_and_recorder(ctx, cases, name):
    tape, k, inputs, rec = cases[name]
    assert device_equals_host(ctx, tape, k, inputs) == rec.status() == (hg.NO_FAILURE, 0)


def test_zero_divisor_fails_the_same_assert(ctx, cases):
    tape, k, inputs, rec = cases["zero_divisor"]
    first, count = device_equals_host(ctx, tape, k, inputs)
    assert (first, count) == rec.status() and count >= 1 and int(tape.reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


@pytest.mark.parametrize("tag", ["zk", "plain"])
@pytest.mark.parametrize("name", ["quotient_opening", "final_poly", "pow_witness", "pi_hash"])
def test_mutations_fail_as_on_the_host(ctx, cases, tag, name):
    tape, k, inputs, _ = cases["fri_%s_%s" % (tag, name)]
    first, count = device_equals_host(ctx, tape, k, inputs)
    assert count >= 1 and int(tape.reshape(-1, 8)[first, 0]) & 0xFF == hg.OP_ASSERT_EQ


def test_part_one_tapes_give_the_same_columns(ctx, orc):
    """the guard of the kernel's spread form: tapes recorded before it existed"""
    from oracle_lib import Bn254Oracle
    for permutes, rec in ((False, cs.arithmetic_case()[0]), (True, cs.merkle_case(Bn254Oracle(orc), 3, 9, 5)), (True, cs.permute_case()[0])):
        assert min(rec.level_widths()) < 64 and any(e[2] == hg.OP_PERMUTE for e in rec.entries) == permutes
        assert device_equals_host(ctx, rec.tape(), K, rec.inputs) == rec.status() == (hg.NO_FAILURE, 0)
        tape = hg.DeviceTape(ctx, rec.tape(), K, len(rec.inputs))
        advice, _ = tape.synthesize(np.array(rec.inputs, dtype=np.uint64))
        tape.close()
        assert np.array_equal(advice, rec.advice())


def test_end_to_end_at_k17(ctx):
    """from_artifact -> prove_from_inputs(check=True) -> gl355_plonk_verify with the four hash words as instances; refused with one changed"""
    c = fc.case(False)
    rec = c.rec
    g, g_lagrange = h2.kzg_setup(ctx, rec.k, TAU)
    prover = h2.PlonkProver.from_artifact(ctx, rec.artifact(), g, g_lagrange, checkable=True)
    try:
        proof, status = prover.prove_from_inputs(c.inputs, [rec.instance], bytes(range(32)), check=True)
        assert status == (hg.NO_FAILURE, 0)
        vk = prover.verifying_key(h2.kzg_setup_g2(TAU))
        assert rec.instance == [int(v) for v in c.pi_hash]
        assert vk.verify([rec.instance], proof), vk.last_error
        changed = list(rec.instance)
        changed[2] ^= 1
        assert vk.verify([changed], proof) is False
    finally:
        prover.close()
