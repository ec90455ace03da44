"""GPU: changing a Semaphore group.  A resident AccessSet (semaphore.AccessSet(ctx, keys, resident=True): its tree is an api.DeviceMerkleTree) replaces a
member through update_members at the cost of that member's path; signals made afterwards carry the new root, the batch runtime reads every unit's path
from the resident tree (gl355_semaphore_units_tree) and proves the same bytes as from the downloaded digests."""
import importlib

import numpy as np
import pytest

import plonk_verifier as pv
from test_gpu_prover import make_access_set, rand_field

pytestmark = pytest.mark.gpu
E_INVALID_ARG = -1


@pytest.fixture(scope="module")
def group(gl, ctx, orc):
    """16 members (height 4): a resident access set and a host one over the same keys, member 9 replaced in both"""
    sem = importlib.import_module("stark-verifier_amd.semaphore")
    host, sks, rng = make_access_set(gl, ctx, 4, 0x903)
    keys = host.tree.leaves.copy()
    resident = sem.AccessSet(ctx, keys, resident=True)
    assert resident.resident and not host.resident and resident.tree_height() == host.tree_height() == 4
    assert np.array_equal(resident.tree.cap, host.tree.cap) and np.array_equal(resident.tree.digests, host.tree.digests)
    circuit = resident.build(None)
    new_sk = rand_field(rng, 4)
    new_key = ctx.hash_no_pad(np.concatenate([new_sk, np.zeros(4, np.uint64)]))
    old_cap = resident.tree.cap
    for aset in (resident, host):
        aset.update_members([9], [new_key])
    assert resident.build(None) is circuit          # the circuit depends on the height alone and is kept
    keys[9] = new_key
    dig, cap = orc.merkle_build(keys, 0)
    return dict(resident=resident, host=host, sks=sks, new_sk=new_sk, keys=keys, dig=dig, cap=cap, old_cap=old_cap, rng=rng)


def test_replaced_member_changes_the_root_in_both_modes(group, orc):
    g = group
    assert not np.array_equal(g["cap"], g["old_cap"])
    for aset in (g["resident"], g["host"]):       # non-resident mode rebuilds: the same bytes
        assert np.array_equal(aset.tree.cap[0], g["cap"][0])
        assert np.array_equal(aset.tree.digests, g["dig"])
        assert np.array_equal(aset.tree.leaves, g["keys"])
        assert np.array_equal(aset.tree.prove(9), orc.merkle_prove(g["dig"], 16, 0, 9))
    with pytest.raises(Exception):
        g["host"].update_members([16], [g["keys"][0]])
    with pytest.raises(Exception):
        g["resident"].update_members([16], [g["keys"][0]])
    assert np.array_equal(g["resident"].tree.digests, g["dig"])


def test_signal_of_the_new_member_verifies_and_the_old_key_proves_another_root(group, orc):
    g = group
    aset, topic = g["resident"], rand_field(g["rng"], 4)
    signal, data = aset.make_signal_fast(g["new_sk"], topic, 9, 0x9A1)
    pv.verify(orc, data.common(), signal.proof)
    assert np.array_equal(signal.proof["public_inputs"][:4], g["cap"][0])
    assert np.array_equal(signal.nullifier[0], orc.hash_no_pad(np.concatenate([g["new_sk"], topic])))
    # the dense-witness path (fill_semaphore_targets) reads the resident tree too; make_signal itself asserts root == cap
    signal2, _ = aset.make_signal(g["new_sk"], topic, 9, np.random.default_rng(0x9A2), check=True)
    pv.verify(orc, data.common(), signal2.proof)
    # the replaced key is no member any more: its proof is still a valid proof (as test_native_batch_runtime notes), of a root that is not the set's
    old, _ = aset.make_signal_fast(g["sks"][9], topic, 9, 0x9A3)
    pv.verify(orc, data.common(), old.proof)
    assert not np.array_equal(old.proof["public_inputs"][:4], g["cap"][0])
    # another member's path runs through the changed digests
    other, _ = aset.make_signal_fast(g["sks"][8], topic, 8, 0x9A4)
    assert np.array_equal(other.proof["public_inputs"][:4], g["cap"][0])


def test_batch_runtime_on_the_resident_tree_proves_the_same_bytes(gl, ctx, group, orc):
    g = group
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    aset = g["resident"]
    sks = g["sks"].copy()
    sks[9] = g["new_sk"]
    topic = rand_field(np.random.default_rng(0x9B0), 4)
    data, rows = aset.build(None)
    idx, _, _ = aset.witness_rows(rows, sks[0], topic, 0)
    sem = plonk.NativeCircuit(ctx, data.export_blob(idx))
    members = np.array([3, 9, 0, 15, 7], dtype=np.uint64)
    ctxs = [gl.Context(0) for _ in range(3)]
    try:
        digests = aset.tree.digests
        leaves_h, proofs_h, per_h = plonk.semaphore_units(ctxs, sem, None, sks, topic, digests, members, 1000, want_proofs=True)
        leaves_d, proofs_d, per_d = plonk.semaphore_units(ctxs, sem, None, sks, topic, aset.tree, members, 1000, want_proofs=True)
        assert sum(per_d) == members.size
        assert np.array_equal(leaves_d, leaves_h) and np.array_equal(proofs_d, proofs_h)
        for j, m in enumerate(members):
            assert np.array_equal(leaves_d[j, :4], orc.hash_no_pad(np.concatenate([sks[m], topic]))), m
            f, p = sem.semaphore_prove(ctx, sks[m], topic, int(m), orc.merkle_prove(g["dig"], 16, 0, int(m)), plonk.derive_key(1000, 2 * j))
            assert np.array_equal(proofs_d[j], f) and np.array_equal(p[:4], g["cap"][0]), m
        with pytest.raises(gl.Gl355Error) as e:
            plonk.semaphore_units(ctxs, sem, None, sks, topic, aset.tree, np.array([16], dtype=np.uint64), 1)
        assert e.value.code == E_INVALID_ARG
        # the entry takes the access set's kind of tree only: cap height 0, 4-word leaves, Poseidon
        for kwargs, keys in ((dict(cap_height=1), g["keys"]), (dict(cap_height=0, hasher=gl.HASH_BN254_POSEIDON), g["keys"]),
                             (dict(cap_height=0), np.concatenate([g["keys"], g["keys"][:, :1]], axis=1))):
            t = gl.DeviceMerkleTree(ctx, keys, **kwargs)
            with pytest.raises(gl.Gl355Error) as e:
                plonk.semaphore_units(ctxs, sem, None, sks, topic, t, members, 1000)
            assert e.value.code == E_INVALID_ARG, kwargs
            t.close()
    finally:
        for c in ctxs:
            c.close()
        sem.close()
