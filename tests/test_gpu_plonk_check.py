"""GPU: gl355_plonk_check_witness (halo2's MockProver::run(..).assert_satisfied(), verifier_api.rs:34-52, :72-73) against the plain-Python model
of tests/halo2_mock_model.py, which evaluates the Expression TREES: on every circuit of tests/halo2_mock_cases.py (the reference's chip shape
at k = 7 .. 10, the tuple-lookup circuit at k = 7 and 9, twelve random circuits) the clean witness gives zero failures, and for every mutation
class that applies the device's COMPLETE failure list equals the model's record for record; a capacity below the total returns the exact
prefix and the exact total; a second run and a run with device-resident inputs return the same words.

Ground truth beyond the model, at k <= 9: every clean and mutated witness is also proved (PlonkProver.prove under a gl355_kzg_setup key) and
verified (PlonkVerifier.verify): zero failures exactly when the proof is accepted, a non-empty list exactly when prove errors or verify
rejects.  The exception, on purpose: cases whose every record is poison (a gate or lookup input that reads a blinding row).  There the
constraint is evaluated on the prover's blinding values and a proof may verify by luck, so the test asserts only that the check flags them."""
import ctypes as C
import importlib

import numpy as np
import pytest

import halo2_mock_cases as mc

pytestmark = pytest.mark.gpu
h2 = importlib.import_module("stark-verifier_amd.halo2")
TAU = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF % h2.R
_params = {}


def params(ctx, k):
    if k not in _params:
        _params[k] = h2.kzg_setup(ctx, k, TAU) + (h2.kzg_setup_g2(TAU),)
    return _params[k]


def proof_accepted(gl, ctx, case, fixed, advice, instances):
    """prove-then-verify, the only way to tell a bad witness without the check: False if prove errors or the verifier rejects"""
    g, gl_, s_g2 = params(ctx, case.k)
    prover = h2.PlonkProver(ctx, case.cs, case.k, g, gl_, fixed, case.mapping)
    try:
        try:
            proof = prover.prove(advice, instances, bytes((11 * i + case.k) & 0xFF for i in range(32)))
        except gl.Gl355Error:
            return False
        vk = prover.verifying_key(s_g2)
        try:
            return vk.verify(instances, proof)
        finally:
            vk.close()
    finally:
        prover.close()


def records(recs):
    return [tuple(int(v) for v in r) for r in recs]


@pytest.mark.parametrize("name", [c[0] for c in mc.CIRCUITS])
def test_failure_lists_equal_the_model(gl, ctx, name):
    import torch
    case = mc.Case(name)
    cs, k, w = case.cs, case.k, case.w
    assert case.clean == []
    mock = h2.MockProver(ctx, cs, k, w.fixed, case.mapping)
    recs, total = mock.check(w.advice, case.instances)
    assert (records(recs), total) == ([], 0)
    mock.assert_satisfied(w.advice, case.instances)
    if k <= 9:
        assert proof_accepted(gl, ctx, case, w.fixed, w.advice, case.instances)
    map_d = torch.from_numpy(np.ascontiguousarray(case.mapping).view(np.int32)).cuda()
    met = 0
    for cls in mc.CLASSES:
        m = case.mutation(cls)
        if m is None:
            assert not case.applies(cls)
            continue
        met += 1
        want = m["failures"]
        assert want, (name, cls)                                    # the cap (tests/test_halo2_mock_model.py checks it on the CPU too)
        adv, fixed = case.advice_array(m), case.fixed_array(m)
        mp = mock if m["fixed"] is None else h2.MockProver(ctx, cs, k, fixed, case.mapping)
        recs, total = mp.check(adv, m["instances"], capacity=len(want) + 32)
        got = records(recs)
        print("%s %s: model %d failures, device %d" % (name, cls, len(want), total))
        assert total == len(want) and got == want, (name, cls, got[:6], want[:6])
        # names resolved on the host
        for f in mp.verify(adv, m["instances"]):
            if f.kind in (h2.FAIL_GATE, h2.FAIL_GATE_POISONED):
                assert cs.gates[[g[0] for g in cs.gates].index(f.name)][1][f.position] is cs.all_gate_polys()[f.index]
        # a capacity below the total: the exact prefix, the exact total; capacity 0: yes / no
        # (a list of ONE record has no capacity strictly between 0 and the total: test_many_failures_and_every_capacity covers long lists)
        for cap in sorted(c for c in {1, len(want) // 2, len(want) - 1} if 0 < c < len(want)):
            r2, t2 = mp.check(adv, m["instances"], capacity=cap)
            assert t2 == len(want) and records(r2) == want[:cap], (name, cls, cap)
        assert mp.check(adv, m["instances"], capacity=0)[1] == len(want)
        # again, and with every input resident on the device: the same words
        r3, t3 = mp.check(adv, m["instances"], capacity=len(want) + 32)
        assert t3 == total and np.array_equal(r3, recs)
        adv_d = torch.from_numpy(adv.view(np.int64)).cuda()
        fix_d = torch.from_numpy(fixed.view(np.int64)).cuda()
        r4, t4 = h2.MockProver(ctx, cs, k, fix_d.data_ptr(), map_d.data_ptr()).check(adv_d.data_ptr(), m["instances"], capacity=len(want) + 32)
        assert t4 == total and np.array_equal(r4, recs)
        assert np.array_equal(adv_d.cpu().numpy().view(np.uint64), adv)          # advice is not modified
        with pytest.raises(h2.NotSatisfied):
            mp.assert_satisfied(adv, m["instances"])
        if k <= 9:
            if mc.poison_only(want):
                continue          # poison only: the proof may verify by luck of the blinding values; the check flags it (asserted above)
            assert not proof_accepted(gl, ctx, case, fixed, adv, m["instances"]), (name, cls)
    assert met >= 2


def test_no_mapping_means_no_copy_check(ctx):
    case = mc.Case("tuple-k7")
    m = case.mutation("copy_member")
    rest = [f for f in m["failures"] if f[0] != h2.FAIL_PERMUTATION]
    assert len(rest) < len(m["failures"])
    recs, total = h2.MockProver(ctx, case.cs, case.k, case.w.fixed, None).check(case.advice_array(m), m["instances"])
    assert total == len(rest) and records(recs) == rest


def test_prove_with_check_raises_instead_of_proving(gl, ctx):
    case = mc.Case("chips-k7")
    g, gl_, _ = params(ctx, case.k)
    plain = h2.PlonkProver(ctx, case.cs, case.k, g, gl_, case.w.fixed, case.mapping)
    with pytest.raises(ValueError):
        plain.prove(case.w.advice, case.instances, bytes(32), check=True)
    plain.close()
    prover = h2.PlonkProver(ctx, case.cs, case.k, g, gl_, case.w.fixed, case.mapping, checkable=True)
    seed = bytes(32)
    assert prover.prove(case.w.advice, case.instances, seed, check=True) == prover.prove(case.w.advice, case.instances, seed)
    m = case.mutation("gate_cell")
    with pytest.raises(h2.NotSatisfied) as ei:
        prover.prove(case.advice_array(m), m["instances"], seed, check=True)
    assert ei.value.total == len(m["failures"]) and "gate '" in str(ei.value) and "row %d" % m["failures"][0][2] in str(ei.value)
    prover.close()


def test_many_failures_and_every_capacity(ctx):
    """k = 12, a whole advice column zeroed: thousands of records over bitmaps that span several blocks of the count / scan / extraction
    kernels.  The complete list equals the model's full evaluation, and capacities around lane, block and total boundaries return the exact prefix."""
    from halo2_mock_model import MockModel
    ch = importlib.import_module("stark-verifier_amd.halo2_chips")
    k = 12
    cs, cfg, w = ch.synthetic_circuit(k, table_bits=9, n_permutations=2, seed=0x355)
    adv = w.advice.copy()
    adv[cfg.arithmetic_config.r.index, :w.usable] = 0
    adv[cfg.arithmetic_config.q_limbs[1].index, 5:w.usable:7, 0] = 1 << 9          # outside the 9-bit table
    mapping = w.assembly.mapping_array()
    want = MockModel(cs, k, w.fixed_ints(), mapping).verify([h2.from_limbs(adv[c]) for c in range(cs.num_advice)], w.instance)
    kinds = {f[0] for f in want}
    assert len(want) > 5000 and kinds == {h2.FAIL_GATE, h2.FAIL_LOOKUP, h2.FAIL_PERMUTATION}
    mp = h2.MockProver(ctx, cs, k, w.fixed, mapping)
    recs, total = mp.check(adv, w.instance, capacity=len(want) + 7)
    assert total == len(want) and records(recs) == want
    for cap in (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, len(want) - 1, len(want)):
        r, t = mp.check(adv, w.instance, capacity=cap)
        assert t == len(want) and records(r) == want[:cap], cap
    assert mp.check(adv, w.instance, capacity=0)[1] == len(want)


def test_errors(ctx):
    """a truncated descriptor and a mapping entry >= n are GL355_E_INVALID_ARG; an unsatisfied witness is not an error"""
    case = mc.Case("chips-k7")
    cs, k, w = case.cs, case.k, case.w
    desc = h2.export_desc(cs, k, 0)
    flat = h2.to_limbs([v for c in case.instances for v in c])
    lens = np.array([len(c) for c in case.instances] + [0], dtype=np.uint32)
    mapping = np.ascontiguousarray(case.mapping)
    total = C.c_uint64(0)

    def call(d, mp):
        return ctx.lib.gl355_plonk_check_witness(ctx.h, d.ctypes.data, d.size, w.fixed.ctypes.data, mp.ctypes.data, w.advice.ctypes.data, flat.ctypes.data, lens.ctypes.data,
                                                 None, 0, C.byref(total), None)
    assert call(desc, mapping) == 0 and total.value == 0
    assert call(desc[:-3].copy(), mapping) == -1
    assert call(desc[:20].copy(), mapping) == -1
    bad = desc.copy(); bad[0] ^= np.uint64(1)
    assert call(bad, mapping) == -1
    m2 = mapping.copy(); m2[0, 0, 1] = 1 << k
    assert call(desc, m2) == -1
    m2 = mapping.copy(); m2[1, 3, 0] = len(cs.permutation)
    assert call(desc, m2) == -1
    assert call(desc, mapping) == 0 and total.value == 0
