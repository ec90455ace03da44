"""GPU: part 3 of the Halo2 verifier circuit on the device.  gl355_halo2_synthesize against the host replay, word for word and with the same
status, on Plonky2VerifierCircuit over three real proofs, on the public-inputs hasher and on the gate constrainers; every mutation fails with
the host's (first, count).  The run form (halo2_run_kernel: a run of narrow levels in one launch) under GL355_HALO2_RUN_MAX unset, 0 and 1,
each in a fresh child process, on the hasher and verifier tapes and on synthetic tapes aimed at where such a kernel can go wrong: all
settings must give the host replay's columns and status.  One circuit end to end at k = 17 with the 12 public inputs as instances."""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halo2_verifier_cases as hv
from test_gpu_halo2_fri import TAU, device_equals_host

pytestmark = pytest.mark.gpu
hg, h2, K = hv.hg, hv.h2, hv.K
HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = {"unset": None, "off": "0", "one": "1"}


def inputs_of(rec):
    return np.array(rec.inputs, dtype=np.uint64)


@pytest.mark.parametrize("name", ["zk", "plain", "all_gates"])
def test_verifier_circuit_device_equals_host(ctx, name):
    c = hv.verifier_case(name)
    assert device_equals_host(ctx, c.rec.tape(), c.rec.k, c.inputs) == c.rec.status() == (hg.NO_FAILURE, 0)


@pytest.mark.parametrize("n", hv.HASH_LENGTHS)
def test_hasher_device_equals_host(ctx, n):
    rec = hv.hasher_case(n)[0]
    assert device_equals_host(ctx, rec.tape(), rec.k, inputs_of(rec)) == rec.status() == (hg.NO_FAILURE, 0)


@pytest.mark.parametrize("vector", [0, 1], ids=["random", "edge"])
def test_gate_constrainers_device_equal_host(ctx, vector):
    for name in sorted(hv.GATES):
        rec = hv.gate_case(name, vector)[0]
        assert device_equals_host(ctx, rec.tape(), rec.k, inputs_of(rec)) == rec.status() == (hg.NO_FAILURE, 0), name
    for num_selectors in (2, 1):
        rec = hv.filtered_case(num_selectors, vector)[0]
        assert device_equals_host(ctx, rec.tape(), rec.k, inputs_of(rec)) == rec.status() == (hg.NO_FAILURE, 0)


def test_mutations_fail_as_on_the_host(ctx):
    c = hv.verifier_case("all_gates")
    tape = hg.DeviceTape(ctx, c.rec.tape(), c.rec.k, len(c.inputs))
    try:
        for name, bad in hv.verifier_mutations("all_gates").items():
            advice, status = tape.synthesize(bad)
            host, host_status = hg.synthesize_host(c.rec.tape(), c.rec.k, bad)
            assert status == host_status and status[1] >= 1, name
            assert np.array_equal(advice, host), name
    finally:
        tape.close()


# ---- the run form ---------------------------------------------------------------------------------------------------------------------------
RUN_MAX = {"unset": 256, "off": 0, "one": 1}                        # what each setting puts in force; 256 is the default DESIGN.md states


def launches_of(rec, run_max):
    """the rule as the issue words it, over the recorder's own levels: a level belongs to a run when it has no PERMUTE entry and at most
    run_max entries; maximal runs of at least two such levels are one launch each, every other level is one launch"""
    widths = rec.level_widths()
    permute = {e[0] for e in rec.entries if e[2] == hg.OP_PERMUTE}
    narrow = [bool(run_max) and w <= run_max and level not in permute for level, w in zip(sorted({e[0] for e in rec.entries}), widths)]
    runs = [len(list(g)) for flag, g in itertools.groupby(narrow) if flag]
    runs = [n for n in runs if n >= 2]
    return dict(run_max=run_max, levels_in_runs=sum(runs), runs=len(runs), launches=len(widths) - sum(runs) + len(runs))


@pytest.fixture(scope="module")
def run_tapes(tmp_path_factory):
    """-> (path of the .npz the children read, {name: [sha256 of the host replay's columns, first, count]}, {name: recorder}); every tape is
    also held against its recorder here, once.  The real tapes: the hasher at every length, Plonky2VerifierCircuit on all three proofs
    (all_gates: all 12 constrainers, more than one selector), the vanishing identity alone (fails), and the all_gates tape on each of its
    one-word mutations, so that a failing status comes out of real runs too"""
    recs = {"hasher_%d" % n: hv.hasher_case(n)[0] for n in hv.HASH_LENGTHS}
    recs.update({"verifier_" + name: hv.verifier_case(name).rec for name in ("zk", "plain", "all_gates")})
    recs["vanishing_alone"] = hv.vanishing_alone_case()[0]
    recs.update({name: hv.run_case(name) for name in hv.RUN_CASES})
    cases = {name: (rec, inputs_of(rec), rec.status(), rec.advice()) for name, rec in recs.items()}
    for name, bad in hv.verifier_mutations("all_gates").items():
        cases["mutated_" + name] = (recs["verifier_all_gates"], bad, None, None)
    arrays, want = {}, {}
    for name, (rec, inputs, rec_status, rec_advice) in cases.items():
        tape = rec.tape()
        advice, status = hg.synthesize_host(tape, rec.k, inputs)
        assert rec.k == K, name
        if rec_status is None:
            assert status[1] >= 1, name
        else:
            assert status == rec_status and np.array_equal(advice, rec_advice), name
        arrays["tape_" + name], arrays["k_" + name], arrays["inputs_" + name] = tape, np.uint64(rec.k), inputs
        want[name] = [hashlib.sha256(np.ascontiguousarray(advice).tobytes()).hexdigest(), status[0], status[1]]
    path = str(tmp_path_factory.mktemp("run_form") / "tapes.npz")
    np.savez(path, **arrays)
    return path, want, {name: case[0] for name, case in cases.items()}


def test_run_cases_are_what_they_claim():
    """the shape of the synthetic tapes: the widths, the PERMUTE level, the two failing assertions in different levels, the tape that is one run"""
    widths = hv.run_case("widths").level_widths()
    assert widths[1:] == list(hv.RUN_WIDTHS) * 2
    chain = hv.run_case("chain").level_widths()
    assert len(chain) == 3001 and set(chain[1:]) == {1}
    seams = hv.run_case("seams")
    permute_levels = {e[0] for e in seams.entries if e[2] == hg.OP_PERMUTE}
    assert len(permute_levels) == 1 and seams.level_widths()[min(permute_levels) - 1] == 1
    assert seams.level_widths() == [5006, 3, 2, 4, 4, 1, 4, 2, 5000, 1, 4999, 2, 2]      # PACK, PERMUTE and UNPACK are levels 5 to 7
    ops = hv.run_case("ops")
    failing = [e for e in ops.entries if e[5]]
    assert ops.status()[1] == 2 and len({e[0] for e in failing}) == 2 and max(ops.level_widths()) <= 64
    assert {hg.OP_PACK, hg.OP_UNPACK, hg.OP_VALUE, hg.OP_ASSERT_EQ} <= {e[2] for e in ops.entries} and not any(e[2] == hg.OP_PERMUTE for e in ops.entries)
    kinds = {int(w) >> 60 for e in ops.entries if e[2] in (hg.OP_VALUE, hg.OP_MULADD) for w in e[4]}
    assert {hg.K_INV, hg.K_INV_EXT} <= kinds
    one = hv.run_case("one_run")
    assert max(one.level_widths()) <= 4 and len(one.level_widths()) > 40 and not any(e[2] in (hg.OP_PERMUTE, hg.OP_CONST) for e in one.entries)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_run_form_gives_the_host_replay(run_tapes, setting):
    path, want, recs = run_tapes
    env = dict(os.environ)
    env.pop("GL355_HALO2_RUN_MAX", None)
    if SETTINGS[setting] is not None:
        env["GL355_HALO2_RUN_MAX"] = SETTINGS[setting]
    child = subprocess.run([sys.executable, os.path.join(HERE, "halo2_run_child.py"), path], env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    got = json.loads(child.stdout.strip().split("\n")[-1])
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name][1:3] == want[name][1:], "%s: status %r, the host replay's %r" % (name, got[name][1:3], want[name][1:])
        assert got[name][0] == want[name][0], "%s: the columns differ from the host replay's" % name
        # what the library says it launched (the list gl355_halo2_synthesize walks) is the rule applied to the recorder's levels
        assert got[name][3] == launches_of(recs[name], RUN_MAX[setting]), name
    assert want["ops"][2] == 2 and want["ops"][1] == hv.run_case("ops").status()[0]
    assert all(want[name][2] >= 1 for name in want if name.startswith("mutated_")) and want["vanishing_alone"][2] >= 1
    # by hand, so that the rule above is held against something too: the seams tape (widths in test_run_cases_are_what_they_claim)
    levels = {"unset": (8, 3, 8), "off": (0, 0, 13), "one": (0, 0, 13)}[setting]
    assert (got["seams"][3]["levels_in_runs"], got["seams"][3]["runs"], got["seams"][3]["launches"]) == levels
    chain = got["chain"][3]
    if setting == "off":
        assert all(g[3]["runs"] == 0 and g[3]["levels_in_runs"] == 0 for g in got.values())
    else:                                                            # the run kernel did the work: 3 000 levels of one entry in one launch
        assert chain["runs"] == 1 and chain["levels_in_runs"] >= 3000 and chain["launches"] <= 2
    if setting == "unset":
        assert got["one_run"][3]["launches"] == 1
        assert all(got[name][3]["runs"] >= 1 for name in got if name.startswith(("hasher_1", "verifier_", "mutated_")))


def test_end_to_end_at_k17(ctx):
    """from_artifact -> prove_from_inputs(check=True) -> gl355_plonk_verify with the 12 public inputs as instances; refused with one changed"""
    c = hv.verifier_case("plain")
    rec = c.rec
    g, g_lagrange = h2.kzg_setup(ctx, rec.k, TAU)
    prover = h2.PlonkProver.from_artifact(ctx, rec.artifact(), g, g_lagrange, checkable=True)
    try:
        proof, status = prover.prove_from_inputs(c.inputs, [rec.instance], bytes(range(32)), check=True)
        assert status == (hg.NO_FAILURE, 0)
        vk = prover.verifying_key(h2.kzg_setup_g2(TAU))
        assert rec.instance == [int(v) for v in c.pi] and len(rec.instance) == 12
        assert vk.verify([rec.instance], proof), vk.last_error
        changed = list(rec.instance)
        changed[5] ^= 1
        assert vk.verify([changed], proof) is False
    finally:
        prover.close()
