"""SURVEY 8(f) N4 at size: a synthetic circuit with the reference's column / gate / lookup shape (halo2_chips.AllChipConfig: 19 advice and 13 fixed
columns, 12 permutation columns, nine 16-bit range lookups, degree 6) at k = argv[1:] (default 17 20 23; the reference finalises at k = 23:
README.md:171-177, 505-511 s on 16 vCPUs) through gl355_plonk_keygen / gl355_plonk_prove on cuda:0, every proof checked by the restated
halo2 verifier (tests/halo2_verifier.py; pairing check in the exponent under the known tau) and by the native one (gl355_plonk_verify under
[tau] G2, host only: native_verified, native_verify_ms and its split into transcript + expressions / MSM / pairing).  One JSON line per k.
`--check` with the k values: the same run also puts the same witness through gl355_plonk_check_witness (MockProver), inputs resident on the
device, warm, best of five, once clean and once with one advice cell broken: check_witness_ms, its three stage times, the host-to-device time
of its inputs on its own, and the ratio to create_proof + native verify -- the only way to tell a bad witness without it (the restated Python
verifier is skipped in this mode).
`--batch` instead of k values: the batch verifier's numbers at k = 12 (batches of 32 and 256, device against host MSM, the MSM alone over a
range of term counts) and gl355_kzg_params_check at k = 20 and 23, one JSON line.
`--synth [openings] [fri] [--levels DIR] [--no-synthetic]` instead of k values: witness synthesis of FriOpeningsCircuit and FriVerifierCircuit
(halo2_verifier_circuit.py) over one wrap proof: gl355_halo2_synthesize with the inputs and the columns resident (one warm-up, best of five, all
five kept) against gl355_halo2_synthesize_host on one thread plus the upload of the same columns from pageable host memory -- what a caller
without the device path pays; rows, k, entries, levels and their widths; the status must be NO_FAILURE and gl355_plonk_check_witness must find
nothing; create_proof on the synthesised witness against synthetic_circuit at the same k (--no-synthetic leaves that out).  One JSON line per
circuit.  --levels DIR also writes per level [entries, PERMUTE entries] (the launches of one synthesis, in order) and the tape with its inputs
there: what a kernel trace of the run is joined with (profiles/halo2_synth_fri.txt).  `verifier` among the circuits is Plonky2VerifierCircuit (part 3);
`--aggregate N` takes, instead of the wrap of one Semaphore signal, the wrap of an aggregation of N signals (4 + 8 N public inputs: the
reference's own benchmark flow with N = 128), the circuits' names then end in _aggN.  Every line also says how many levels fall into runs and
how many runs and launches there are under the run_max in force, as the library itself reports them (gl355_halo2_tape_launches).
`--tapes DIR`: device synthesis alone (one warm-up, best of five) of every tape_*.npz a `--synth --levels DIR` run left there, one JSON line per
tape: cheap enough to start one process per setting of GL355_HALO2_RUN_MAX / GL355_HALO2_SPREAD_MAX and alternate them
(profiles/halo2_synth_verifier.txt)."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TAU = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF


def run(gl, ctx, k, verify=True, reps=2, check=False):
    import torch
    h2 = importlib.import_module("stark-verifier_amd.halo2")
    ch = importlib.import_module("stark-verifier_amd.halo2_chips")
    out = {"k": k}
    t0 = time.perf_counter()
    cs, cfg, w = ch.synthetic_circuit(k, table_bits=min(16, k - 1), n_permutations=64 if k >= 14 else 4)
    out["witness_host_s"] = round(time.perf_counter() - t0, 2)
    n = 1 << k
    torch.cuda.empty_cache()
    used_before = (torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9       # whatever else lives on the device (other bench blocks' contexts)
    # the SRS stays on the device (ParamsKZG::setup, verifier_api.rs:77)
    g = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    gl_ = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tau = h2.to_limbs([TAU % h2.R])[0]
    ctx.check(ctx.lib.gl355_kzg_setup(ctx.h, tau.ctypes.data, k, g.data_ptr(), gl_.data_ptr()))
    ctx.sync()
    out["kzg_setup_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    prover = h2.PlonkProver(ctx, cs, k, g.data_ptr(), gl_.data_ptr(), w.fixed, w.assembly.mapping_array())
    out["keygen_s"] = round(time.perf_counter() - t0, 3)
    out.update({"extended_k": prover.info["extended_k"], "proof_bytes": prover.info["proof_bytes"], "advice_columns": cs.num_advice, "fixed_columns": cs.num_fixed,
                "permutation_columns": len(cs.permutation), "lookups": len(cs.lookups), "degree": cs.degree(), "gate_polynomials": len(cs.all_gate_polys())})
    adv = torch.from_numpy(w.advice.view(np.int64)).cuda()          # witness resident: create_proof's timed region starts with the columns in HBM
    torch.cuda.synchronize()
    best = None
    for r in range(reps):
        t0 = time.perf_counter()
        proof, ms = prover.prove(adv.data_ptr(), w.instance, bytes([r] * 32), timed=True)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, ms, proof)
    out["create_proof_s"] = round(best[0], 3)
    out["stage_ms"] = {k_: round(v, 1) for k_, v in best[1].items()}
    used = (torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9
    out["gpu_mem_GB"] = round(used - used_before, 1)             # SRS + proving key + witness + everything the proofs allocated (allocator cache included)
    out["gpu_mem_device_total_used_GB"] = round(used, 1)
    # the native verifier (verify_proof with VerifierSHPLONK, chip/native_chip/test_utils.rs:82-93): host only, best of three
    nv = prover.verifying_key(h2.kzg_setup_g2(TAU % h2.R))
    nbest = None
    for _ in range(3):
        t0 = time.perf_counter()
        ok = nv.verify(w.instance, best[2])
        dt = (time.perf_counter() - t0) * 1e3
        if nbest is None or dt < nbest[0]:
            nbest = (dt, nv.stage_ms())
    out["native_verified"] = bool(ok)
    out["native_verify_ms"] = round(nbest[0], 3)
    out["native_verify_stage_ms"] = {k_: round(v, 3) for k_, v in nbest[1].items()}
    nv.close()
    if verify:
        import halo2_verifier as hv
        pt = lambda a: (lambda x, y: None if (x, y) == (0, 0) else (x, y))(h2.from_limbs(a[:4])[0], h2.from_limbs(a[4:])[0])      # noqa: E731
        vk = dict(digest=prover.digest, fixed_commitments=[pt(c) for c in prover.fixed_commitments], sigma_commitments=[pt(c) for c in prover.sigma_commitments])
        t0 = time.perf_counter()
        out["verified"] = bool(hv.verify(k, cs, vk, w.instance, best[2], TAU % h2.R))
        out["verify_host_s"] = round(time.perf_counter() - t0, 2)
    if check:
        out["check"] = run_check(ctx, h2, cs, cfg, w, k, adv, (out["create_proof_s"] * 1e3 + out["native_verify_ms"]))
    prover.close()
    del adv, g, gl_
    torch.cuda.empty_cache()
    return out


def run_check(ctx, h2, cs, cfg, w, k, adv, prove_verify_ms, reps=5):
    """gl355_plonk_check_witness on the witness `adv` (device) that was just proved: device-resident inputs, one warm-up call, best of `reps`"""
    import torch
    out = {}
    mapping = np.ascontiguousarray(w.assembly.mapping_array())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fixed_d = torch.from_numpy(w.fixed.view(np.int64)).cuda()
    map_d = torch.from_numpy(mapping.view(np.int32)).cuda()
    adv_again = torch.from_numpy(w.advice.view(np.int64)).cuda()
    torch.cuda.synchronize()
    out["h2d_ms"] = round((time.perf_counter() - t0) * 1e3, 1)          # fixed + mapping + advice from pageable host memory: not part of check_witness_ms
    del adv_again
    mp = h2.MockProver(ctx, cs, k, fixed_d.data_ptr(), map_d.data_ptr())
    broken = adv.clone()
    row = 5
    broken[cfg.arithmetic_config.c.index, row, 0] += 1                 # one cell of an active "base field constraint" row
    torch.cuda.synchronize()
    for name, a in (("clean", adv), ("broken", broken)):
        mp.check(a.data_ptr(), w.instance, 64)                          # warm: the context's allocator holds the buffers afterwards
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            recs, total = mp.check(a.data_ptr(), w.instance, 64)
            dt = (time.perf_counter() - t0) * 1e3
            if best is None or dt < best[0]:
                best = (dt, dict(mp.stage_ms))
        out[name] = {"check_witness_ms": round(best[0], 2), "stage_ms": {k_: round(v, 2) for k_, v in best[1].items()}, "failures": int(total),
                     "first": [h2.describe_failure(mp._resolve(r)) for r in recs[:2]]}
    out["check_witness_ms"] = out["clean"]["check_witness_ms"]
    out["prove_plus_native_verify_ms"] = round(prove_verify_ms, 1)
    out["ratio_to_prove_plus_verify"] = round(out["check_witness_ms"] / prove_verify_ms, 4)
    del fixed_d, map_d, broken
    return out


def timed(f, reps=3):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None or dt < best else best
    return r, round(best, 3)


def run_batch(gl, ctx, k=12):
    """verify_batch of 32 and 256 proofs of the reference's chip shape against n x one proof, with the device and the host MSM; the MSM alone
    (host sum against gl355_bn254_g1_msm from host arrays) over term counts -- the figure behind PLONK_VERIFY_DEVICE_MSM_MIN; the parameter check"""
    h2 = importlib.import_module("stark-verifier_amd.halo2")
    ch = importlib.import_module("stark-verifier_amd.halo2_chips")
    out = {"k": k}
    cs, cfg, w = ch.synthetic_circuit(k, table_bits=k - 1, n_permutations=4)
    g, gl_ = h2.kzg_setup(ctx, k, TAU % h2.R)
    prover = h2.PlonkProver(ctx, cs, k, g, gl_, w.fixed, w.assembly.mapping_array())
    nv = prover.verifying_key(h2.kzg_setup_g2(TAU % h2.R))
    proofs = [prover.prove(w.advice, w.instance, bytes([b & 0xFF, b >> 8] * 16)) for b in range(256)]
    ok, one = timed(lambda: nv.verify(w.instance, proofs[0]), 5)
    out["single"] = {"ok": ok, "ms": one, "stage_ms": nv.stage_ms(), "proof_bytes": len(proofs[0])}
    for nb in (32, 256):
        insts = [w.instance] * nb
        ok_d, ms_d = timed(lambda: nv.verify_batch(ctx, insts, proofs[:nb], seed=bytes(32)))
        st_d = nv.stage_ms()
        ok_h, ms_h = timed(lambda: nv.verify_batch(None, insts, proofs[:nb], seed=bytes(32)))
        st_h = nv.stage_ms()
        out["batch_%d" % nb] = {"ok": ok_d and ok_h, "device_msm_ms": ms_d, "device_stage_ms": st_d, "host_msm_ms": ms_h, "host_stage_ms": st_h,
                                "n_times_single_ms": round(nb * one, 1)}
    # the combined MSM alone (stage time of verify_batch), forced to the device against the host sum, over batch sizes: the figure behind
    # PLONK_VERIFY_DEVICE_MSM_MIN (plonk_verifier.cpp)
    cl = cs.chunk_len()
    per_proof = cs.num_advice + 3 * len(cs.lookups) + (len(cs.permutation) + cl - 1) // cl + 1 + (cs.degree() - 1) + 2
    sweep = {}
    for nb in (1, 2, 4, 8, 16, 32, 64, 128):
        insts = [w.instance] * nb
        os.environ["GL355_PLONK_VERIFY_DEVICE_MSM_MIN"] = "0"
        msd = min(nv.stage_ms()["msm"] for _ in range(3) if nv.verify_batch(ctx, insts, proofs[:nb], seed=bytes(32)))
        del os.environ["GL355_PLONK_VERIFY_DEVICE_MSM_MIN"]
        msh = min(nv.stage_ms()["msm"] for _ in range(3) if nv.verify_batch(None, insts, proofs[:nb], seed=bytes(32)))
        sweep[nb] = {"terms": nb * per_proof + cs.num_fixed + len(cs.permutation) + 1, "device_msm_ms": round(msd, 3), "host_msm_ms": round(msh, 3)}
    out["msm_sweep"] = sweep
    prover.close()
    for kk in (20, 23):
        gg, ll = h2.kzg_setup(ctx, kk, TAU % h2.R)
        s2 = h2.kzg_setup_g2(TAU % h2.R)
        okp, msp = timed(lambda: h2.kzg_params_check(ctx, gg, s2, kk, seed=bytes(32)), 1)
        okl, msl = timed(lambda: h2.kzg_params_check(ctx, gg, s2, kk, g_lagrange=ll, seed=bytes(32)), 1)
        out["params_check_k%d" % kk] = {"ok": okp and okl, "powers_ms": msp, "powers_and_lagrange_ms": msl}
        del gg, ll
    return out


def wrap_proof(gl, ctx):
    """a Semaphore proof wrapped under the BN254-Poseidon config (wrapper.rs:35-56) -> (the wrap circuit, its flat proof, its public inputs)"""
    from oracle_lib import rand_field
    from test_gpu_prover import make_access_set
    rcn = importlib.import_module("stark-verifier_amd.recursion")
    aset, sks, rng = make_access_set(gl, ctx, 3, 0x2542)
    sig, data = aset.make_signal_fast(sks[4], rand_field(rng, 4), 4, 3, flat_only=True)
    inner = (sig.proof, np.concatenate([aset.tree.cap[0], sig.nullifier[0], sig.topics[0]]))
    wc = rcn.WrapperCircuit(ctx, data.common()).build([inner], rng)
    flat, pis = wc.prove_flat([inner], seed=17)
    return wc, flat, pis


def aggregate_wrap_proof(gl, ctx, n_signals):
    """n_signals Semaphore signals of one access set -> the aggregation tree (recursion.rs:187-247) -> its BN254-Poseidon wrap
    -> (the wrap circuit, its flat proof, its 4 + 8 n_signals public inputs)"""
    from oracle_lib import rand_field
    rcn = importlib.import_module("stark-verifier_amd.recursion")
    sem = importlib.import_module("stark-verifier_amd.semaphore")
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    assert n_signals >= 2 and n_signals & (n_signals - 1) == 0
    rng = np.random.default_rng(0x2543)
    sks = rand_field(rng, (n_signals, 4))
    keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
    aset = sem.AccessSet(ctx, keys)
    topic = rand_field(rng, 4)
    data, rows = aset.build(rng)
    idx, _, _ = aset.witness_rows(rows, sks[0], topic, 0)
    semc = plonk.NativeCircuit(ctx, data.export_blob(idx))
    leaves, proofs, _ = plonk.semaphore_units([ctx], semc, None, sks, topic, aset.tree.digests, np.arange(n_signals, dtype=np.uint64), 7000, want_proofs=True)
    signals = [(proofs[j], np.concatenate([aset.tree.cap[0], leaves[j]])) for j in range(n_signals)]
    proof, pis, cd = rcn.Aggregator(ctx, data.common()).aggregate(signals, seed=100, rng=rng)
    wc = rcn.WrapperCircuit(ctx, cd).build([(proof, pis)], rng)
    flat, wpis = wc.prove_flat([(proof, pis)], seed=17)
    assert wpis.size == 4 + 8 * n_signals
    return wc, flat, wpis


def time_synthesis(ctx, tape, k, inputs):
    """one warm-up, five timed calls with the inputs and the columns resident -> (sorted ms, status, the columns on the device, the DeviceTape)"""
    import torch
    hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
    dt = hg.DeviceTape(ctx, tape, k, inputs.size)
    d_in = torch.from_numpy(inputs.view(np.int64)).cuda()
    dev = torch.empty((hg.N_ADVICE, 1 << k, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _, status = dt.synthesize(d_in.data_ptr(), out=dev.data_ptr())                 # warm
    runs = sorted(timed(lambda: dt.synthesize(d_in.data_ptr(), out=dev.data_ptr()), 1)[1] for _ in range(5))
    return runs, status, dev, d_in, dt


def run_tapes(gl, ctx, directory):
    """device synthesis alone of every tape_*.npz in `directory` -> one dict per tape"""
    hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
    outs = []
    for f in sorted(os.listdir(directory)):
        if not (f.startswith("tape_") and f.endswith(".npz")):
            continue
        z = np.load(os.path.join(directory, f))
        name = f[5:-4]
        runs, status, dev, d_in, dt = time_synthesis(ctx, z["tape"], int(z["k"][0]), z["inputs"])
        levels = np.load(os.path.join(directory, "levels_%s.npy" % name))
        outs.append({"circuit": name, "k": int(z["k"][0]), **dt.launches(),
                     "spread_max": os.environ.get("GL355_HALO2_SPREAD_MAX", "default"), "levels": len(levels), "device_synthesis_ms": runs[0], "device_synthesis_ms_runs": runs,
                     "status": [int(status[0]) if status[0] != hg.NO_FAILURE else -1, status[1]],
                     "columns_word_sum": int(dev.sum().item()) & 0xFFFFFFFFFFFFFFFF})
        dt.close()
        del dev, d_in
    return outs


def level_table(rec):
    """per level of the tape: [entries, PERMUTE entries] (the order of gl355_halo2_synthesize's launches)"""
    hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
    t = rec.tape().reshape(-1, 8)
    level, op = (t[:, 0] >> np.uint64(8)).astype(np.int64), (t[:, 0] & np.uint64(0xFF)).astype(np.int64)
    return np.stack([np.bincount(level)[1:], np.bincount(level, weights=(op == hg.OP_PERMUTE))[1:].astype(np.int64)], axis=1)


def synth_circuit(gl, ctx, name, circuit, inputs, out, levels_dir=None):
    """record `circuit` from `inputs`, then: device synthesis against host replay + upload, the status, gl355_plonk_check_witness on the resident
    columns, create_proof at that k and the native verifier"""
    import torch
    h2 = importlib.import_module("stark-verifier_amd.halo2")
    hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
    t0 = time.perf_counter()
    rec = circuit.record(inputs)
    out["record_s"] = round(time.perf_counter() - t0, 1)
    widths = rec.level_widths()
    k, tape = rec.k, rec.tape()
    levels = level_table(rec)
    assert [int(w) for w in levels[:, 0]] == widths
    with_permute = levels[:, 1] > 0
    out.update({"circuit": name, "k": k, "rows_used": rec.rows_used, "query_rounds": len(circuit.queries), "tape_entries": len(rec.entries), "tape_MB": round(tape.nbytes / 1e6, 1),
                "levels": len(widths), "entries_per_level": {"min": int(min(widths)), "median": int(np.median(widths)), "max": int(max(widths))},
                "levels_with_permute": int(with_permute.sum()), "levels_of_one_permute": int((levels[:, 1] == 1).sum()),
                "levels_one_entry_wide": int((levels[:, 0] <= 2).sum()), "instances": len(rec.instance)})
    if levels_dir:
        os.makedirs(levels_dir, exist_ok=True)
        np.save(os.path.join(levels_dir, "levels_%s.npy" % name), levels)
        np.savez(os.path.join(levels_dir, "tape_%s.npz" % name), tape=tape, inputs=inputs, k=np.array([k]))
    runs, status, dev, d_in, dt = time_synthesis(ctx, tape, k, inputs)
    out.update(dt.launches())                                        # run_max in force, levels in runs, runs, launches: the library's own list
    out["device_synthesis_ms"], out["device_synthesis_ms_runs"] = runs[0], runs
    out["status"] = [int(status[0]) if status[0] != hg.NO_FAILURE else -1, status[1]]
    assert status == (hg.NO_FAILURE, 0), "the circuit refuses the wrap proof: %r" % (status,)
    hg.synthesize_host(tape, k, inputs)                                            # warm
    (host, _), out["host_replay_ms"] = timed(lambda: hg.synthesize_host(tape, k, inputs), 5)       # one thread; validates the tape on every call
    out["device_equals_host"] = bool(np.array_equal(dev.cpu().numpy().view(np.uint64), host))

    def upload():
        t = torch.from_numpy(host.view(np.int64)).cuda()
        torch.cuda.synchronize()
        return t
    upload()
    _, out["upload_pageable_ms"] = timed(upload, 5)
    out["host_replay_plus_upload_ms"] = round(out["host_replay_ms"] + out["upload_pageable_ms"], 3)
    out["device_speedup"] = round(out["host_replay_plus_upload_ms"] / out["device_synthesis_ms"], 2)
    g, gl_ = h2.kzg_setup(ctx, k, TAU % h2.R)
    t0 = time.perf_counter()
    prover = h2.PlonkProver.from_artifact(ctx, rec.artifact(), g, gl_, checkable=True)
    out["layout_and_keygen_s"] = round(time.perf_counter() - t0, 1)
    fails = prover.mock_prover().verify(dev.data_ptr(), [rec.instance], 8)         # gl355_plonk_check_witness on the synthesised columns
    out["check_witness_failures"] = len(fails)
    assert not fails, [h2.describe_failure(f) for f in fails]
    prover.prove(dev.data_ptr(), [rec.instance], bytes(32))                        # warm
    proof, ms = timed(lambda: prover.prove(dev.data_ptr(), [rec.instance], bytes([1] * 32)), 5)
    out["create_proof_ms"] = ms
    nv = prover.verifying_key(h2.kzg_setup_g2(TAU % h2.R))
    out["native_verified"] = bool(nv.verify([rec.instance], proof))
    nv.close()
    prover.close()
    dt.close()
    del dev, d_in, g, gl_
    torch.cuda.empty_cache()
    return out


def run_synth(gl, ctx, which=("openings", "fri"), levels_dir=None, synthetic=True, aggregate=0):
    """-> one dict per circuit of `which`: FriOpeningsCircuit (part 1), FriVerifierCircuit (part 2) and Plonky2VerifierCircuit (part 3) over
    the same wrap proof: of one Semaphore signal, or of an aggregation of `aggregate` signals"""
    vc = importlib.import_module("stark-verifier_amd.halo2_verifier_circuit")
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    t0 = time.perf_counter()
    wc, flat, pis = aggregate_wrap_proof(gl, ctx, aggregate) if aggregate else wrap_proof(gl, ctx)
    proof_s = round(time.perf_counter() - t0, 1)
    cd = wc.data.common()
    outs = []
    for name in which:
        out = {"wrap_degree_bits": int(wc.data.degree_bits), "proof_words": int(flat.size), "public_inputs": int(len(pis)), "wrap_proof_s": proof_s}
        if name == "openings":
            circuit = vc.FriOpeningsCircuit(cd)
            inputs = circuit.inputs(flat)
        elif name == "fri":
            circuit = vc.FriVerifierCircuit(cd)
            inputs = circuit.inputs(flat, plonk.host_hash_no_pad(pis))
        else:
            circuit = vc.Plonky2VerifierCircuit(cd)
            inputs = circuit.inputs(flat, pis)
        synth_circuit(gl, ctx, name + ("_agg%d" % aggregate if aggregate else ""), circuit, inputs, out, levels_dir)
        if synthetic:
            out["create_proof_synthetic_circuit_ms"] = round(run(gl, ctx, out["k"], verify=False, reps=5)["create_proof_s"] * 1e3, 1)
        outs.append(out)
    return outs


if __name__ == "__main__":
    import torch
    torch.cuda.init()            # torch's bundled ROCm runtime first, then libgl355.so (tests/conftest.py has the reason)
    gl = importlib.import_module("stark-verifier_amd")
    ctx = gl.Context(0)
    if sys.argv[1:] == ["--batch"]:
        print(json.dumps(run_batch(gl, ctx)), flush=True)
        ctx.close()
        sys.exit(0)
    if sys.argv[1:2] == ["--tapes"]:
        for out in run_tapes(gl, ctx, sys.argv[2]):
            print(json.dumps(out), flush=True)
        ctx.close()
        sys.exit(0)
    if sys.argv[1:2] == ["--synth"]:
        rest = sys.argv[2:]
        levels_dir = rest[rest.index("--levels") + 1] if "--levels" in rest else None
        which = [a for a in rest if a in ("openings", "fri", "verifier")] or ["openings", "fri"]
        aggregate = int(rest[rest.index("--aggregate") + 1]) if "--aggregate" in rest else 0
        for out in run_synth(gl, ctx, which, levels_dir, synthetic="--no-synthetic" not in rest, aggregate=aggregate):
            print(json.dumps(out), flush=True)
        ctx.close()
        sys.exit(0)
    check = "--check" in sys.argv[1:]
    for k in [int(a) for a in sys.argv[1:] if a != "--check"] or [17, 20, 23]:
        print(json.dumps(run(gl, ctx, k, verify=not check, check=check)), flush=True)
    ctx.close()
