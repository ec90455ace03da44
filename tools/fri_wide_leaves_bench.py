#!/usr/bin/env python3
"""The leaf stage of a wide-arity FRI layer tree in its two forms, and the threshold between them (GL355_OPT_LEAF_LANES_LOG, option 7).
  python tools/fri_wide_leaves_bench.py [reps=5] [contexts=10] [units=160]
1. Solo: gl355_fri_prove of ONE layer that folds by 4 / 8 / 16 (leaves of 8 / 16 / 32 words) with 2^10 .. 2^20 leaves, the option at 0
   (fri_leaves_units_kernel + hash_leaves_kernel) and at 31 (fri_wide_leaves_units_kernel), both in the same run; the times are the
   gl355_profile_* scopes of the leaf stage alone.  Cap height 4 gives 16 cap subtrees, a lone unit's launch (psd_permute_lanes<3>); cap
   height 6 gives 64, the form a lock-step batch launches (<0>): the kernel indexes leaves over all units of a launch, so eight units of
   2^k leaves are the launch of one unit of 2^(k+3).
2. Ten contexts: units/s of gl355_semaphore_units at ConstantArityBits(3, 5), zero-knowledge on, with the option at 0 and at each candidate."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_CTX = int(sys.argv[2]) if len(sys.argv) > 2 else 10
UNITS = int(sys.argv[3]) if len(sys.argv) > 3 else 160
lib = importlib.import_module("stark-verifier_amd._lib").load(init_torch=False)
assert lib.gl355_runtime_config(0, N_CTX, 0) == 0
gl = importlib.import_module("stark-verifier_amd")
plonk = importlib.import_module("stark-verifier_amd.plonk")
sem = importlib.import_module("stark-verifier_amd.semaphore")
rec = importlib.import_module("stark-verifier_amd.recursion")
OPT, RATE_BITS, NQ = 7, 3, 3


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def leaf_stage_ms(ctx, coeffs, log_n, cap, ab, setting):
    ctx.set_option(OPT, setting)
    arity = np.array([ab], dtype=np.uint32)
    caps = np.zeros(4 << cap, dtype=np.uint64)
    final = np.zeros(2 * ((1 << log_n) >> ab), dtype=np.uint64)
    w, idx = C.c_uint64(), np.zeros(NQ, dtype=np.uint64)
    evals = np.zeros((NQ, 2 << ab), dtype=np.uint64)
    sibs = np.zeros((NQ, max(1, log_n + RATE_BITS - ab - cap), 4), dtype=np.uint64)

    def run():
        ch = plonk.Challenger(0)
        ctx.check(lib.gl355_fri_prove(ctx.h, ptr(coeffs), log_n, RATE_BITS, cap, ptr(arity), 1, 0, NQ, C.byref(ch.c), ptr(caps), ptr(final), C.byref(w),
                                      ptr(idx), ptr(evals), ptr(sibs)))
    run()
    ctx.sync()
    ctx.profile_enable(True)
    ctx.profile_read()
    for _ in range(REPS):
        run()
    ctx.sync()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    names = ("fri_wide_leaves_units_kernel",) if setting else ("fri_layer_leaves", "hash_leaves_kernel")
    assert all(prof.get(n, (0, 0.0, 0))[0] == REPS for n in names), (setting, {k: v[0] for k, v in prof.items()})
    return sum(prof[n][1] for n in names) / REPS, caps.copy()


def solo(ctx):
    rng = np.random.default_rng(1)
    for cap, what in ((4, "16 cap subtrees: a lone unit, psd_permute_lanes<3>"), (6, "64 cap subtrees: the form of a lock-step batch, psd_permute_lanes<0>")):
        print("leaf stage alone, ms per layer, %d repetitions; %s" % (REPS, what))
        print("%-8s" % "leaves" + "".join("  %2d words: pair   lanes  ratio" % (2 << ab) for ab in (2, 3, 4)))
        for log_nl in range(10, 21):
            line = "2^%-6d" % log_nl
            for ab in (2, 3, 4):
                log_n = log_nl + ab - RATE_BITS
                coeffs = rng.integers(0, plonk.P, size=2 << log_n, dtype=np.uint64)
                pair, caps0 = leaf_stage_ms(ctx, coeffs, log_n, cap, ab, 0)
                lanes, caps1 = leaf_stage_ms(ctx, coeffs, log_n, cap, ab, 31)
                assert np.array_equal(caps0, caps1)
                line += "           %7.3f %7.3f %6.2f" % (pair, lanes, lanes / pair)
            print(line, flush=True)


def ten_contexts(ctxs):
    ctx = ctxs[0]
    rng = np.random.default_rng(0x357)
    sks = gl.api.rand_field(rng, (1 << 20, 4))
    keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
    topic = gl.api.rand_field(rng, 4)
    aset = sem.AccessSet(ctx, keys)
    data, rows = aset.build(rng, config=plonk.CircuitConfig(reduction_arity_bits=3))
    idx, _, _ = aset.witness_rows(rows, sks[0], topic, 0)
    semc = plonk.NativeCircuit(ctx, data.export_blob(idx, wide_arity=True))
    flat0, pis0 = semc.semaphore_prove(ctx, sks[0], topic, 0, aset.tree.prove_host(0), 1)
    rc = rec.RecursiveCircuit(ctx, data.common(), k=1, config=plonk.CircuitConfig(reduction_arity_bits=3, use_interpolation_gate=True)).build([(flat0, pis0)], rng)
    recn = rc.native()
    members = np.arange(UNITS, dtype=np.uint64)
    print("gl355_semaphore_units at ConstantArityBits(3, 5), zero-knowledge on (both circuits 2^%d / 2^%d), %d contexts, %d units, units/s of three repetitions" % (
        data.degree_bits, rc.data.degree_bits, len(ctxs), UNITS))
    want = None
    for setting in (0, 12, 14, 16, 18, 20, 31, 0):
        for c in ctxs:
            c.set_option(OPT, setting)
        plonk.semaphore_units(ctxs, semc, recn, sks, topic, aset.tree.digests, members[:2 * len(ctxs)], 5000)
        rates = []
        for r in range(3):
            t0 = time.perf_counter()
            leaves, proofs, _ = plonk.semaphore_units(ctxs, semc, recn, sks, topic, aset.tree.digests, members, 6000, want_proofs=True)
            rates.append(UNITS / (time.perf_counter() - t0))
        want = proofs if want is None else want
        assert np.array_equal(proofs, want), "the option changed a proof"
        print("  option 7 = %-2d  %s" % (setting, " / ".join("%.1f" % v for v in rates)), flush=True)


def main():
    ctxs = [gl.Context(0) for _ in range(N_CTX)]
    for c in ctxs:
        c.set_option(2, 2)
        c.set_option(3, 2)
    solo(ctxs[0])
    ten_contexts(ctxs)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
