#!/usr/bin/env python3
"""Kernel-level yardstick of the constraint / quotient kernel (csrc/quotient.hip) on one GPU.
  python tools/quotient_time.py [--warmup 5] [--reps 20] [--only semaphore|recursive]
Builds the Semaphore circuit (2^13 rows, 2^16 points of the quotient coset) and the recursive verifier circuit (2^14 rows, 2^17 points,
all 11 gate kinds) the way tests/test_gpu_cpu_prover.py does, fills the wire and Z oracles with random field elements (the kernel has
no data-dependent branch), calls gl355_quotient_values --warmup times untimed and --reps times timed, and prints median / min / max
milliseconds per launch from the context's `quotient_kernel` profile scope (HIP events around the one kernel launch).
It is also the program to run under a hardware-counter pass (rocprofv3 --pmc ... -- python tools/quotient_time.py)."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gl = importlib.import_module("stark-verifier_amd")
api = importlib.import_module("stark-verifier_amd.api")
sem = importlib.import_module("stark-verifier_amd.semaphore")
rec = importlib.import_module("stark-verifier_amd.recursion")
from oracle_lib import rand_field  # noqa: E402


def circuits(ctx, only):
    """(name, CircuitData) of the two circuits; the recursive one verifies one Semaphore signal"""
    rng = np.random.default_rng(0x703)
    sks = rand_field(rng, (1 << 3, 4))
    keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
    aset = sem.AccessSet(ctx, keys)
    topic = rand_field(rng, 4)
    sig, data = aset.make_signal_fast(sks[2], topic, 2, 5, flat_only=True)
    if only in (None, "semaphore"):
        yield "semaphore", data
    if only in (None, "recursive"):
        inner = (sig.proof, np.concatenate([aset.tree.cap[0], sig.nullifier[0], sig.topics[0]]))
        yield "recursive", rec.RecursiveCircuit(ctx, data.common(), k=1).build([inner], rng).data


def time_quotient(ctx, data, warmup, reps):
    cfg = data.config
    n = 1 << data.degree_bits
    nq = n * cfg.max_quotient_degree_factor
    nch = cfg.num_challenges
    rng = np.random.default_rng(0x355)
    wb = api.PolynomialBatch.from_values(ctx, rand_field(rng, (cfg.num_wires, n)), cfg.rate_bits, cfg.cap_height)
    zb = api.PolynomialBatch.from_values(ctx, rand_field(rng, (nch * (1 + data.num_partial_products), n)), cfg.rate_bits, cfg.cap_height)
    betas, gammas, alphas, pi_hash = rand_field(rng, nch), rand_field(rng, nch), rand_field(rng, nch), rand_field(rng, 4)
    k_is = np.ascontiguousarray(data.k_is)
    out = np.empty((nch, nq), dtype=np.uint64)

    def launch():
        ctx.check(ctx.lib.gl355_quotient_values(ctx.h, C.byref(data.c_circuit), data.constants_sigmas.h, wb.h, zb.h, api._ptr(k_is),
                                                api._ptr(betas), api._ptr(gammas), api._ptr(alphas), api._ptr(pi_hash), api._ptr(out)))
    for _ in range(warmup):
        launch()
    ctx.sync()
    ctx.profile_enable(True)
    ctx.profile_read()
    ms = []
    for _ in range(reps):
        launch()
        cnt, total, _ = ctx.profile_read()["quotient_kernel"]
        assert cnt == 1
        ms.append(total)
    ctx.profile_enable(False)
    wb.close()
    zb.close()
    return nq, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["semaphore", "recursive"], default=None)
    args = ap.parse_args()
    ctx = gl.Context(0)
    for name, data in circuits(ctx, args.only):
        nq, ms = time_quotient(ctx, data, args.warmup, args.reps)
        print("quotient_kernel %-9s points=2^%d gates=%d  median %.4f ms  min %.4f  max %.4f  (%d launches)" % (
            name, nq.bit_length() - 1, data.c_circuit.num_gates, statistics.median(ms), min(ms), max(ms), len(ms)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
