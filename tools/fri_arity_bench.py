#!/usr/bin/env python3
"""What a FRI reduction arity above 2 buys a lone unit: the unit shape (degree 13, rate 3, cap 4, 28 queries, 16 PoW bits) proven at
ConstantArityBits(1 | 2 | 3 | 4, 5), every arity in the same run.
  python tools/fri_arity_bench.py [reps]
Per arity: the proof's words and its layer words per query; from gl355_profile_* over `reps` calls of gl355_fri_prove on a random
degree-13 polynomial: layer leaves, layer trees (leaf hash + levels), folds, layer openings, and the wall time of the whole tail
(transcript and proof of work included); and the latency of a whole lone proof (gl355_prove_sparse of the Semaphore circuit padded to
2^13 rows, without blinding rows: their number depends on the arity and would change the degree)."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gl = importlib.import_module("stark-verifier_amd")
plonk = importlib.import_module("stark-verifier_amd.plonk")
sem = importlib.import_module("stark-verifier_amd.semaphore")

LOG_N, RATE_BITS, CAP, QUERIES, POW_BITS = 13, 3, 4, 28, 16
TREE = ("hash_leaves_kernel", "merkle_level_kernel", "merkle_level_lanes_kernel", "merkle_top_kernel")


def rand_field(rng, shape):
    return rng.integers(0, plonk.P, size=shape, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def tail(ctx, arities, reps):
    """-> (wall ms per call, {profile name: ms per call}) of gl355_fri_prove"""
    shape = plonk.fri_layer_shape(LOG_N + RATE_BITS, CAP, arities)
    coeffs = rand_field(np.random.default_rng(1), 2 << LOG_N)
    arity = np.array(arities, dtype=np.uint32)
    caps = np.zeros(len(arities) * (4 << CAP), dtype=np.uint64)
    final = np.zeros(2 * ((1 << LOG_N) >> sum(arities)), dtype=np.uint64)
    w, idx = C.c_uint64(), np.zeros(QUERIES, dtype=np.uint64)
    evals = np.zeros((QUERIES, sum(wd for wd, _ in shape)), dtype=np.uint64)
    sibs = np.zeros((QUERIES, sum(d for _, d in shape), 4), dtype=np.uint64)

    def run(k):
        ch = plonk.Challenger()
        ch.observe(np.arange(1, 12, dtype=np.uint64) + np.uint64(k))
        ctx.check(ctx.lib.gl355_fri_prove(ctx.h, ptr(coeffs), LOG_N, RATE_BITS, CAP, ptr(arity), len(arities), POW_BITS, QUERIES, C.byref(ch.c),
                                          ptr(caps), ptr(final), C.byref(w), ptr(idx), ptr(evals), ptr(sibs)))
    for k in range(3):
        run(k)
    ctx.sync()
    ctx.profile_enable(True)
    ctx.profile_read()
    t0 = time.perf_counter()
    for k in range(reps):
        run(100 + k)
    ctx.sync()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    prof = {k: v[1] / reps for k, v in ctx.profile_read().items() if not k.startswith("host:")}
    ctx.profile_enable(False)
    return wall, prof


def lone_unit(ctx, a, reps):
    """-> (proof words, layer words per query, ms per lone proof)"""
    cfg = plonk.CircuitConfig(reduction_arity_bits=a, zero_knowledge=False)
    rng = np.random.default_rng(0x357)
    sks = rand_field(rng, (1 << 4, 4))
    keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
    aset = sem.AccessSet(ctx, keys)
    builder = plonk.CircuitBuilder(cfg)
    rows = aset.semaphore_circuit(builder)
    data = builder.build(ctx, rng, min_degree_bits=LOG_N)
    assert data.degree_bits == LOG_N
    idx, vals, pi = aset.witness_rows(rows, sks[3], rand_field(rng, 4), 3)
    flat = plonk.prove_sparse(ctx, data, idx, vals, pi, 1, flat_only=True)
    data.verify(flat, pi)
    for k in range(3):
        plonk.prove_sparse(ctx, data, idx, vals, pi, 2 + k, flat_only=True)
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(reps):
        plonk.prove_sparse(ctx, data, idx, vals, pi, 10 + k, flat_only=True)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    layer_words = sum(w + 4 * d for w, d in plonk.fri_layer_shape(LOG_N + RATE_BITS, CAP, data.fri_arity_bits))
    return data.fri_arity_bits, flat.size, layer_words, ms


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ctx = gl.Context(0)
    print("unit shape: degree 2^%d, rate_bits %d, cap_height %d, %d queries, %d PoW bits; %d repetitions; times in ms" % (LOG_N, RATE_BITS, CAP, QUERIES, POW_BITS, reps))
    print("%-6s %-7s %-11s %-11s %-9s %-9s %-8s %-8s %-9s %-9s" % ("arity", "layers", "proof words", "layer w/q", "leaves", "trees", "fold", "open", "FRI tail", "lone unit"))
    base = None
    for a in (1, 2, 3, 4):
        arities, words, layer_words, unit_ms = lone_unit(ctx, a, reps)
        wall, prof = tail(ctx, arities, reps)
        trees = sum(prof.get(k, 0.0) for k in TREE)
        row = (prof.get("fri_layer_leaves", 0.0), trees, prof.get("fri_fold", 0.0), prof.get("open_batch", 0.0), wall, unit_ms)
        base = base or row
        print("2^%-4d %-7d %-11d %-11d %-9.3f %-9.3f %-8.3f %-8.3f %-9.3f %-9.3f" % ((a, len(arities), words, layer_words) + row))
        print("%-38s %-9s %-9s %-8s %-8s %-9s %-9s" % (("  against arity 2^1:",) + tuple("%.2fx" % (r / b) if b else "-" for r, b in zip(row, base))))
        print("  leaf hash of the layer trees alone: %.3f ms" % prof.get("hash_leaves_kernel", 0.0))
    ctx.close()


if __name__ == "__main__":
    main()
