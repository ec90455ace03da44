#!/usr/bin/env python3
"""What CosetInterpolationGate buys and costs the recursive proof: the circuit that verifies one Semaphore proof (degree 2^13, rate 3,
cap 4, 28 queries, 16 PoW bits, proven without blinding rows as in tools/fri_arity_bench.py) with the inner proof at
ConstantArityBits(1 | 3 | 4, 5), every case in the same run.
  python tools/coset_interpolation_bench.py [reps]
Per case: the inner proof's words, the recursive circuit's gate rows / degree / interpolation rows / tape entries, the wall time of
gl355_prove_sparse of it over `reps` proofs, and the quotient kernel's time per proof from gl355_profile_*.  The outer circuit has the
flagship's configuration (zero-knowledge, 28 queries, its own FRI at arity 2).  The case "(1, 5) + gate" is the (1, 5) circuit with
an unused CosetInterpolationGate{4, 6} in its gate set: the same rows through the kernel instances that know the gate (one more
filter factor in its selector group, the thirteenth evaluator compiled in, never active)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gl = importlib.import_module("stark-verifier_amd")
plonk = importlib.import_module("stark-verifier_amd.plonk")
sem = importlib.import_module("stark-verifier_amd.semaphore")
rec = importlib.import_module("stark-verifier_amd.recursion")
gad = importlib.import_module("stark-verifier_amd.gadgets")
_lib = importlib.import_module("stark-verifier_amd._lib")

LOG_N = 13


def rand_field(rng, shape):
    return rng.integers(0, plonk.P, size=shape, dtype=np.uint64)


def inner_proof(ctx, a):
    cfg = plonk.CircuitConfig(reduction_arity_bits=a, zero_knowledge=False)
    rng = np.random.default_rng(0x357)
    sks = rand_field(rng, (1 << 4, 4))
    keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
    aset = sem.AccessSet(ctx, keys)
    builder = plonk.CircuitBuilder(cfg)
    rows = aset.semaphore_circuit(builder)
    data = builder.build(ctx, rng, min_degree_bits=LOG_N)
    idx, vals, pi = aset.witness_rows(rows, sks[3], rand_field(rng, 4), 3)
    flat = plonk.prove_sparse(ctx, data, idx, vals, pi, 1, flat_only=True)
    data.verify(flat, pi)
    return data, flat, pi


def outer_circuit(ctx, data, flat, pi, flag, extra_gate=None):
    b = gad.GadgetBuilder(plonk.CircuitConfig(use_interpolation_gate=flag))
    proof = plonk.parse_proof(data, flat)
    proof["public_inputs"] = pi
    pis = rec.verify_proof(b, data.common(), proof, register_pis=False)
    rec.wrap_public_inputs(b, [pis])
    pi_vals = np.array(b.finalize_public_inputs(), dtype=np.uint64)
    if extra_gate is not None:
        b.cb.gate_type(*extra_gate)
    n_gate_rows = len(b.cb.rows)
    n_interp = sum(1 for gi, _ in b.cb.rows if b.cb.gate_types[gi][0] == _lib.GATE_COSET_INTERPOLATION)
    outer = b.cb.build(ctx, np.random.default_rng(0x358))
    idx, rows = b.sparse_witness()
    return outer, idx, rows, pi_vals, n_gate_rows, n_interp, len(b.tape)


def timed(ctx, outer, idx, rows, pi, reps):
    flat = plonk.prove_sparse(ctx, outer, idx, rows, pi, 1, flat_only=True)
    outer.verify(flat, pi)
    for k in range(3):
        plonk.prove_sparse(ctx, outer, idx, rows, pi, 2 + k, flat_only=True)
    ctx.sync()
    ctx.profile_enable(True)
    ctx.profile_read()
    t0 = time.perf_counter()
    for k in range(reps):
        plonk.prove_sparse(ctx, outer, idx, rows, pi, 10 + k, flat_only=True)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    cnt, q_ms, _ = prof.get("quotient_kernel", (0, 0.0, 0))
    return flat.size, ms, q_ms / max(cnt, 1)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ctx = gl.Context(0)
    print("recursive circuit over one Semaphore proof (degree 2^%d, 28 queries); outer: zero-knowledge, 28 queries, own arity 2; %d repetitions; ms" % (LOG_N, reps))
    print("%-14s %-12s %-10s %-7s %-12s %-9s %-12s %-12s %-10s" % ("inner FRI", "inner words", "gate rows", "degree", "interp rows", "tape", "outer words", "prove_sparse", "quotient"))
    base = None
    for name, a, extra in (("(1, 5)", 1, None), ("(1, 5) + gate", 1, (_lib.GATE_COSET_INTERPOLATION, plonk.coset_interpolation_param(4, 8))), ("(3, 5)", 3, None),
                           ("(4, 5)", 4, None)):
        data, flat, pi = inner_proof(ctx, a)
        t0 = time.perf_counter()
        outer, idx, rows, pi_vals, n_rows, n_interp, n_tape = outer_circuit(ctx, data, flat, pi, a > 1, extra)
        build_s = time.perf_counter() - t0
        words, ms, q_ms = timed(ctx, outer, idx, rows, pi_vals, reps)
        base = base or (ms, q_ms)
        print("%-14s %-12d %-10d 2^%-5d %-12d %-9d %-12d %-12.3f %-10.3f" % (name, flat.size, n_rows, outer.degree_bits, n_interp, n_tape, words, ms, q_ms))
        print("%-14s inner arities %s; %d gate kinds in %d selector groups; against (1, 5): prove %.3fx, quotient %.3fx; gadget pass + build %.1f s" % (
            "", data.fri_arity_bits, len(outer.gates), outer.num_selectors, ms / base[0], q_ms / base[1] if base[1] else 0.0, build_s))
    ctx.close()


if __name__ == "__main__":
    main()
