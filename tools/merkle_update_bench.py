#!/usr/bin/env python3
"""What changing k members of a resident access set costs against rebuilding it: trees of 2^20 and 2^22 leaves of 4 words, cap height 0, and
k in {1, 64, 4096, n/64, n/8, n} uniformly random different leaves (and n/32, n/16, to place the crossover).
  python tools/merkle_update_bench.py [--logs 20,22] [--reps 9] [--out profiles/merkle_update.txt]
Three ways to the new cap, timed alternately in one process on a host clock around calls that end in a stream sync (warm-up calls first, then the
median of `reps` rounds; a round runs each way once):
  dirty    gl355_merkle_tree_update + gl355_merkle_tree_cap with GL355_OPT_MERKLE_UPDATE_FULL_LOG = 0: the host plans the dirty paths, the leaf
           kernel and the level / climb kernels walk them (k = n is a whole rebuild under every setting);
  full     the same two calls with the option at 31: the leaf kernel, then every level of the tree;
  rebuild  what there was before the resident tree: gl355_merkle_build_h from the host leaves, every digest downloaded.
The crossover between the first two is where the option's default belongs; it is printed under each table as a shift of n.
Before the timed rounds the three ways' caps are compared."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gl = importlib.import_module("stark-verifier_amd")

OPT_MERKLE_UPDATE_FULL_LOG = 8


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bench_shape(log_n, reps, out):
    n = 1 << log_n
    rng = np.random.default_rng(0xACC + log_n)
    leaves = rng.integers(0, gl.P, (n, 4), dtype=np.uint64)
    cx = gl.Context(0)
    lib = cx.lib
    tree = gl.DeviceMerkleTree(cx, leaves, 0)
    digests, cap, cap_t = np.empty((2 * (n - 1), 4), np.uint64), np.empty((1, 4), np.uint64), np.empty((1, 4), np.uint64)
    out("2^%d leaves of 4 words, cap height 0 (%d levels); ms, median of %d (min .. max)" % (log_n, log_n, reps))
    out("%10s %24s %24s %24s" % ("k", "dirty", "full", "rebuild"))
    crossover = None
    current = leaves.copy()                # the host leaf array a user of the rebuild keeps; every k's update stays applied on both sides
    for k in (1, 64, 4096, n // 64, n // 32, n // 16, n // 8, n):
        idx = rng.choice(n, size=k, replace=False).astype(np.uint64)
        rows = rng.integers(0, gl.P, (k, 4), dtype=np.uint64)

        def update(full_log):
            cx.set_option(OPT_MERKLE_UPDATE_FULL_LOG, full_log)
            cx.check(lib.gl355_merkle_tree_update(tree.h, ptr(idx), k, ptr(rows)))
            cx.check(lib.gl355_merkle_tree_cap(tree.h, ptr(cap_t)))

        def rebuild():
            current[idx] = rows
            cx.check(lib.gl355_merkle_build_h(cx.h, 0, ptr(current), n, 4, 0, ptr(digests), ptr(cap)))

        ways = (("dirty", lambda: update(0)), ("full", lambda: update(31)), ("rebuild", rebuild))
        caps = []
        for _, fn in ways:                 # warm-up, and the same root three times
            fn()
            fn()
            caps.append((cap_t if fn is not rebuild else cap).copy())
        assert np.array_equal(caps[0], caps[1]) and np.array_equal(caps[0], caps[2]), "the three ways disagree"
        times = {name: [] for name, _ in ways}
        for _ in range(reps):
            for name, fn in ways:
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        med = {name: statistics.median(v) for name, v in times.items()}
        out("%10d " % k + " ".join("%8.3f (%6.3f ..%7.3f)" % (med[name], min(times[name]), max(times[name])) for name, _ in ways))
        if crossover is None and k < n and med["full"] <= med["dirty"]:
            crossover = k
    out("full <= dirty from k = %s on" % ("n >> %d" % (log_n - int(crossover).bit_length() + 1) if crossover else "n (never below it)"))
    out("")
    tree.close()
    cx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,22")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    for log_n in (int(x) for x in args.logs.split(",")):
        bench_shape(log_n, args.reps, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
