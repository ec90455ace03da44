"""Lagrange bases from public powers of tau (gl355_kzg_lagrange_from_powers: the inverse G1 FFT of halo2's ParamsKZG::downsize /
g_to_lagrange) on cuda:0 at k = argv[1:] (default 20 22 23): g from gl355_kzg_setup stays on the device, one warm-up call, then
--reps timed calls, each synchronised.  One JSON line per k with the best and median seconds, the butterflies and scalar multiplications
of the transform, and the Fq product count the DESIGN 4.8 ceiling is priced by (~2.9k products per 4-bit signed-window multiplication)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAU = 0x1234567890ABCDEF1234567890ABCDEF0123456789ABCDEF
PRODUCTS_PER_MUL = 2900          # 4-bit signed windows: 256 doublings x 7 + 64 additions x 16 + the table
PRODUCTS_PER_SEC = 1.5e11        # ~1060 issue clk per 8 x 32-bit product per wave, 1024 SIMDs at 2.4 GHz


def run(gl, ctx, k, reps):
    import torch
    h2 = importlib.import_module("stark-verifier_amd.halo2")
    n = 1 << k
    g = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    tau = h2.to_limbs([TAU % h2.R])[0]
    ctx.check(ctx.lib.gl355_kzg_setup(ctx.h, tau.ctypes.data, k, g.data_ptr(), None))
    ctx.sync()
    ctx.check(ctx.lib.gl355_kzg_lagrange_from_powers(ctx.h, g.data_ptr(), n, k, out.data_ptr()))       # warm-up
    ctx.sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.check(ctx.lib.gl355_kzg_lagrange_from_powers(ctx.h, g.data_ptr(), n, k, out.data_ptr()))
        ctx.sync()
        times.append(time.perf_counter() - t0)
    butterflies = (n // 2) * k
    trivial = n - 1                                  # butterflies with j = 0: 2^(k-s) per stage s
    muls = butterflies - trivial + n                 # + the 1/n scaling
    products = muls * PRODUCTS_PER_MUL
    del g, out
    torch.cuda.empty_cache()
    return {"k": k, "best_s": round(min(times), 3), "median_s": round(statistics.median(times), 3), "reps": reps,
            "butterflies": butterflies, "scalar_muls": muls, "fq_products": products,
            "ceiling_s": round(products / PRODUCTS_PER_SEC, 3), "ceiling_ratio": round(min(times) / (products / PRODUCTS_PER_SEC), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", nargs="*", type=int, default=[20, 22, 23])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    gl = importlib.import_module("stark-verifier_amd")
    ctx = gl.Context(0)
    for k in a.k:
        print(json.dumps(run(gl, ctx, k, max(3, a.reps))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
