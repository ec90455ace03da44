"""One call per shape through gl355_ntt / gl355_coset_ntt / gl355_lde / gl355_lde_bitrev, for a kernel trace of the Goldilocks NTT routes.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ntt_route_sweep.py run [path/to/libgl355.so]
    python tools/ntt_route_sweep.py reduce DIR/.../*_kernel_trace.csv > reduced.txt

`run` goes through the rows of docs/history/ntt_shapes.md and one shape per kernel instance of csrc/ntt_route.h, with a fresh context per value of
GL355_OPT_NTT_SINGLE_PASS_MAX_LOG; a one-word field_batch call separates the shapes in the trace.  `reduce` prints, per shape, the sequence of
(kernel, grid, workgroup, LDS bytes, scratch bytes, registers) -- table builds included, template parameters that an instance list no longer has
normalised away -- so that the traces of two libraries can be compared with diff."""
import csv
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (call, log_n, ...): fft / ifft / coset_fft / coset_ifft take (log_n, extra stride); lde takes (log_n, rate_bits); lde_many the same with
# 65536 device-resident columns (the batch no longer fits a grid dimension)
SHAPES_12 = (
    [("fft", 0, 0)] + [(d, n, 0) for n in range(1, 12) for d in ("fft", "ifft")] +
    [(d, n, 0) for n in (12, 14) for d in ("fft", "coset_fft", "ifft", "coset_ifft")] + [(d, 13, 0) for d in ("fft", "ifft", "coset_ifft")] +
    [("fft", 15, 0), ("fft", 15, 8), ("coset_fft", 15, 0), ("ifft", 15, 0), ("coset_ifft", 15, 0), ("fft", 16, 0), ("fft", 18, 0), ("fft", 20, 0)] +
    [("ifft", n, 0) for n in (16, 17, 18, 19, 20, 21, 22, 24)] + [("coset_fft", n, 0) for n in (16, 17, 18, 19, 20, 24)] +
    [("fft", 21, 0), ("fft", 21, 8), ("fft", 22, 0), ("fft", 22, 8), ("fft", 23, 0), ("fft", 24, 0)] +
    [("lde", n, r) for n, r in ((5, 3), (12, 3), (13, 3), (13, 0), (14, 1), (14, 0), (15, 3), (16, 3), (17, 3), (17, 0), (18, 3), (18, 4), (19, 2),
                                (19, 3), (20, 1), (20, 2), (21, 2), (22, 1))] +
    [("lde_many", n, 1) for n in (13, 14, 15)])
SHAPES = {12: SHAPES_12, 13: [("lde", 13, 3), ("lde", 14, 1)], 14: [("lde", 13, 3), ("lde", 14, 1)]}


def run(lib_path):
    import numpy as np
    import torch                                      # before the library: torch has to initialise the HIP runtime of the process (_lib.load)
    torch.cuda.init()
    sys.path.insert(0, ROOT)
    gl = importlib.import_module("stark-verifier_amd")
    if lib_path:
        gl._lib.LIB_PATH = os.path.abspath(lib_path)
    one = np.ones(1, dtype=np.uint64)
    for opt, shapes in SHAPES.items():
        ctx = gl.Context(0)
        ctx.set_option(4, opt)
        for call, log_n, arg in shapes:
            ctx.field_batch(0, one, one)              # the separator
            n = 1 << log_n
            batch = 2 if log_n < 21 else 1
            if call == "lde":
                ctx.lde(np.ones((batch, n), dtype=np.uint64), arg, bitrev=True)
                ctx.lde(np.ones((batch, n), dtype=np.uint64), arg)
            elif call == "lde_many":
                import ctypes as C
                import torch
                cd = torch.ones((65536, n), dtype=torch.int64, device="cuda")
                out = torch.empty((65536, n << arg), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                ctx.check(ctx.lib.gl355_lde_bitrev(ctx.h, C.c_void_p(cd.data_ptr()), log_n, arg, 7, 65536, C.c_void_p(out.data_ptr())))
                ctx.sync()
                del cd, out
                torch.cuda.empty_cache()
            else:
                x = np.ones((batch, n + arg), dtype=np.uint64)
                ctx.fft(x, inverse=call.endswith("ifft"), shift=7 if call.startswith("coset") else None, stride=n + arg if arg else None,
                        log_n=log_n if arg else None)
            print("done", opt, call, log_n, arg, flush=True)
        ctx.close()


def normalise(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    name = re.sub(r"(ntt_rows_kernel<\d+, \d+, \w+), false, \d+>", r"\1>", name)      # FAST and WPE of the row kernel
    name = re.sub(r"(ntt_cols_kernel<\d+, \w+), false>", r"\1>", name)                # FAST of the column kernel
    return name


def reduce(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    keep = [c for c in rows[0] if re.search(r"Grid_Size|Workgroup_Size|LDS|Scratch|VGPR|SGPR|Private_Segment|Group_Segment", c, re.I)]
    labels = [(opt,) + s for opt, shapes in SHAPES.items() for s in shapes]
    seg = -1
    for r in rows:
        name = normalise(r["Kernel_Name"])
        if "field_batch" in name:
            seg += 1
            print("# shape %d: option %d, %s" % ((seg,) + (labels[seg][0], " ".join(map(str, labels[seg][1:]))) if seg < len(labels) else (seg, -1, "?")))
            continue
        if seg >= 0:
            print(name, " ".join("%s=%s" % (c, r[c]) for c in keep))
    assert seg + 1 == len(labels), "%d separators for %d shapes" % (seg + 1, len(labels))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) == 3 and sys.argv[1] == "reduce":
        reduce(sys.argv[2])
    else:
        sys.exit(__doc__)
