#!/usr/bin/env python3
"""Build the Semaphore circuit of a given tree height and the recursive verifier circuit over it (once per shape) and write them
as circuit artifacts: <dir>/semaphore.gl355, <dir>/recursive.gl355 (format: include/gl355.h).  Needs a GPU (the preprocessed
commitment enters the circuit digest).
    export_artifacts.py <dir> [log_members] [--reduction-arity-bits A | A,B,...]
--reduction-arity-bits builds both circuits at that FRI reduction strategy (an int = ConstantArityBits(A, 5), a comma list = Fixed)
and writes version-4 artifacts, which carry the arity table; the recursive circuit then contains CosetInterpolationGate rows.
Without the option both circuits fold by 2 and the artifacts are version 2, as before."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.cuda.init()
gl = importlib.import_module("stark-verifier_amd")
sem = importlib.import_module("stark-verifier_amd.semaphore")
rec = importlib.import_module("stark-verifier_amd.recursion")
plonk = importlib.import_module("stark-verifier_amd.plonk")
args = sys.argv[1:]
arity = None
if "--reduction-arity-bits" in args:
    at = args.index("--reduction-arity-bits")
    try:
        text = args[at + 1]
        arity = [int(a) for a in text.split(",")] if "," in text else int(text)
    except (IndexError, ValueError):
        sys.exit("usage: export_artifacts.py <dir> [log_members] [--reduction-arity-bits A | A,B,...]   (A, B, ...: 1 to 4)")
    del args[at:at + 2]
if not args:
    sys.exit("usage: export_artifacts.py <dir> [log_members] [--reduction-arity-bits A | A,B,...]")
out = args[0]
log_members = int(args[1]) if len(args) > 1 else 20
os.makedirs(out, exist_ok=True)
ctx = gl.Context(0)
rng = np.random.default_rng(1)
sks = rng.integers(0, 1 << 62, size=(1 << log_members, 4), dtype=np.uint64)
keys = ctx.hash_no_pad(np.concatenate([sks, np.zeros_like(sks)], axis=1))
aset = sem.AccessSet(ctx, keys)
wide = arity is not None
sem_cfg = plonk.CircuitConfig(reduction_arity_bits=arity) if wide else None
# the interpolation gate only where a layer folds by more than 2: `--reduction-arity-bits 1` writes the arity-2 circuits as version 4
folds_wide = wide and any(a > 1 for a in (arity if isinstance(arity, list) else [arity]))
rec_cfg = plonk.CircuitConfig(reduction_arity_bits=arity, use_interpolation_gate=folds_wide) if wide else None
data, rows = aset.build(rng, config=sem_cfg)
topic = rng.integers(0, 1 << 62, size=4, dtype=np.uint64)
idx, vals, pi = aset.witness_rows(rows, sks[0], topic, 0)
blob = data.export_blob(idx, wide_arity=wide)
blob.tofile(os.path.join(out, "semaphore.gl355"))
sig, _ = aset.make_signal_fast(sks[0], topic, 0, 1, flat_only=True)
rc = rec.RecursiveCircuit(ctx, data.common(), k=1, config=rec_cfg).build([(sig.proof, pi)], rng)
rblob = rc.data.export_blob(rc.row_idx, rc.tape, rc.pi_pos, rc.n_inputs, rc.tape_layout, wide_arity=wide)
rblob.tofile(os.path.join(out, "recursive.gl355"))
print("semaphore.gl355: %.1f MB (degree 2^%d), recursive.gl355: %.1f MB (degree 2^%d, %d tape entries)" % (
    blob.nbytes / 1e6, data.degree_bits, rblob.nbytes / 1e6, rc.data.degree_bits, rc.tape.shape[0]))
if wide:
    print("version-%d artifacts, FRI arity bits %r and %r" % (int(blob[1]), data.fri_arity_bits, rc.data.fri_arity_bits))
