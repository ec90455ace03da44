"""Child process of test_gpu_halo2_verifier.py: GL355_HALO2_RUN_MAX is read when a tape is loaded, so every setting gets a process of its
own.  argv: an .npz of tapes (tape_<name>, k_<name>, inputs_<name>) -> one JSON line {name: [sha256 of the advice columns, first, count,
DeviceTape.launches()]}."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

try:                                                                 # as tests/conftest.py: torch's ROCm runtime first
    import torch
    torch.cuda.is_available() and torch.cuda.init()
except Exception:
    pass
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    gl = importlib.import_module("stark-verifier_amd")
    hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
    z = np.load(path, allow_pickle=False)
    ctx = gl.Context(0)
    out = {}
    try:
        for name in sorted(k[5:] for k in z.files if k.startswith("tape_")):
            inputs = z["inputs_" + name]
            tape = hg.DeviceTape(ctx, z["tape_" + name], int(z["k_" + name]), len(inputs))
            try:
                advice, (first, count) = tape.synthesize(inputs)
                launches = tape.launches()
            finally:
                tape.close()
            out[name] = [hashlib.sha256(np.ascontiguousarray(advice).tobytes()).hexdigest(), first, count, launches]
    finally:
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
