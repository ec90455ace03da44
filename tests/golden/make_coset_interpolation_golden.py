"""Mint tests/golden/coset_interpolation_proof.json on a GPU: one proof of the gate-zoo circuit of tests/coset_interpolation_cases.py
(fri_arity_cases.small_circuit + one CosetInterpolationGate row of each size), for the CPU suite
(tests/test_verify_interpolation_host.py), which has no prover.

    python tests/golden/make_coset_interpolation_golden.py [output path]

The fixture has the layout of fri_arity_proof.json: the flat proof (base64 of its little-endian words), its SHA-256, the public
inputs, the constants_sigmas cap, the circuit digest and the configuration; the test rebuilds the circuit tables on the host."""
import base64
import hashlib
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main(out_path):
    import coset_interpolation_cases as cc
    gl = importlib.import_module("stark-verifier_amd")
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    case = cc.CASE
    ctx = gl.Context(0)
    b, pi, _ = cc.zoo_circuit(plonk.CircuitConfig(**case["config"]), case["circuit_seed"])
    data = b.cb.build(ctx, np.random.default_rng(0), min_degree_bits=case["min_degree_bits"])
    idx, rows = b.sparse_witness()
    flat = plonk.prove_sparse(ctx, data, idx, rows, pi, case["proof_seed"], flat_only=True)
    data.verify(flat, pi)
    raw = np.ascontiguousarray(flat, dtype="<u8").tobytes()
    fixture = dict(case, degree_bits=data.degree_bits, fri_arity_bits=list(data.fri_arity_bits), proof_words=int(flat.size),
                   gates=[[int(t), int(p)] for t, p in data.gates],
                   sha256=hashlib.sha256(raw).hexdigest(), proof_b64=base64.b64encode(raw).decode(),
                   public_inputs=[int(v) for v in pi], constants_sigmas_cap=[[int(v) for v in h] for h in data.constants_sigmas_cap],
                   circuit_digest=[int(v) for v in data.circuit_digest])
    with open(out_path, "w") as f:
        json.dump(fixture, f, indent=1)
        f.write("\n")
    ctx.close()
    print("wrote %s: degree 2^%d, arities %s, %d words" % (out_path, data.degree_bits, data.fri_arity_bits, flat.size))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "coset_interpolation_proof.json"))
