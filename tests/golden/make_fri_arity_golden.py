"""Mint tests/golden/fri_arity_proof.json on a GPU: one proof of the small gate-zoo circuit of tests/fri_arity_cases.py at the FRI
reduction arities below, for the CPU suite (tests/test_verify_arity_host.py), which has no prover for arities above 2.

    python tests/golden/make_fri_arity_golden.py [output path]

The fixture holds the flat proof (base64 of its little-endian words), its SHA-256, the public inputs, the constants_sigmas cap, the
circuit digest and the configuration; the test rebuilds the circuit tables on the host from the same configuration."""
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

CASE = dict(config=dict(reduction_arity_bits=[2, 3], zero_knowledge=False, cap_height=1, num_query_rounds=3),
            min_degree_bits=6, circuit_seed=0x7C0, proof_seed=0x7C1)


def main(out_path):
    import fri_arity_cases as fc
    gl = importlib.import_module("stark-verifier_amd")
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    ctx = gl.Context(0)
    b, pi = fc.small_circuit(plonk.CircuitConfig(**CASE["config"]), CASE["circuit_seed"])
    data = b.cb.build(ctx, np.random.default_rng(0), min_degree_bits=CASE["min_degree_bits"])
    idx, rows = b.sparse_witness()
    flat = plonk.prove_sparse(ctx, data, idx, rows, pi, CASE["proof_seed"], flat_only=True)
    data.verify(flat, pi)
    raw = np.ascontiguousarray(flat, dtype="<u8").tobytes()
    fixture = dict(CASE, degree_bits=data.degree_bits, fri_arity_bits=list(data.fri_arity_bits), proof_words=int(flat.size),
                   sha256=hashlib.sha256(raw).hexdigest(), proof_b64=base64.b64encode(raw).decode(),
                   public_inputs=[int(v) for v in pi], constants_sigmas_cap=[[int(v) for v in h] for h in data.constants_sigmas_cap],
                   circuit_digest=[int(v) for v in data.circuit_digest])
    with open(out_path, "w") as f:
        json.dump(fixture, f, indent=1)
        f.write("\n")
    ctx.close()
    print("wrote %s: degree 2^%d, arities %s, %d words" % (out_path, data.degree_bits, data.fri_arity_bits, flat.size))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fri_arity_proof.json"))
