"""TEST INFRASTRUCTURE: the list of bad inputs the native Halo2 verifier (gl355_plonk_verify) and the restated one (tests/halo2_verifier.py)
must agree on -- ordinary malformed data that a verifier rejects with a verdict: every commitment position replaced by another valid curve
point, every evaluation incremented, an instance value changed, a byte dropped / appended, a scalar set to r, a point moved off the curve."""
import pymodel_bn254_curve as pm

R, Q = pm.R, pm.Q


def proof_layout(cs):
    """(points before the evaluations, evaluations): the proof is 64-byte points, then 32-byte scalars, then SHPLONK's two points"""
    cl = cs.chunk_len()
    n_sets = (len(cs.permutation) + cl - 1) // cl if cs.permutation else 0
    n_points = cs.num_advice + 3 * len(cs.lookups) + n_sets + 1 + (cs.degree() - 1)
    n_evals = len(cs.queries[0]) + len(cs.queries[1]) + 1 + len(cs.permutation) + (3 * n_sets - 1 if n_sets else 0) + 5 * len(cs.lookups)
    return n_points, n_evals


def point_bytes(p):
    return (b"\x00" * 64) if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")


def mutations(cs, instances, proof, every=1):
    """[(name, instances, proof)]; every > 1 keeps each `every`-th position of the two long lists (always the first and the last)"""
    n_points, n_evals = proof_layout(cs)
    assert len(proof) == 64 * (n_points + 2) + 32 * n_evals
    ev0 = 64 * n_points
    offs = [64 * i for i in range(n_points)] + [ev0 + 32 * n_evals, ev0 + 32 * n_evals + 64]
    keep = lambda i, m: i % every == 0 or i == m - 1         # noqa: E731
    out = []
    for i, o in enumerate(offs):
        if keep(i, len(offs)):
            out.append(("point %d replaced" % i, instances, proof[:o] + point_bytes(pm.mul(pm.G, 1000 + i)) + proof[o + 64:]))
    for j in range(n_evals):
        if keep(j, n_evals):
            o = ev0 + 32 * j
            v = (int.from_bytes(proof[o:o + 32], "big") + 1) % R
            out.append(("evaluation %d incremented" % j, instances, proof[:o] + v.to_bytes(32, "big") + proof[o + 32:]))
    for c, col in enumerate(instances):
        if col:
            changed = [list(x) for x in instances]
            changed[c][0] = (changed[c][0] + 1) % R
            out.append(("instance value changed", changed, proof))
            break
    out.append(("last byte dropped", instances, proof[:-1]))
    out.append(("byte appended", instances, proof + b"\x00"))
    out.append(("scalar set to r", instances, proof[:ev0] + R.to_bytes(32, "big") + proof[ev0 + 32:]))
    y = (int.from_bytes(proof[32:64], "big") + 1) % Q
    out.append(("point moved off the curve", instances, proof[:32] + y.to_bytes(32, "big") + proof[64:]))
    x = int.from_bytes(proof[:32], "big") + Q
    if x < 1 << 256:
        out.append(("point coordinate not canonical", instances, x.to_bytes(32, "big") + proof[32:]))
    return out
