"""FRI with reduction arities A = 2^a, a = 1..4, restated in Python (plonky2 fri_committed_trees, fri_prover_query_round,
fri_verifier_query_round, compute_evaluation; the reference states the verifier side for a = 1 at chip/fri_chip.rs:168-226,275-316).

Extension arithmetic is pymodel's big-integer one; transforms, trees, proof of work and the sponge are oracle_lib's primitives.  With
s_l = a_0 + .. + a_l:
  fold        out[k] = sum_{j<A} beta^j c[A k + j]; afterwards shift <- shift^A
  layer tree  the values on shift * <omega> in bit-reversed order, leaf i = the A values [A i, A i + A) as 2A words, hash_or_noop
  query       layer l opens leaf x_index >> s_l, path of lde_bits - s_l - cap_height digests
  step        within = idx & (A - 1), coset = idx >> a; evals[within] is the running value; the leaf's values, reordered by
              reverse_index_bits, lie on x g^(A - rev(within)) g^j with g = 7^((p-1)/A); the next value is their interpolant at beta;
              then x <- x^A, idx <- coset
verify() is tests/plonk_verifier.py's verifier with this step in place of its arity-2 one."""
import numpy as np

import plonk_verifier as pv
import pymodel as pm
from oracle_lib import Bn254Oracle, P

E0, E1 = pv.E0, pv.E1
add, sub, mul, base, ext = pv.add, pv.sub, pv.mul, pv.base, pv.ext


def layer_shape(lde_bits, cap_height, arities):
    """per layer (words of an opened leaf, digests of its path): the layout rule of the flat proof"""
    out, s = [], 0
    for a in arities:
        s += a
        out.append((2 << a, lde_bits - s - cap_height))
    return out


def proof_words(cd, n_public_inputs=None):
    """u64 words of the flat proof of common data cd (include/gl355.h), from the layout rule alone"""
    nch, n_cap, lde_bits = cd["num_challenges"], 1 << cd["cap_height"], cd["degree_bits"] + cd["rate_bits"]
    widths = [cd["num_selectors"] + cd["num_constants"] + cd["num_routed_wires"], cd["num_wires"],
              nch * (1 + cd["num_partial_products"]), nch * cd["quotient_degree_factor"]]
    per_query = 1 + sum(w + (4 if (cd["hiding"] and o > 0) else 0) + 4 * (lde_bits - cd["cap_height"]) for o, w in enumerate(widths))
    per_query += sum(w + 4 * d for w, d in layer_shape(lde_bits, cd["cap_height"], cd["arity_bits"]))
    return (8 + 3 * 4 * n_cap + 2 * (sum(widths) + nch) + len(cd["arity_bits"]) * 4 * n_cap
            + 2 * ((1 << cd["degree_bits"]) >> sum(cd["arity_bits"])) + 1 + per_query * cd["num_query_rounds"])


def fold(coeffs, a, beta):
    """flat ext coefficients [2n] -> [2 (n >> a)], from the definition"""
    A, b = 1 << a, ext(beta)
    c = [ext(v) for v in np.asarray(coeffs, dtype=np.uint64).reshape(-1, 2)]
    out = []
    for k in range(len(c) // A):
        acc = E0
        for j in reversed(range(A)):
            acc = add(mul(acc, b), c[A * k + j])
        out.append(acc)
    return np.array(out, dtype=np.uint64).reshape(-1)


def layer_leaves(orc, values, a):
    """natural-order ext values [2N] -> leaves [N >> a][2 << a]"""
    v = np.asarray(values, dtype=np.uint64).reshape(-1, 2)
    return np.ascontiguousarray(orc.reverse_index_bits(v).reshape(v.shape[0] >> a, 2 << a))


def merkle_build(orc, leaves, cap_height, hasher=0):
    if leaves.shape[0] == 1 << cap_height:      # a tree that is all cap: every leaf digest is a cap entry
        hash_no_pad = Bn254Oracle(orc).hash_no_pad if hasher else orc.hash_no_pad
        cap = np.array([lv[:4] if lv.size <= 4 else hash_no_pad(lv) for lv in leaves], dtype=np.uint64).reshape(-1, 4)
        return np.zeros((0, 4), np.uint64), cap
    return Bn254Oracle(orc).merkle_build(leaves, cap_height) if hasher else orc.merkle_build(leaves, cap_height)


def fri_tail(orc, ch, coeffs, rate_bits, cap_height, arities, pow_bits, n_queries, hasher=0):
    """the prover's FRI tail on a host Challenger `ch` (stark-verifier_amd.plonk.Challenger, already started)
    -> caps [L][n_cap][4], final_poly, pow_witness, query indices, per layer (leaves, digests)"""
    c, shift = np.asarray(coeffs, dtype=np.uint64).copy(), 7
    N = (c.size // 2) << rate_bits
    caps, layers = [], []
    for a in arities:
        leaves = layer_leaves(orc, orc.lde_ext(c, rate_bits, shift), a)
        dig, cap = merkle_build(orc, leaves, cap_height, hasher)
        caps.append(cap)
        layers.append((leaves, dig))
        ch.observe(cap)
        c = fold(c, a, ch.get_extension_challenge())
        shift = pow(shift, 1 << a, P)
    ch.observe(c)
    st, pos = ch.pow_state()
    w = orc.pow_grind(st, pos, pow_bits) if pow_bits else 0
    ch.observe(np.array([w], dtype=np.uint64))
    resp = int(ch.squeeze(1)[0])
    assert pow_bits == 0 or resp >> (64 - pow_bits) == 0
    idx = ch.squeeze(n_queries) & np.uint64(N - 1)
    return np.array(caps, dtype=np.uint64).reshape(len(arities), 1 << cap_height, 4), c, w, idx, layers


def interpolate(points, values, x):
    """value at x (ext) of the polynomial of degree < len(points) through (points[j], values[j]); points in the base field"""
    acc = E0
    for j, (pj, vj) in enumerate(zip(points, values)):
        num, den = vj, 1
        for k, pk in enumerate(points):
            if k != j:
                num = mul(num, sub(x, base(pk)))
                den = den * (pj - pk) % P
        acc = add(acc, mul(num, base(pow(den, P - 2, P))))
    return acc


def step(evals, idx, x, a, beta):
    """one verifier step: evals = the A ext values of the opened leaf -> (evals[within], next value, coset index, x^A)"""
    A = 1 << a
    within, coset = idx & (A - 1), idx >> a
    g = pm.root_of_unity(a)
    start = x * pow(g, A - pm.bitrev(within, a), P) % P
    points = [start * pow(g, j, P) % P for j in range(A)]
    values = [evals[pm.bitrev(j, a)] for j in range(A)]
    return evals[within], interpolate(points, values, ext(beta)), coset, pow(x, A, P)


def verify(orc, cd, proof):
    """plonk_verifier.verify for any arities: the same transcript, vanishing identity and batch combination; only the per-layer
    loop differs.  Raises plonk_verifier.VerifyError naming the failed check."""
    nch = cd["num_challenges"]
    arities = [int(a) for a in cd["arity_bits"]]
    fri = proof["opening_proof"]
    lde_bits = cd["degree_bits"] + cd["rate_bits"]
    shape = layer_shape(lde_bits, cd["cap_height"], arities)
    if (len(fri["query_round_proofs"]) != cd["num_query_rounds"] or len(fri["commit_phase_merkle_caps"]) != len(arities)
            or len(fri["final_poly"]) != (1 << cd["degree_bits"]) >> sum(arities)
            or any(len(r["steps"]) != len(arities) or any(len(e) != w or len(s) != d for (e, s), (w, d) in zip(r["steps"], shape))
                   for r in fri["query_round_proofs"])):
        raise pv.VerifyError("proof shape")
    op = {k: [ext(v) for v in vals] for k, vals in proof["openings"].items()}
    pi_hash = [int(v) for v in orc.hash_no_pad(np.asarray(proof["public_inputs"], dtype=np.uint64))]
    hasher = cd.get("hasher", 0)
    tr = pv.Transcript(orc, hasher)
    tr.observe(cd["circuit_digest"])
    tr.observe(pi_hash)
    tr.observe(proof["wires_cap"])
    betas, gammas = tr.squeeze(nch), tr.squeeze(nch)
    tr.observe(proof["plonk_zs_partial_products_cap"])
    alphas = tr.squeeze(nch)
    tr.observe(proof["quotient_polys_cap"])
    zeta = tuple(tr.squeeze(2))
    zeta_batch = op["constants"] + op["plonk_sigmas"] + op["wires"] + op["plonk_zs"] + op["partial_products"] + op["quotient_polys"]
    next_batch = op["plonk_zs_next"]
    for v in zeta_batch + next_batch:
        tr.observe(list(v))
    fri_alpha = tuple(tr.squeeze(2))
    fri_betas = []
    for cap in fri["commit_phase_merkle_caps"]:
        tr.observe(cap)
        fri_betas.append(tuple(tr.squeeze(2)))
    tr.observe(fri["final_poly"])
    tr.observe([fri["pow_witness"]])
    pow_response = tr.squeeze(1)[0]
    query_indices = tr.squeeze(cd["num_query_rounds"])
    n = 1 << cd["degree_bits"]
    zeta_pow_n = pv.ext_pow(zeta, n)
    van = pv.eval_vanishing_poly(cd, zeta, zeta_pow_n, op, pi_hash, betas, gammas, alphas)
    z_h = sub(zeta_pow_n, E1)
    qdf = cd["quotient_degree_factor"]
    for i in range(nch):
        if mul(z_h, pv.reduce_with_powers(op["quotient_polys"][i * qdf:(i + 1) * qdf], zeta_pow_n)) != van[i]:
            raise pv.VerifyError("quotient identity fails for challenge %d" % i)
    if cd["pow_bits"] and pow_response >> (64 - cd["pow_bits"]):
        raise pv.VerifyError("proof of work")
    g = pm.root_of_unity(cd["degree_bits"])
    zeta_next = (zeta[0] * g % P, zeta[1] * g % P)
    widths = [cd["num_selectors"] + cd["num_constants"] + cd["num_routed_wires"], cd["num_wires"],
              nch * (1 + cd["num_partial_products"]), nch * qdf]
    all_polys = [(o, i) for o in range(4) for i in range(widths[o])]
    batches = [(zeta, all_polys, zeta_batch), (zeta_next, [(2, i) for i in range(nch)], next_batch)]
    reduced_openings = [pv.reduce_with_powers(vals, fri_alpha) for _, _, vals in batches]
    caps = [cd["constants_sigmas_cap"], proof["wires_cap"], proof["plonk_zs_partial_products_cap"], proof["quotient_polys_cap"]]
    N = 1 << lde_bits
    omega = pm.root_of_unity(lde_bits)
    for q, rnd in zip(query_indices, fri["query_round_proofs"]):
        x_index = q % N
        if rnd["index"] != x_index:
            raise pv.VerifyError("query index mismatch")
        for o, (leaf, sib) in enumerate(rnd["initial_trees"]):
            want = widths[o] + (4 if (cd["hiding"] and o > 0) else 0)
            if len(leaf) != want or not orc.merkle_verify(leaf, x_index, sib, caps[o], cd["cap_height"], hasher):
                raise pv.VerifyError("initial tree %d opening" % o)
        x = 7 * pow(omega, pm.bitrev(x_index, lde_bits), P) % P
        total = E0
        for (point, polys, _), red in zip(batches, reduced_openings):
            evals = [base(rnd["initial_trees"][o][0][i]) for o, i in polys]
            num = sub(pv.reduce_with_powers(evals, fri_alpha), red)
            total = add(mul(total, pv.ext_pow(fri_alpha, len(evals))), mul(num, pm.ext_inv(sub(base(x), point))))
        prev, idx = total, x_index
        for l, a in enumerate(arities):
            evals_flat, sib = rnd["steps"][l]
            evals = [ext(evals_flat[2 * j:2 * j + 2]) for j in range(1 << a)]
            opened, nxt, coset, x = step(evals, idx, x, a, fri_betas[l])
            if opened != prev:
                raise pv.VerifyError("fold consistency at layer %d" % l)
            if not orc.merkle_verify(np.asarray(evals_flat, dtype=np.uint64), coset, sib, fri["commit_phase_merkle_caps"][l], cd["cap_height"], hasher):
                raise pv.VerifyError("layer %d Merkle opening" % l)
            prev, idx = nxt, coset
        if pv.reduce_with_powers([ext(c) for c in fri["final_poly"]], base(x)) != prev:
            raise pv.VerifyError("final polynomial")
    return dict(query_indices=query_indices, fri_betas=fri_betas)
