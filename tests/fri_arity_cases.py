"""A small gate-zoo circuit for the FRI-arity tests (test helper): base and extension arithmetic, a Poseidon sponge, bit
decomposition, random access, reductions and the MDS gate -- every gate kind the gadget builder emits, in a few dozen rows -- plus
the mutations of a flat proof's FRI layers that the C and the Python verifier must reject at the same named check."""
import importlib

import numpy as np

import fri_arity_model as fm
import plonk_verifier as pv
from oracle_lib import rand_field


def small_circuit(config, seed):
    """-> (GadgetBuilder with the witness of inputs drawn from `seed`, public-input values); the layout does not depend on the seed"""
    gad = importlib.import_module("stark-verifier_amd.gadgets")
    rng = np.random.default_rng(seed)
    b = gad.GadgetBuilder(config)
    inputs = rand_field(rng, 8 + 16 + 24)
    xs = b.add_virtual_targets([int(v) for v in inputs[:8]])
    s = b.add(b.mul(xs[0], xs[1]), xs[2])
    e1, e2 = (xs[0], xs[1]), (xs[2], xs[3])
    q = b.ext_div(b.ext_mul(e1, e2), e2)
    b.connect_ext(q, e1)
    h = b.hash_n_to_hash_no_pad(xs + xs[:3])
    bits = b.split_le_64(xs[5])
    items = b.add_virtual_targets([int(v) for v in inputs[8:24]])
    picked = b.random_access(b.le_sum(bits[:4]), items)
    alpha = (xs[6], xs[7])
    coeffs = b.add_virtual_targets([int(v) for v in inputs[24:48]])
    red = b.reduce_with_powers_base(coeffs, alpha)
    ecoeffs = [(coeffs[2 * i], coeffs[2 * i + 1]) for i in range(12)]
    red2 = b.reduce_with_powers_ext(ecoeffs, alpha)
    mds = b.mds_ext(ecoeffs)
    b.register_public_inputs([s, h[0], picked, red[1], red2[0], mds[3][1]])
    pi_vals = b.finalize_public_inputs()
    return b, np.array(pi_vals, dtype=np.uint64)


def config_of(plonk, **kw):
    kw.setdefault("num_query_rounds", 3)
    return plonk.CircuitConfig(**kw)


def fri_layer_positions(cd, flat, query=0):
    """word positions inside flat proof `flat` of common data cd: per FRI layer of query `query` (start of the opened leaf, its words),
    and the position of the final polynomial"""
    nch, n_cap, lde_bits = cd["num_challenges"], 1 << cd["cap_height"], cd["degree_bits"] + cd["rate_bits"]
    widths = [cd["num_selectors"] + cd["num_constants"] + cd["num_routed_wires"], cd["num_wires"],
              nch * (1 + cd["num_partial_products"]), nch * cd["quotient_degree_factor"]]
    shape = fm.layer_shape(lde_bits, cd["cap_height"], cd["arity_bits"])
    final_pos = 8 + 3 * 4 * n_cap + 2 * (sum(widths) + nch) + len(shape) * 4 * n_cap
    pos = query_start(cd)
    per_initial = 1 + sum(w + (4 if (cd["hiding"] and o > 0) else 0) + 4 * (lde_bits - cd["cap_height"]) for o, w in enumerate(widths))
    pos += query * (per_initial + sum(w + 4 * d for w, d in shape)) + per_initial
    out = []
    for w, d in shape:
        out.append((pos, w))
        pos += w + 4 * d
    return out, final_pos


def mutations(cd, flat):
    """(name, mutated flat proof, the check both verifiers must name), on the first layer of the first query that folds by more than 2"""
    flat = np.asarray(flat, dtype=np.uint64)
    layers, final_pos = fri_layer_positions(cd, flat)
    l = next(i for i, a in enumerate(cd["arity_bits"]) if a > 1)
    a, s_before = cd["arity_bits"][l], sum(cd["arity_bits"][:l])
    pos, words = layers[l]
    x_index = int(flat[query_start(cd)])
    within = (x_index >> s_before) & ((1 << a) - 1)
    other = (within + 1) % (1 << a)

    def flip(p):
        f = flat.copy()
        f[p] ^= np.uint64(1)
        return f
    swapped = flat.copy()
    swapped[pos + 2 * within:pos + 2 * within + 2] = flat[pos + 2 * other:pos + 2 * other + 2]
    swapped[pos + 2 * other:pos + 2 * other + 2] = flat[pos + 2 * within:pos + 2 * within + 2]
    yield "an eval that is not the queried one", flip(pos + 2 * other + 1), "merkle %d" % l
    yield "the queried eval", flip(pos + 2 * within), "fold %d" % l
    yield "two evals of one leaf swapped", swapped, "fold %d" % l
    # the final polynomial is absorbed before the proof-of-work witness: changing it changes the response, which then misses its
    # leading zeros (all but 2^-pow_bits of the time), before any query is looked at
    yield "a final coefficient", flip(final_pos + 1), "pow" if cd["pow_bits"] else "final"


def query_start(cd):
    """word position of the first query (its x_index)"""
    nch, n_cap = cd["num_challenges"], 1 << cd["cap_height"]
    widths = [cd["num_selectors"] + cd["num_constants"] + cd["num_routed_wires"], cd["num_wires"],
              nch * (1 + cd["num_partial_products"]), nch * cd["quotient_degree_factor"]]
    return (8 + 3 * 4 * n_cap + 2 * (sum(widths) + nch) + len(cd["arity_bits"]) * 4 * n_cap
            + 2 * ((1 << cd["degree_bits"]) >> sum(cd["arity_bits"])) + 1)


C_CHECKS = {"merkle": "FRI layer opening does not verify", "fold": "FRI fold consistency", "final": "final polynomial", "pow": "proof of work",
            "shape": "proof length does not match the circuit"}


def verdicts(orc, gl, plonk, data, flat, pi):
    """-> (the check gl355_verify names, the check the model verifier names): None = accepted; gl355_verify's as `kind`, the model's
    as `kind` or `kind layer`"""
    try:
        data.verify(flat, pi)
        c_check = None
    except gl.Gl355Error as e:
        assert e.code == -7, e
        msg = str(e).split(": ", 1)[1]
        c_check = next((k for k, v in C_CHECKS.items() if v == msg), msg)
    try:
        proof = plonk.parse_proof(data, flat)
    except (ValueError, AssertionError):      # another layer count, or words left over
        return c_check, "shape"
    proof["public_inputs"] = pi
    try:
        fm.verify(orc, data.common(), proof)
        m_check = None
    except pv.VerifyError as e:
        msg = str(e)
        if msg == "proof shape":
            m_check = "shape"
        elif msg == "final polynomial":
            m_check = "final"
        elif msg == "proof of work":
            m_check = "pow"
        elif msg.startswith("fold consistency at layer "):
            m_check = "fold %s" % msg.rsplit(" ", 1)[1]
        elif msg.startswith("layer ") and msg.endswith("Merkle opening"):
            m_check = "merkle %s" % msg.split(" ")[1]
        else:
            m_check = msg
    return c_check, m_check
