"""plonky2's CosetInterpolationGate { subgroup_bits b, degree d } (gates/coset_interpolation.rs, D = 2) restated over big integers
(TEST INFRASTRUCTURE), in the style of plonk_verifier.eval_gate: layout, constraints over extension values, the witness generator,
a wrapper that teaches plonk_verifier.eval_gate the gate, and a row checker for a GadgetBuilder's witness.

No plonky2 source is at hand: the definition is the one include/gl355.h states, and what the tests pin is that the prover's kernel,
both verifiers, the in-circuit evaluator and the witness generators agree with this model and, through fri_arity_model.interpolate,
with the interpolant the gate is for.  The barycentric weights are formed here from their definition 1 / prod_{j != i}(x_i - x_j);
the product uses the closed form x_i / N."""
import plonk_verifier as pv
import pymodel as pm

P = pm.P
COSET_INTERPOLATION = 12
E0, E1 = pv.E0, pv.E1
add, sub, mul, base = pv.add, pv.sub, pv.mul, pv.base


def with_max_degree(bits, max_degree):
    """-> (degree, number of intermediate (eval, prod) pairs)"""
    n = 1 << bits
    n_int = (n - 2) // (max_degree - 1)
    return (n - 2) // (n_int + 1) + 2, n_int


def param(bits, degree):
    return bits | degree << 8


def layout(bits, degree):
    n = 1 << bits
    n_int = (n - 2) // (degree - 1)
    start_int = 1 + 2 * n + 4
    return dict(bits=bits, degree=degree, n=n, n_int=n_int, shift=0, values=[1 + 2 * i for i in range(n)], point=1 + 2 * n,
                value=1 + 2 * n + 2, start_int=start_int, int_eval=[start_int + 2 * i for i in range(n_int)],
                int_prod=[start_int + 2 * (n_int + i) for i in range(n_int)], shifted=start_int + 4 * n_int,
                num_routed=start_int, num_wires=start_int + 4 * n_int + 2, num_constraints=2 * (2 + 2 * n_int))


def domain(bits):
    g = pm.root_of_unity(bits)
    return [pow(g, i, P) for i in range(1 << bits)]


def weights_by_product(bits):
    xs = domain(bits)
    out = []
    for i, xi in enumerate(xs):
        d = 1
        for j, xj in enumerate(xs):
            if j != i:
                d = d * (xi - xj) % P
        out.append(pow(d, P - 2, P))
    return out


def weights_on_subgroup(bits):
    n_inv = pow(1 << bits, P - 2, P)
    return [x * n_inv % P for x in domain(bits)]


def chunks(lay):
    """the point ranges of the fold: [0, d), then per intermediate i [1 + (d - 1)(i + 1), min(that + d - 1, N))"""
    d, n = lay["degree"], lay["n"]
    out = [(0, d)]
    for i in range(lay["n_int"]):
        lo = 1 + (d - 1) * (i + 1)
        out.append((lo, min(lo + d - 1, n)))
    return out


def _amul(a, b):
    return (add(mul(a[0], b[0]), mul(base(7), mul(a[1], b[1]))), add(mul(a[0], b[1]), mul(a[1], b[0])))


def _asub(a, b):
    return (sub(a[0], b[0]), sub(a[1], b[1]))


def _aadd(a, b):
    return (add(a[0], b[0]), add(a[1], b[1]))


def _ascal(c, a):
    return (mul(c, a[0]), mul(c, a[1]))


def eval_gate(gate, consts, w, pi_hash):
    """the constraints of gate (COSET_INTERPOLATION, b | d << 8) at extension wire values w: wire pairs are algebra elements, `shift`
    an extension scalar"""
    t, p = gate
    assert t == COSET_INTERPOLATION
    lay = layout(p & 0xFF, (p >> 8) & 0xFF)
    xs, ws = domain(lay["bits"]), weights_by_product(lay["bits"])

    def alg(j):
        return (w[j], w[j + 1])
    x = alg(lay["shifted"])
    out = list(_asub(alg(lay["point"]), _ascal(w[lay["shift"]], x)))

    def fold(ev, prod, lo, hi):
        for i in range(lo, hi):
            xm = (sub(x[0], base(xs[i])), x[1])
            ev, prod = _aadd(_amul(ev, xm), _amul(_ascal(base(ws[i]), alg(lay["values"][i])), prod)), _amul(prod, xm)
        return ev, prod
    ranges = chunks(lay)
    ev, prod = fold((E0, E0), (E1, E0), *ranges[0])
    for i in range(lay["n_int"]):
        ie, ip = alg(lay["int_eval"][i]), alg(lay["int_prod"][i])
        out += list(_asub(ie, ev)) + list(_asub(ip, prod))
        ev, prod = fold(ie, ip, *ranges[1 + i])
    out += list(_asub(alg(lay["value"]), ev))
    assert len(out) == lay["num_constraints"]
    return out


def generate(bits, degree, shift, values, point):
    """the generator on a witness row (every wire a base-field number, an extension value = two wires): shift int, values N pairs,
    point a pair -> the row's wires; None when the shift is zero (a failed witness, not a division)"""
    lay = layout(bits, degree)
    if shift % P == 0:
        return None
    w = [0] * lay["num_wires"]
    w[0] = shift % P
    for i, v in enumerate(values):
        w[1 + 2 * i], w[2 + 2 * i] = v[0] % P, v[1] % P
    w[lay["point"]], w[lay["point"] + 1] = point[0] % P, point[1] % P
    x = mul(pv.ext(point), base(pow(shift, P - 2, P)))
    w[lay["shifted"]], w[lay["shifted"] + 1] = x
    xs, ws = domain(bits), weights_by_product(bits)
    ev, prod = E0, E1
    ranges = chunks(lay)
    for k, (lo, hi) in enumerate(ranges):
        if k:
            w[lay["int_eval"][k - 1]], w[lay["int_eval"][k - 1] + 1] = ev
            w[lay["int_prod"][k - 1]], w[lay["int_prod"][k - 1] + 1] = prod
        for i in range(lo, hi):
            xm = sub(x, base(xs[i]))
            ev, prod = add(mul(ev, xm), mul(mul(pv.ext(values[i]), base(ws[i])), prod)), mul(prod, xm)
    w[lay["value"]], w[lay["value"] + 1] = ev
    return w


def install(monkeypatch):
    """plonk_verifier.eval_gate learns the gate: pv.eval_vanishing_poly, pv.verify and fri_arity_model.verify then evaluate circuits
    that contain it"""
    original = pv.eval_gate

    def patched(gate, consts, w, pi_hash):
        if gate[0] == COSET_INTERPOLATION:
            return eval_gate(gate, consts, w, pi_hash)
        return original(gate, consts, w, pi_hash)
    monkeypatch.setattr(pv, "eval_gate", patched)
    return patched


def check_rows(b, pi_hash=None, rows=None):
    """every row of GadgetBuilder b's witness (or of `rows`: row -> {col: value}) satisfies its gate; -> the number of rows of each
    gate type.  pi_hash: the four words a PublicInputGate row must carry (rows of that gate are skipped without it)."""
    seen = {}
    nw = b.nw
    for r, cols in (rows if rows is not None else b.rows).items():
        gate = b.cb.gate_types[b.cb.rows[r][0]]
        consts = [base(c) for c in b.cb.rows[r][1]] + [E0, E0]
        if gate[0] == pv.PUBLIC_INPUT and pi_hash is None:
            continue
        w = [base(cols.get(c, 0)) for c in range(nw)]
        evaluator = eval_gate if gate[0] == COSET_INTERPOLATION else pv.eval_gate
        bad = [k for k, c in enumerate(evaluator(gate, consts, w, pi_hash)) if c != E0]
        assert not bad, "row %d (gate %r): constraints %r do not vanish" % (r, gate, bad[:4])
        seen[gate[0]] = seen.get(gate[0], 0) + 1
    return seen
