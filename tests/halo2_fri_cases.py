"""Real proofs for FriVerifierCircuit (test_halo2_fri_circuit.py, test_gpu_halo2_fri.py): a depth-1 Semaphore signal proved on the CPU
(cpu_semaphore + CpuProver) under Bn254PoseidonHash with cap height 1, two query rounds, 3 proof-of-work bits and a final polynomial of
two coefficients, once with zero_knowledge on (salted leaves: unsalted_eval matters; 2^8 rows, seven FRI layers) and once off (2^3 rows, two
layers).  get_challenges is restated here over pv.Transcript, because pv.verify returns only some of the challenges.  Everything is built
once per process, and every recording is checked to fit k = 17."""
import functools
import importlib

import numpy as np

import cpu_semaphore as csem
import halo2_synth_cases as cs
import plonk_verifier as pv
from oracle_lib import Oracle, rand_field

hg, h2, P, K = cs.hg, cs.h2, cs.P, cs.K
vc = importlib.import_module("stark-verifier_amd.halo2_verifier_circuit")
plonk = importlib.import_module("stark-verifier_amd.plonk")

CONFIG = dict(hasher=1, cap_height=1, num_query_rounds=2, proof_of_work_bits=3, final_poly_bits=1)
SEEDS = {True: 0xF2A, False: 0xF2B}


def challenges(orc, cd, proof, pi_hash):
    """get_challenges (plonk_verifier_chip.rs:55-154) -> fri_alpha, fri_betas, pow_response and the RAW squeezed indices"""
    op = {k: [pv.ext(v) for v in vals] for k, vals in proof["openings"].items()}
    fri = proof["opening_proof"]
    nch = cd["num_challenges"]
    tr = pv.Transcript(orc, cd["hasher"])
    tr.observe(cd["circuit_digest"])
    tr.observe(pi_hash)
    tr.observe(proof["wires_cap"])
    tr.squeeze(nch), tr.squeeze(nch)
    tr.observe(proof["plonk_zs_partial_products_cap"])
    tr.squeeze(nch)
    tr.observe(proof["quotient_polys_cap"])
    zeta = tuple(tr.squeeze(2))
    for name in ("constants", "plonk_sigmas", "wires", "plonk_zs", "partial_products", "quotient_polys", "plonk_zs_next"):
        for v in op[name]:
            tr.observe(list(v))
    fri_alpha = tuple(tr.squeeze(2))
    fri_betas = []
    for cap in fri["commit_phase_merkle_caps"]:
        tr.observe(cap)
        fri_betas.append(tuple(tr.squeeze(2)))
    tr.observe(fri["final_poly"])
    tr.observe([fri["pow_witness"]])
    pow_response = tr.squeeze(1)[0]
    indices = tr.squeeze(cd["num_query_rounds"])
    ints = lambda t: tuple(int(v) for v in t)      # noqa: E731
    return dict(zeta=ints(zeta), fri_alpha=ints(fri_alpha), fri_betas=[ints(b) for b in fri_betas], pow_response=int(pow_response), indices=[int(i) for i in indices])


class Case:
    """one proof: common data, the flat proof, the hash of its public inputs, the circuit, its input vector and the recorder"""

    def __init__(self, zk):
        self.orc = orc = Oracle()
        self.zk = zk
        case = csem.build_case(orc, 1, SEEDS[zk], config=plonk.CircuitConfig(zero_knowledge=zk, **CONFIG))
        self.data = data = case["data"]
        self.cd = cd = data.common()
        idx, vals, pi = csem.witness(orc, case, 1, rand_field(case["rng"], 4))
        self.flat = case["cpu"].prove_sparse(idx, vals, pi, 41)
        self.pi = pi
        self.pi_hash = np.array([int(v) for v in orc.hash_no_pad(np.asarray(pi, dtype=np.uint64))], dtype=np.uint64)
        assert cd["hasher"] == 1 and cd["cap_height"] == 1 and cd["num_query_rounds"] == 2 and cd["pow_bits"] >= 3 and bool(cd["hiding"]) == zk
        assert len(cd["arity_bits"]) >= 2 and (1 << cd["degree_bits"]) >> len(cd["arity_bits"]) >= 2
        self.verify(self.flat)                                       # pv.verify accepts the proof
        self.circuit = vc.FriVerifierCircuit(cd)
        self.inputs = self.circuit.inputs(self.flat, self.pi_hash)
        self.rec = self.circuit.record(self.inputs)
        assert self.rec.k == K, "the recording does not fit k = 17"
        self.challenges = challenges(orc, cd, self.parse(self.flat), self.pi_hash)

    def parse(self, flat):
        proof = plonk.parse_proof(self.data, flat)
        proof["public_inputs"] = self.pi
        return proof

    def verify(self, flat):
        return pv.verify(self.orc, self.cd, self.parse(flat))

    def mutations(self):
        """-> {name: input vector}: one word changed each.  The changed proof-of-work witness is chosen so that the new response has a
        non-zero top bit (asserted here), so fri_verify_proof_of_work must fail whatever else does"""
        c = self.circuit
        out = {}
        for name, word in (("quotient_opening", c.openings["quotient_polys"][1][0]), ("final_poly", c.final_poly[1][1]), ("pi_hash", c.pi_hash[2])):
            bad = self.inputs.copy()
            bad[word] = (int(bad[word]) + 1) % P
            out[name] = bad
        for delta in range(1, 64):
            bad = self.inputs.copy()
            bad[c.pow_witness] = (int(bad[c.pow_witness]) + delta) % P
            response = challenges(self.orc, self.cd, self.parse(bad[:c.proof_words]), self.pi_hash)["pow_response"]
            if response >> 63:
                break
        assert response >> 63, "no nearby proof-of-work witness gives a response with its top bit set"
        out["pow_witness"] = bad
        return out


@functools.lru_cache(maxsize=None)
def case(zk):
    return Case(zk)


@functools.lru_cache(maxsize=None)
def mutations(zk):
    return case(zk).mutations()


# ---- GoldilocksExtensionChip on edge operands -----------------------------------------------------------------------------------------------
EDGE = [(0, 0), (1, 0), (P - 1, P - 1), (0, 5), (0x123456789ABCDEF, 0), (3, P - 2)]


def ext_operands(rec):
    g = hg.GoldilocksChip(rec)
    cells = [g.assign_value(hg.Input(i)) for i in range(len(rec.inputs))]
    return [[cells[2 * i], cells[2 * i + 1]] for i in range(len(cells) // 2)]


@functools.lru_cache(maxsize=None)
def extension_case():
    """every GoldilocksExtensionChip method on operands that include 0, 1, p - 1, (0, y1) and (y0, 0)
    -> (recorder, [(method, operand values, result cells)])"""
    rec = hg.Recorder(K, [v for e in EDGE for v in e])
    ge = hg.GoldilocksExtensionChip(rec)
    ge.goldilocks_chip.load_table()
    xs = ext_operands(rec)
    val = lambda e: (e[0].value, e[1].value)      # noqa: E731
    out = []
    for i, a in enumerate(xs):
        b, c = xs[(i + 1) % len(xs)], xs[(i + 2) % len(xs)]
        out.append(("mul_add", (val(a), val(b), val(c)), ge.mul_add_extension(a, b, c)))
        out.append(("add", (val(a), val(b)), ge.add_extension(a, b)))
        out.append(("sub", (val(a), val(b)), ge.sub_extension(a, b)))
        out.append(("mul", (val(a), val(b)), ge.mul_extension(a, b)))
        out.append(("mul_sub", (val(a), val(b), val(c)), ge.mul_sub_extension(a, b, c)))
        out.append(("square", (val(a),), ge.square_extension(a)))
        out.append(("scalar_mul", (val(a), P - 1), ge.scalar_mul(a, P - 1)))
        out.append(("arithmetic", (3, P - 1, val(a), val(b), val(c)), ge.arithmetic_extension(3, P - 1, a, b, c)))
        out.append(("mul_with_const", (5, val(a), val(b)), ge.mul_extension_with_const(5, a, b)))
        out.append(("select", (val(a), val(b), val(c)), ge.select(a, b, c)))
        out.append(("exp2", (val(a), 3), ge.exp_power_of_2_extension(a, 3)))
        out.append(("convert", (a[0].value,), ge.convert_to_extension(a[0])))
        if val(b) != (0, 0):
            out.append(("div", (val(a), val(b)), ge.div_extension(a, b)))
            out.append(("div_add", (val(a), val(b), val(c)), ge.div_add_extension(a, b, c)))
    a, b = xs[2], xs[5]
    for power in range(4):
        out.append(("exp", (val(a), power), ge.exp(a, power)))
    out.append(("shift", (val(a), 3, val(b)), ge.shift(a, 3, b)))
    out.append(("mul_many", tuple(val(x) for x in xs[1:4]), ge.mul_many_extension(xs[1:4])))
    for count in (0, 1, 3):
        terms = xs[2:2 + count]
        out.append(("reduce", (val(a), [val(t) for t in terms]), ge.reduce_extension(a, terms)))
        out.append(("reduce_base_terms", (val(a), [t[1].value for t in terms]), ge.reduce_base_field_terms_extension(a, [t[1] for t in terms])))
        out.append(("reduce_base", (b[1].value, [val(t) for t in terms]), ge.reduce_extension_field_terms_base(b[1], terms)))
    out.append(("zero", (), ge.zero_extension()))
    out.append(("one", (), ge.one_extension()))
    out.append(("two", (), ge.two_extension()))
    out.append(("constant", ((P - 1, 9),), ge.constant_extension((P - 1, 9))))
    ge.assert_equal_extension(ge.sub_extension(a, a), ge.zero_extension())
    ge.assert_one_extension(ge.div_extension(b, b))
    return rec, out


@functools.lru_cache(maxsize=None)
def zero_divisor_case():
    """div_extension by (0, 0) between good rows: y_inv is (0, 0), the assert_one of y y_inv fails, the rows are written all the same"""
    rec = hg.Recorder(K, [5, 6, 0, 0])
    ge = hg.GoldilocksExtensionChip(rec)
    ge.goldilocks_chip.load_table()
    x, y = ext_operands(rec)
    q = ge.div_extension(x, y)
    ge.add_extension(q, x)
    return rec, q


def synth_cases():
    """name -> (tape, k, input vector, recorder or None): what the host and the device interpreters are compared on"""
    out = {}
    for name, rec in (("extension", extension_case()[0]), ("zero_divisor", zero_divisor_case()[0])):
        out[name] = (rec.tape(), rec.k, np.array(rec.inputs, dtype=np.uint64), rec)
    for zk in (True, False):
        c = case(zk)
        tag = "zk" if zk else "plain"
        out["fri_" + tag] = (c.rec.tape(), c.rec.k, c.inputs, c.rec)
        for name, bad in mutations(zk).items():
            out["fri_%s_%s" % (tag, name)] = (c.rec.tape(), c.rec.k, bad, None)
    return out


# ---- the mock model's gate and lookup rules, vectorised over the rows ------------------------------------------------------------------------
def _size(e, memo):
    if id(e) not in memo:
        memo[id(e)] = 1 + sum(_size(x, memo) for x in (e.a, e.b) if isinstance(x, h2.Expression))
    return memo[id(e)]


def evaluate_rows(e, rows, columns, cs_, n, sizes):
    """halo2_mock_model.evaluate on all of `rows` at once (object arrays of Python integers), for rows whose queries stay below the usable
    rows (no poison).  A product evaluates its smaller factor first and the other one only where that is non-zero: the model's
    `unpoisoned zero times anything is zero`, which is what spares the Poseidon gates on the rows whose selector is off"""
    op = e.op
    if op == "const":
        return np.full(len(rows), e.a % h2.R, dtype=object)
    if op == "query":
        col, rot = cs_.queries[e.a][e.b]
        return columns[e.a](col, (rows + rot) % n)
    if op == "neg":
        return (-evaluate_rows(e.a, rows, columns, cs_, n, sizes)) % h2.R
    if op == "scale":
        return evaluate_rows(e.a, rows, columns, cs_, n, sizes) * e.b % h2.R
    if op == "add":
        return (evaluate_rows(e.a, rows, columns, cs_, n, sizes) + evaluate_rows(e.b, rows, columns, cs_, n, sizes)) % h2.R
    assert op == "mul"
    first, second = (e.a, e.b) if _size(e.a, sizes) <= _size(e.b, sizes) else (e.b, e.a)
    x = evaluate_rows(first, rows, columns, cs_, n, sizes)
    out = np.zeros(len(rows), dtype=object)
    nz = np.flatnonzero(x != 0)
    if len(nz):
        out[nz] = x[nz] * evaluate_rows(second, rows[nz], columns, cs_, n, sizes) % h2.R
    return out


def mock_failures_fast(rec, advice):
    """test_halo2_goldilocks.mock_failures for a circuit of tens of thousands of rows: the same rows (every row with a selector on, and their
    readers), the same rules and the same records, with the gates and the lookup inputs evaluated by evaluate_rows instead of row by row
    (test_halo2_fri_circuit.py holds the two against each other on a satisfied and on a failing witness)"""
    from halo2_mock_model import GATE, LOOKUP, MockModel
    lay = rec.layout()
    cs_, n = lay.cs, lay.n
    fixed, mapping = lay.fixed_array(), lay.mapping_array()
    model = MockModel(cs_, rec.k, None, None)
    rows = np.array([r for r in model.readers(cs.selector_rows(rec)) if r < model.usable], dtype=np.int64)
    assert rows.min() + min(model.rotations) >= 0 and rows.max() + max(model.rotations) < model.usable, "a query would be poisoned"
    ints = lambda a: (a[:, 0].astype(object) + (a[:, 1].astype(object) << 64) + (a[:, 2].astype(object) << 128) + (a[:, 3].astype(object) << 192)) % h2.R      # noqa: E731
    inst = np.zeros(n, dtype=object)
    inst[:len(rec.instance)] = [v % h2.R for v in rec.instance]
    columns = {h2.ADVICE: lambda col, r: ints(advice[col][r]), h2.FIXED: lambda col, r: ints(fixed[col][r]), h2.INSTANCE: lambda col, r: inst[r]}
    sizes, out, ordinal = {}, [], 0
    for _, polys in cs_.gates:
        for poly in polys:
            v = evaluate_rows(poly, rows, columns, cs_, n, sizes)
            out += [(GATE, ordinal, int(r), 0) for r in rows[np.flatnonzero(v != 0)]]
            ordinal += 1
    for li, (_, ins, _) in enumerate(cs_.lookups):                   # every table is the 16-bit range table (RANGE_TABLE there)
        assert len(ins) == 1
        v = evaluate_rows(ins[0], rows, columns, cs_, n, sizes)
        out += [(LOOKUP, li, int(r), 0) for r in rows[np.flatnonzero(v >= (1 << 16))]]
    return sorted(out + cs.copy_failures(cs_, mapping, advice, fixed, rec.instance))
