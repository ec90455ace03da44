"""Cases for part 3 of the Halo2 verifier circuit (test_halo2_gate_constrainers.py, test_halo2_public_inputs_hasher.py,
test_halo2_plonky2_verifier_circuit.py, test_gpu_halo2_verifier.py): the 12 gate constrainers on small parameters, the public-inputs hasher,
Plonky2VerifierCircuit on the two real proofs of halo2_fri_cases and on a third whose circuit uses all 12 gate kinds, their one-word
mutations, and synthetic tapes aimed at the device's run form.  Everything is built once per process; every recording fits k = 17."""
import functools
import importlib

import numpy as np

import halo2_fri_cases as fc
import plonk_verifier as pv
from oracle_lib import CpuProver, Oracle, rand_field

hg, h2, P, K, vc, plonk = fc.hg, fc.h2, fc.P, fc.K, fc.vc, fc.plonk
hp = importlib.import_module("stark-verifier_amd.halo2_plonk_chips")
ps = importlib.import_module("stark-verifier_amd.poseidon_spec")
gad = importlib.import_module("stark-verifier_amd.gadgets")

# the smallest parameter that makes every loop of a constrainer run at least twice
GATES = {"noop": (pv.NOOP, 0), "constant": (pv.CONSTANT, 2), "public_input": (pv.PUBLIC_INPUT, 0), "base_sum": (pv.BASE_SUM, 2),
         "poseidon": (pv.POSEIDON, 0), "arithmetic": (pv.ARITHMETIC, 2), "arithmetic_extension": (pv.ARITHMETIC_EXT, 2),
         "multiplication_extension": (pv.MUL_EXT, 2), "poseidon_mds": (pv.POSEIDON_MDS, 0), "random_access": (pv.RANDOM_ACCESS, 2 | 2 << 8 | 1 << 16),
         "reducing": (pv.REDUCING, 2), "reducing_extension": (pv.REDUCING_EXT, 2)}
N_WIRES, N_CONSTANTS = 135, 2


def val(e):
    return (e[0].value, e[1].value)


def accepted(rec):
    """what every recording must pass: status clean, host replay equal to the recorder's eager columns, the mock model clean on every row used"""
    advice, status = hg.synthesize_host(rec.tape(), rec.k, np.array(rec.inputs, dtype=np.uint64))
    assert rec.k == K and status == rec.status() == (hg.NO_FAILURE, 0)
    assert np.array_equal(advice, rec.advice())
    assert fc.mock_failures_fast(rec, advice) == []


def gate_vectors():
    """-> [words]: a random vector and one made of halo2_fri_cases.EDGE, each N_CONSTANTS constants, N_WIRES wires (extension elements) and
    the four words of a public-inputs hash"""
    rng = np.random.default_rng(0x6A7E)
    n = 2 * (N_CONSTANTS + N_WIRES) + 4
    edge = [v for i in range(n // 2 + 1) for v in fc.EDGE[i % len(fc.EDGE)]][:n - 4] + [0, P - 1, 1, 0x123456789ABCDEF]
    return [[int(v) for v in rand_field(rng, n)], edge]


def assign_gate_inputs(rec):
    """-> (constants, wires, hash) as cells, with their values"""
    g = hg.GoldilocksChip(rec)
    g.load_table()
    cells = [g.assign_value(hg.Input(i)) for i in range(len(rec.inputs))]
    pairs = [[cells[2 * i], cells[2 * i + 1]] for i in range(N_CONSTANTS + N_WIRES)]
    return pairs[:N_CONSTANTS], pairs[N_CONSTANTS:], cells[-4:]


@functools.lru_cache(maxsize=None)
def gate_case(name, vector):
    """eval_unfiltered_constraint of one gate alone -> (recorder, constraint cells, the values plonk_verifier.eval_gate gives)"""
    rec = hg.Recorder(K, gate_vectors()[vector])
    consts, wires, pi_hash = assign_gate_inputs(rec)
    cells = hp.GateConstrainer(rec, GATES[name]).eval_unfiltered_constraint(consts, wires, pi_hash)
    want = pv.eval_gate(GATES[name], [val(c) for c in consts], [val(w) for w in wires], [c.value for c in pi_hash])
    return rec, cells, want


def filter_common(num_selectors):
    """a selector layout over five gates: one group of four when num_selectors > 1 (and public_input in a group of its own), all in one group otherwise"""
    gates = [GATES["noop"], GATES["constant"], GATES["arithmetic"], GATES["base_sum"], GATES["public_input"]]
    if num_selectors > 1:
        groups, selector_indices = [(0, 4), (4, 5)], [0, 0, 0, 0, 1]
    else:
        groups, selector_indices = [(0, 5)], [0] * 5
    return dict(gates=gates, groups=groups, selector_indices=selector_indices, num_selectors=num_selectors, num_gate_constraints=4)


def filtered_want(cd, consts, wires, pi_hash):
    """the filter loop of plonk_verifier.eval_vanishing_poly (plonk_verifier.py:229-238), term for term"""
    allc = [pv.E0] * cd["num_gate_constraints"]
    for gi, gate in enumerate(cd["gates"]):
        sel = cd["selector_indices"][gi]
        lo, hi = cd["groups"][sel]
        filt = pv.E1
        for k in [k for k in range(lo, hi) if k != gi] + ([pv.UNUSED_SELECTOR] if cd["num_selectors"] > 1 else []):
            filt = pv.mul(filt, pv.sub(pv.base(k), consts[sel]))
        for k, c in enumerate(pv.eval_gate(gate, consts[cd["num_selectors"]:], wires, pi_hash)):
            allc[k] = pv.add(allc[k], pv.mul(filt, c))
    return allc


@functools.lru_cache(maxsize=None)
def filtered_case(num_selectors, vector):
    """eval_gate_constraints over filter_common -> (recorder, the combined constraint cells, want, the common data, (consts, wires, hash) values)"""
    cd = filter_common(num_selectors)
    words = list(gate_vectors()[vector])
    if vector == 1:                                                  # a selector polynomial opens to anything at zeta: once to a gate's own index
        words[0:2] = [2, 0]
    rec = hg.Recorder(K, words)
    g = hg.GoldilocksChip(rec)
    g.load_table()
    cells = [g.assign_value(hg.Input(i)) for i in range(len(words))]
    pairs = [[cells[2 * i], cells[2 * i + 1]] for i in range(N_CONSTANTS + N_WIRES)]
    consts, wires, pi_hash = pairs[:num_selectors + 2], pairs[num_selectors + 2:], cells[-4:]
    got = hp.PlonkVerifierChip(rec, cd).eval_gate_constraints(consts, wires, pi_hash)
    values = ([val(c) for c in consts], [val(w) for w in wires], [c.value for c in pi_hash])
    return rec, got, filtered_want(cd, *values), cd, values


# ---- the extension algebra, restated over plonk_verifier's extension arithmetic ---------------------------------------------------------------
def amul(a, b):
    return (pv.add(pv.mul(a[0], b[0]), pv.mul(pv.base(7), pv.mul(a[1], b[1]))), pv.add(pv.mul(a[0], b[1]), pv.mul(a[1], b[0])))


def aadd(a, b):
    return (pv.add(a[0], b[0]), pv.add(a[1], b[1]))


def asub(a, b):
    return (pv.sub(a[0], b[0]), pv.sub(a[1], b[1]))


def ascal(c, a):
    return (pv.mul(c, a[0]), pv.mul(c, a[1]))


@functools.lru_cache(maxsize=None)
def algebra_case():
    """every GoldilocksExtensionAlgebraChip method on operands from EDGE and random ones -> (recorder, [(method, got cells, want)])"""
    rng = np.random.default_rng(0xA16E)
    words = [v for e in fc.EDGE for v in e] + [int(v) for v in rand_field(rng, 12)]
    rec = hg.Recorder(K, words)
    gea = hp.GoldilocksExtensionAlgebraChip(rec)
    gea.goldilocks_extension_chip.goldilocks_chip.load_table()
    xs = fc.ext_operands(rec)
    algs = [[xs[i], xs[i + 1]] for i in range(len(xs) - 1)]
    aval = lambda a: (val(a[0]), val(a[1]))      # noqa: E731
    out = []
    for i, a in enumerate(algs):
        b, c, e = algs[(i + 3) % len(algs)], algs[(i + 5) % len(algs)], xs[(i + 2) % len(xs)]
        out.append(("mul_add", gea.mul_add_ext_algebra(a, b, c), aadd(amul(aval(a), aval(b)), aval(c))))
        out.append(("mul", gea.mul_ext_algebra(a, b), amul(aval(a), aval(b))))
        out.append(("sub", gea.sub_ext_algebra(a, b), asub(aval(a), aval(b))))
        out.append(("scalar_mul_add", gea.scalar_mul_add_ext_algebra(e, b, c), aadd(ascal(val(e), aval(b)), aval(c))))
        out.append(("scalar_mul", gea.scalar_mul_ext_algebra(e, a), ascal(val(e), aval(a))))
        out.append(("convert", gea.convert_to_ext_algebra(e), (val(e), pv.E0)))
        pairs = [(a[0], b[1]), (e, c[0])]
        want = val(c[1])
        for x, y in pairs:
            want = pv.add(pv.mul(pv.base(5), pv.mul(val(x), val(y))), want)
        out.append(("inner_product", [gea.inner_product_extension(5, c[1], pairs)] * 2, (want, want)))
    out.append(("zero", gea.zero_ext_algebra(), (pv.E0, pv.E0)))
    return rec, out


# ---- PublicInputsHasherChip --------------------------------------------------------------------------------------------------------------------
HASH_LENGTHS = (0, 1, 7, 8, 9, 16, 17)                              # the oracle's hash_no_pad takes the empty vector too


def hasher_inputs(n):
    rng = np.random.default_rng(0x4A5 + n)
    words = [int(v) for v in rand_field(rng, n)]
    for i, v in zip(range(0, n, 3), (0, P - 1, 1)):                  # 0 and p - 1 among the inputs
        words[i] = v
    return words


@functools.lru_cache(maxsize=None)
def hasher_case(n):
    """hash(inputs, 4) of n inputs -> (recorder, output cells, [(offset, levels) after each permutation])"""
    rec = hg.Recorder(K, hasher_inputs(n))
    g = hg.GoldilocksChip(rec)
    g.load_table()
    cells = [g.assign_value(hg.Input(i)) for i in range(n)]
    chip = hp.PublicInputsHasherChip(rec)
    marks = []
    permutation = chip.permutation

    def marked():
        permutation()
        marks.append((rec.offset, max(c.level for c in chip.state)))
    chip.permutation = marked
    return rec, chip.hash(cells, 4), marks


# ---- Plonky2VerifierCircuit --------------------------------------------------------------------------------------------------------------------
class VerifierCase:
    """one proof under Plonky2VerifierCircuit: the circuit, its input vector and recorder, the challenges and the vanishing polynomial at zeta
    as plonk_verifier.py computes them"""

    def __init__(self, orc, data, cd, flat, pi):
        self.orc, self.data, self.cd, self.flat = orc, data, cd, flat
        self.pi = np.asarray(pi, dtype=np.uint64)
        self.circuit = vc.Plonky2VerifierCircuit(cd)
        self.inputs = self.circuit.inputs(flat, self.pi)
        self.rec = self.circuit.record(self.inputs)
        assert self.rec.k == K, "the recording does not fit k = 17"
        self.pi_hash = [int(v) for v in orc.hash_no_pad(self.pi)]
        proof = self.parse(flat)
        self.accepted = pv.verify(orc, cd, proof)                    # raises unless plonk_verifier.py accepts the proof
        self.challenges = fc.challenges(orc, cd, proof, self.pi_hash)
        op = {k: [pv.ext(v) for v in vals] for k, vals in proof["openings"].items()}
        zeta = tuple(int(v) for v in self.accepted["zeta"])
        self.vanishing = pv.eval_vanishing_poly(cd, zeta, pv.ext_pow(zeta, 1 << cd["degree_bits"]), op, self.pi_hash, self.accepted["betas"],
                                                self.accepted["gammas"], self.accepted["alphas"])

    def parse(self, flat):
        proof = plonk.parse_proof(self.data, flat)
        proof["public_inputs"] = self.pi
        return proof

    def mutations(self):
        """-> {name: input vector}, one word changed each"""
        c = self.circuit
        words = dict(wire_opening=c.openings["wires"][1][0], constant_opening=c.openings["constants"][c.cd["num_selectors"]][0],
                     zs_next_opening=c.openings["plonk_zs_next"][0][1], partial_product_opening=c.openings["partial_products"][1][0],
                     quotient_opening=c.openings["quotient_polys"][1][0], public_input=c.public_inputs[1])
        out = {}
        for name, word in words.items():
            bad = self.inputs.copy()
            bad[word] = (int(bad[word]) + 1) % P
            out[name] = bad
        return out


def all_gates_proof(orc):
    """a small GadgetBuilder circuit that uses all 12 gate kinds, proved by the CPU prover under halo2_fri_cases.CONFIG
    -> (CircuitData, flat proof, public inputs)"""
    rng = np.random.default_rng(0x7A9E)
    b = gad.GadgetBuilder(plonk.CircuitConfig(zero_knowledge=False, **fc.CONFIG))
    inputs = rand_field(rng, 48)
    inputs[8] = 1
    t = [plonk.Src(v, i) for i, v in enumerate(inputs)]
    xs = b.add_virtual_targets(t[:8])
    s = b.add(b.mul(xs[0], xs[1]), xs[2])
    q = b.ext_div(b.ext_mul((xs[0], xs[1]), (xs[2], xs[3])), (xs[2], xs[3]))
    h = b.hash_n_to_hash_no_pad(xs + xs[:3])
    bit = b.add_virtual_target(t[8])
    b.assert_bool(bit)
    b.permute_swapped(xs + [b.zero()] * 4, swap=bit)
    bits = b.split_le_64(xs[5])
    items = b.add_virtual_targets(t[9:25])
    b.random_access(b.le_sum(bits[:4]), items)
    red = b.reduce_with_powers_base(b.add_virtual_targets(t[25:40]), (xs[6], xs[7]))
    ext_coeffs = b.add_virtual_targets(t[40:48])
    red_ext = b.reduce_with_powers_ext([(ext_coeffs[2 * i], ext_coeffs[2 * i + 1]) for i in range(4)], (xs[6], xs[7]))
    b.mds_ext([(items[2 * i], items[2 * i + 1]) for i in range(6)] * 2)
    # the builder has no gadget over MulExtensionGate: one row of it by hand, two of its 13 operations filled (wires 6 i .. 6 i + 5:
    # two multiplicands and const_0 times their product, in the extension algebra over base-field wires)
    c0 = 3
    row = b._new_row(pv.MUL_EXT, 13, constants=[c0])
    for i in range(2):
        x, y = (int(inputs[4 * i]), int(inputs[4 * i + 1])), (int(inputs[4 * i + 2]), int(inputs[4 * i + 3]))
        z = gad.emul(x, y)
        for col, v in enumerate(list(x) + list(y) + [c0 * z[0] % P, c0 * z[1] % P]):
            b._set(row, 6 * i + col, v)
    b.register_public_inputs([s, h[0], red[1], q[0], red_ext[0]])
    pi = np.array(b.finalize_public_inputs(), dtype=np.uint64)
    data = b.cb.layout()
    cpu = CpuProver.from_circuit_data(orc, data)
    data.set_digest(cpu.cap())
    for i in range(4):
        cpu.pd.circuit_digest[i] = int(data.circuit_digest[i])
    idx, vals = b.sparse_witness()
    return data, cpu.prove_sparse(idx, vals, pi, 41), pi


@functools.lru_cache(maxsize=None)
def verifier_case(name):
    """name: "zk", "plain" (the two Semaphore proofs of halo2_fri_cases, 12 public inputs: two hasher permutations) or "all_gates" """
    if name == "all_gates":
        orc = Oracle()
        data, flat, pi = all_gates_proof(orc)
        return VerifierCase(orc, data, data.common(), flat, pi)
    c = fc.case(name == "zk")
    return VerifierCase(c.orc, c.data, c.cd, c.flat, c.pi)


@functools.lru_cache(maxsize=None)
def verifier_mutations(name):
    return verifier_case(name).mutations()


@functools.lru_cache(maxsize=None)
def vanishing_alone_case():
    """verify_vanishing_identity on random openings and challenges (no proof): the values must be the model's, the identity must fail"""
    cd = verifier_case("plain").cd
    rng = np.random.default_rng(0x7A21)
    nch, n_const = cd["num_challenges"], cd["num_selectors"] + cd["num_constants"]
    counts = dict(constants=n_const, plonk_sigmas=cd["num_routed_wires"], wires=cd["num_wires"], plonk_zs=nch, plonk_zs_next=nch,
                  partial_products=nch * cd["num_partial_products"], quotient_polys=nch * cd["quotient_degree_factor"])
    n = 2 * sum(counts.values()) + 4 + 2 + 3 * nch
    rec = hg.Recorder(K, [int(v) for v in rand_field(rng, n)])
    g = hg.GoldilocksChip(rec)
    g.load_table()
    it = iter([g.assign_value(hg.Input(i)) for i in range(n)])
    take = lambda m: [next(it) for _ in range(m)]      # noqa: E731
    op = {name: [take(2) for _ in range(count)] for name, count in counts.items()}
    pi_hash, zeta, betas, gammas, alphas = take(4), take(2), take(nch), take(nch), take(nch)
    chip = hp.PlonkVerifierChip(rec, cd)
    got = chip.verify_vanishing_identity(op, pi_hash, zeta, betas, gammas, alphas)
    z = val(zeta)
    want = pv.eval_vanishing_poly(cd, z, pv.ext_pow(z, 1 << cd["degree_bits"]), {k: [val(e) for e in v] for k, v in op.items()},
                                  [c.value for c in pi_hash], *[[c.value for c in cs_] for cs_ in (betas, gammas, alphas)])
    return rec, got, want, chip.identity_rows


def failing_assert_rows(rec):
    """-> [the set of rows its two operands name] for every failing ASSERT_EQ entry of the recorder"""
    return [{int(w) & 0xFFFFFFFFFF for w in e[4]} for e in rec.entries if e[5] and e[2] == hg.OP_ASSERT_EQ]


# ---- synthetic tapes for the device's run form ------------------------------------------------------------------------------------------------
RUN_WIDTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def _rec(words):
    rec = hg.Recorder(K, words)
    g = hg.GoldilocksChip(rec)
    g.load_table()
    return rec, g


def _widths_levels(rec, g, first, last, widths):
    """one level per width: every entry multiplies the first and the last cell the previous level wrote and adds its own index"""
    ar = g.arithmetic_chip
    for width in widths:
        row = [ar.apply(first, last, g.assign_constant(i)).r for i in range(width)]
        assert len({c.level for c in row}) == 1
        first, last = row[0], row[-1]
    return first, last


@functools.lru_cache(maxsize=None)
def run_case(name):
    """-> recorder.  chain: 3 000 dependent MULADD entries, one per level.  widths: the RUN_WIDTHS levels, twice over.  seams: runs cut by a
    PERMUTE level and by a level wider than any run_max in use, with runs of one and of two levels at the seams.  ops: PACK, UNPACK, VALUE
    with INV and INV_EXT and ASSERT_EQ inside a run, exactly two of the assertions failing, in different levels.  one_run: no CONST entry and no
    PERMUTE, so the whole tape is one run"""
    if name == "chain":
        rec, g = _rec([3, 5])
        a, b = g.assign_value(hg.Input(0)), g.assign_value(hg.Input(1))
        acc = a
        for _ in range(3000):
            acc = g.mul_add(acc, b, a)
        return rec
    if name == "widths":
        rec, g = _rec([3, 5])
        a, b = g.assign_value(hg.Input(0)), g.assign_value(hg.Input(1))
        for i in range(2049):
            g.assign_constant(i)                                     # the constants first: level 1
        _widths_levels(rec, g, a, b, RUN_WIDTHS + RUN_WIDTHS)
        return rec
    if name == "seams":
        rec, g = _rec([3, 5, 7])
        a, b, c = (g.assign_value(hg.Input(i)) for i in range(3))
        for i in range(5000):
            g.assign_constant(i)
        first, last = _widths_levels(rec, g, a, b, (3, 2, 4))        # with the PACK level (4 wide): a run of four levels, after the wide opening level
        state = g.all_chip.permute([first, last, c] * 4)             # PACK level, PERMUTE level, UNPACK level
        first, last = _widths_levels(rec, g, state[0], state[11], (2,))      # with the UNPACK level: a run of two
        first, last = _widths_levels(rec, g, first, last, (5000,))   # wider than run_max
        first, last = _widths_levels(rec, g, first, last, (1,))      # a single narrow level between two wide ones: no run
        first, last = _widths_levels(rec, g, first, last, (4999,))
        _widths_levels(rec, g, first, last, (2, 2))                  # a run of two at the end
        return rec
    if name == "ops":
        rec, g = _rec([3, 5, 7, 0, 0, P - 1])
        ge = hg.GoldilocksExtensionChip(rec)
        ar = g.arithmetic_chip
        cells = [g.assign_value(hg.Input(i)) for i in range(6)]
        packed = ar.pack(cells[:3])
        digits = ar.unpack(packed)
        g.assert_equal(digits[1], cells[1])
        nz = g.is_zero(cells[3])                                     # INV of zero
        g.is_zero(cells[0])                                          # INV
        q = ge.div_extension(cells[0:2], cells[1:3])                 # INV_EXT
        g.assert_equal(nz, cells[3])                                 # fails (1 != 0), in an early level
        g.assert_equal(g.mul(g.mul(q[0], q[1]), cells[5]), cells[0])      # fails, two levels later
        return rec
    assert name == "one_run"
    rec = hg.Recorder(K, [3, 5, 7, 11])
    ar = hg.ArithmeticChip(rec)
    rec.table_loaded = True
    cells = [ar.assign_value(hg.Input(i)) for i in range(4)]
    for i in range(40):
        cells = [ar.apply(cells[j], cells[(j + 1) % 4], cells[(j + 2) % 4]).r for j in range(4)]
        if i % 8 == 0:
            cells[0] = ar.assign_value(cells[0])
    ar.assert_equal(cells[0], cells[0])
    return rec


RUN_CASES = ("chain", "widths", "seams", "ops", "one_run")
