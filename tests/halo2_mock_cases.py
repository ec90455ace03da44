"""The circuits and the mutated witnesses of the MockProver tests (tests/test_halo2_mock_model.py on the CPU, tests/test_gpu_plonk_check.py on
the device): the reference's chip shape (halo2_chips.synthetic_circuit) at k = 7 .. 10, halo2_circuits.plonk_with_tuple_lookup at k = 7 and 9,
halo2_circuits.random_circuit for the twelve seeds of tests/test_gpu_halo2.py -- and five classes of mutation, each applied to up to CELLS cells
drawn by a fixed seed from the cells the model (tests/halo2_mock_model.py) reports as constrained:
  gate_cell     an advice cell inside an active gate row (+1)
  lookup_input  an advice cell a lookup input reads, pushed to a value outside the table
  copy_member   one advice member of a copy cycle (+1)
  instance      an instance value (+1)
  blinding_row  an advice cell in the first blinding row (row `usable`) that a gate reads through a positive rotation -- with that gate's
                selector switched ON at the last usable row, the circuit bug halo2's poison exists to catch: whatever the cell holds, the
                prover overwrites it.  This class changes a FIXED cell too, so it comes with its own fixed columns.
A class applies to a circuit only if the circuit has the structure (lookups / copy cycles / instance columns / rotated gates); every class
that applies must make the model report at least one failure (test_halo2_mock_model.py asserts that for every circuit here)."""
import importlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from halo2_circuits import plonk_with_tuple_lookup, random_circuit  # noqa: E402
from halo2_mock_model import GATE, GATE_POISONED, LOOKUP, MockModel  # noqa: E402

h2 = importlib.import_module("stark-verifier_amd.halo2")
ch = importlib.import_module("stark-verifier_amd.halo2_chips")
R = h2.R
CELLS = 3
CLASSES = ("gate_cell", "lookup_input", "copy_member", "instance", "blinding_row")

CIRCUITS = ([("chips-k%d" % k, k) for k in (7, 8, 9, 10)] + [("tuple-k%d" % k, k) for k in (7, 9)] + [("random-%d" % s, 6 + s % 3) for s in range(12)])


def build(name):
    """-> (cs, k, Witness)"""
    kind, arg = name.split("-")
    if kind == "chips":
        k = int(arg[1:])
        cs, _, w = ch.synthetic_circuit(k, table_bits={7: 5, 8: 6, 9: 7, 10: 7}[k], n_permutations=1, seed=0x355)
    elif kind == "tuple":
        k = int(arg[1:])
        cs, w = plonk_with_tuple_lookup(k, {7: 5, 9: 6}[k])
    else:
        k = 6 + int(arg) % 3
        cs, w = random_circuit(k, int(arg))
    return cs, k, w


def advice_queries(e, cs, acc):
    """the (column, rotation) advice queries of an expression tree"""
    if e.op == "query":
        if e.a == h2.ADVICE:
            acc.add(cs.queries[h2.ADVICE][e.b])
    elif e.op != "const":
        advice_queries(e.a, cs, acc)
        if e.op in ("add", "mul"):
            advice_queries(e.b, cs, acc)
    return acc


def fixed_queries(e, cs, acc):
    if e.op == "query":
        if e.a == h2.FIXED:
            acc.add(cs.queries[h2.FIXED][e.b])
    elif e.op != "const":
        fixed_queries(e.a, cs, acc)
        if e.op in ("add", "mul"):
            fixed_queries(e.b, cs, acc)
    return acc


def walk(e):
    yield e
    if e.op not in ("const", "query"):
        yield from walk(e.a)
        if e.op in ("add", "mul"):
            yield from walk(e.b)


class Case:
    """one circuit with its satisfying witness as integers, its model and the model's verdict on the clean witness"""

    def __init__(self, name):
        self.name = name
        self.cs, self.k, self.w = build(name)
        w = self.w
        self.n, self.usable = w.n, w.usable
        self.fixed = w.fixed_ints()
        self.advice = w.advice_ints()
        self.instances = [list(c) for c in w.instance]
        self.mapping = w.assembly.mapping_array()
        self.model = MockModel(self.cs, self.k, self.fixed, self.mapping)
        self.clean = self.model.verify(self.advice, self.instances)
        self.tables = self.model.tables(self.advice, self.instances)
        # do the table expressions read anything but fixed columns?  If not, a change of advice or instance cells leaves the tables alone
        self.tables_read_witness = any(e.op == "query" and e.a != h2.FIXED for _, _, tabs in self.cs.lookups for t in tabs for e in walk(t))

    def near(self, advice, instances, changed_rows, fixed=None):
        model = self.model if fixed is None else MockModel(self.cs, self.k, fixed, self.mapping)
        return model.verify_near(self.tables, self.clean, advice, instances, changed_rows, tables_unchanged=fixed is None and not self.tables_read_witness)

    # ---- candidates per class: (advice column, row, new value) | (instance column, row, new value) ---------------------------------------
    def _try_advice(self, col, row, value):
        adv = list(self.advice)
        adv[col] = list(adv[col])
        adv[col][row] = value % R
        return adv

    def applies(self, cls):
        """by the circuit's STRUCTURE alone: does it have what the class targets?"""
        cs = self.cs
        if cls == "gate_cell":
            return bool(cs.gates)
        if cls == "lookup_input":
            return any(advice_queries(e, cs, set()) for _, ins, _ in cs.lookups for e in ins)
        if cls == "copy_member":
            return any(col.kind == h2.ADVICE and tuple(int(v) for v in self.mapping[j][i]) != (j, i) for j, col in enumerate(cs.permutation) for i in range(self.n))
        if cls == "instance":
            return any(len(c) for c in self.instances)
        # a gate polynomial that reads advice one row ahead and has a fixed column (its selector) at the current row
        return any(any(rot == 1 for _, rot in advice_queries(p, cs, set())) and any(rot == 0 for _, rot in fixed_queries(p, cs, set())) for p in cs.all_gate_polys())

    def mutation(self, cls, seed=0x355):
        """-> None if the class does not apply to this circuit, else dict(advice, instances, fixed (None: unchanged), cells, failures): the
        mutated witness as integers, the cells that were changed and the model's complete failure list"""
        if not self.applies(cls):
            return None
        rng = random.Random("%s/%s/%d" % (self.name, cls, seed))
        cs, u = self.cs, self.usable
        picked, rows = [], set()
        adv, inst, fixed = [list(c) for c in self.advice], [list(c) for c in self.instances], None
        if cls == "gate_cell":
            cand = [(c, r) for c in range(cs.num_advice) for r in range(u)]
            rng.shuffle(cand)
            for c, r in cand[:400]:
                f = self.near(self._try_advice(c, r, self.advice[c][r] + 1), self.instances, {r})
                if any(x[0] == GATE for x in f):
                    picked.append(("advice", c, r))
                    adv[c][r] = (adv[c][r] + 1) % R
                    rows.add(r)
                    if len(picked) == CELLS:
                        break
        elif cls == "lookup_input":
            if not cs.lookups:
                return None
            cand = []
            for li, (_, ins, _) in enumerate(cs.lookups):
                for col, rot in sorted(set().union(*[advice_queries(e, cs, set()) for e in ins])):
                    cand += [(col, r) for r in range(u) if 0 <= r - rot < u]
            cand = sorted(set(cand))
            rng.shuffle(cand)
            for c, r in cand[:400]:
                outside = R - 1 - rng.randrange(1 << 40)                 # no table of these circuits holds a value this close to r
                f = self.near(self._try_advice(c, r, outside), self.instances, {r})
                if any(x[0] == LOOKUP and x[3] == 0 for x in f):
                    picked.append(("advice", c, r))
                    adv[c][r] = outside
                    rows.add(r)
                    if len(picked) == CELLS:
                        break
        elif cls == "copy_member":
            cand = [(j, i) for j, col in enumerate(cs.permutation) if col.kind == h2.ADVICE for i in range(self.n)
                    if tuple(int(v) for v in self.mapping[j][i]) != (j, i)]
            if not cand:
                return None
            rng.shuffle(cand)
            for j, i in cand[:CELLS]:
                c = cs.permutation[j].index
                picked.append(("advice", c, i))
                adv[c][i] = (adv[c][i] + 1) % R
                rows.add(i)
        elif cls == "instance":
            cand = [(c, r) for c in range(cs.num_instance) for r in range(len(self.instances[c]))]
            if not cand:
                return None
            rng.shuffle(cand)
            for c, r in cand[:CELLS]:
                picked.append(("instance", c, r))
                inst[c][r] = (inst[c][r] + 1) % R
                rows.add(r)
        elif cls == "blinding_row":
            # a polynomial that reads advice at rotation +1 and a fixed column at rotation 0: that fixed cell := 1 at the last usable row
            cand = []
            for _, polys in cs.gates:
                for poly in polys:
                    aq = [c for c, rot in advice_queries(poly, cs, set()) if rot == 1]
                    fq = [c for c, rot in fixed_queries(poly, cs, set()) if rot == 0]
                    cand += [(f, a) for f in fq for a in aq]
            cand = sorted(set(cand))
            if not cand:
                return None
            rng.shuffle(cand)
            fixed = [list(c) for c in self.fixed]
            for f, a in cand:
                trial = [list(c) for c in fixed]
                trial[f][u - 1] = 1
                if any(x[0] == GATE_POISONED for x in self.near(self.advice, self.instances, {u - 1}, fixed=trial)):
                    fixed = trial
                    adv[a][u] = rng.randrange(R)
                    picked += [("fixed", f, u - 1), ("advice", a, u)]
                    rows |= {u - 1, u}
                    if len(picked) >= 2 * CELLS:
                        break
            if not picked:
                fixed = None
        else:
            raise ValueError(cls)
        assert picked, "%s: no constrained cell found for class %s" % (self.name, cls)
        failures = self.near(adv, inst, rows, fixed=fixed)
        return dict(advice=adv, instances=inst, fixed=fixed, cells=picked, failures=failures)

    # ---- the arrays the library takes -------------------------------------------------------------------------------------------------------
    def advice_array(self, m=None):
        a = self.w.advice.copy()
        for kind, c, r in (m["cells"] if m else ()):
            if kind == "advice":
                self.w.set_int(a, c, r, m["advice"][c][r])
        return a

    def fixed_array(self, m=None):
        a = self.w.fixed.copy()
        for kind, c, r in (m["cells"] if m else ()):
            if kind == "fixed":
                self.w.set_int(a, c, r, m["fixed"][c][r])
        return a


def poison_only(failures):
    """every record is a poisoned gate or a poisoned lookup input: the prover's blinding values decide whether a proof verifies"""
    return bool(failures) and all(f[0] == GATE_POISONED or (f[0] == LOOKUP and f[3] == 1) for f in failures)
