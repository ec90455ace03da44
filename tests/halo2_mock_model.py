"""A plain-Python restatement of gl355_plonk_check_witness (include/gl355.h), i.e. of halo2's MockProver::verify as the reference runs it
(verifier_api.rs:34-52, :72-73): the checker the device's failure list is compared with, record for record.

It works on the `Expression` TREES of a ConstraintSystem with a poison-carrying value -- never on the compiled register programs -- so a
mistake in ProgramBuilder (sharing of subexpressions, register allocation, operand order) or in the device interpreter shows as a difference.

Rules, with n = 2^k and usable = n - (blinding_factors + 1):
  value     (v, poisoned).  An ADVICE query that lands in a row >= usable is poisoned (the prover overwrites those rows with blinding values);
            fixed and instance queries never are (instance columns are padded with zeros).  Sum and negation pass poison on; a product is
            poisoned if an operand is, unless the OTHER operand is an unpoisoned zero: then it is an unpoisoned zero (halo2's
            Value::Real(0) * Poison = Real(0)).  Scaling is a product with an unpoisoned constant.
  gates     every polynomial (ordinal = cs.all_gate_polys() order) at every row < usable: poisoned -> (GATE_POISONED, ordinal, row, 0), else
            non-zero -> (GATE, ordinal, row, 0)
  lookups   table = the table tuples of the rows < usable with no poisoned element; every row < usable: a poisoned input tuple ->
            (LOOKUP, lookup, row, 1), else not in the table -> (LOOKUP, lookup, row, 0)
  copies    every cell (j, i), i < n, of the permutation's columns against the cell mapping[j][i] names: (PERMUTATION, j, i, partner's j)
The result is the complete list, sorted by (kind, index, row)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
h2 = importlib.import_module("stark-verifier_amd.halo2")
R = h2.R
GATE, GATE_POISONED, LOOKUP, PERMUTATION = range(4)


def mul(a, b):
    (x, px), (y, py) = a, b
    if (px or py) and not ((not px and x == 0) or (not py and y == 0)):
        return (0, True)
    return (x * y % R, False)


def evaluate(e, query):
    """e: h2.Expression; query(kind, query index) -> (value, poisoned).  -> (value, poisoned); the value of a poisoned result means nothing"""
    op = e.op
    if op == "const":
        return (e.a, False)
    if op == "query":
        return query(e.a, e.b)
    if op == "neg":
        v, p = evaluate(e.a, query)
        return ((-v) % R, p)
    if op == "scale":
        return mul(evaluate(e.a, query), (e.b, False))
    x, y = evaluate(e.a, query), evaluate(e.b, query)
    if op == "add":
        return ((x[0] + y[0]) % R, x[1] or y[1])
    assert op == "mul"
    return mul(x, y)


class MockModel:
    """cs, k and the circuit's side (fixed: [column][row] integers, mapping: [n_perm][n][2] or None)"""

    def __init__(self, cs, k, fixed, mapping):
        self.cs, self.k, self.n = cs, k, 1 << k
        self.usable = self.n - (cs.blinding_factors() + 1)
        self.fixed, self.mapping = fixed, mapping
        self.rotations = sorted({rot for kind in cs.queries for _, rot in cs.queries[kind]})

    def _query_at(self, advice, instances, row):
        cs, n, usable, fixed = self.cs, self.n, self.usable, self.fixed

        def q(kind, qi):
            col, rot = cs.queries[kind][qi]
            r = (row + rot) % n
            if kind == h2.ADVICE:
                return (advice[col][r] % R, r >= usable)
            if kind == h2.FIXED:
                return (fixed[col][r] % R, False)
            return (instances[col][r] % R if r < len(instances[col]) else 0, False)
        return q

    def cell(self, advice, instances, column, row):
        if column.kind == h2.ADVICE:
            return advice[column.index][row] % R
        if column.kind == h2.FIXED:
            return self.fixed[column.index][row] % R
        return instances[column.index][row] % R if row < len(instances[column.index]) else 0

    def readers(self, rows):
        """the rows whose gates and lookup inputs can read a cell of one of `rows`"""
        return sorted({(r - rot) % self.n for r in rows for rot in self.rotations})

    def verify(self, advice, instances, rows=None, tables=None):
        """advice: [column][row] integers, instances: per column a list.  rows: None, or the only rows at which gates and lookup inputs are
        evaluated (tables and copy constraints are always checked in full) -- for a witness that differs from a satisfying one in a few
        cells, rows = readers(changed rows) gives the complete list at a fraction of the cost, PROVIDED the tables did not change
        (verify_near does that bookkeeping).  tables: this witness's tables() if the caller has them already."""
        cs, usable = self.cs, self.usable
        rows = range(usable) if rows is None else [r for r in rows if r < usable]
        out = []
        ordinal = 0
        for _, polys in cs.gates:
            for poly in polys:
                for row in rows:
                    v, p = evaluate(poly, self._query_at(advice, instances, row))
                    if p:
                        out.append((GATE_POISONED, ordinal, row, 0))
                    elif v:
                        out.append((GATE, ordinal, row, 0))
                ordinal += 1
        for li, table in enumerate(self.tables(advice, instances) if tables is None else tables):
            ins = cs.lookups[li][1]
            for row in rows:
                t = [evaluate(e, self._query_at(advice, instances, row)) for e in ins]
                if any(p for _, p in t):
                    out.append((LOOKUP, li, row, 1))
                elif tuple(v for v, _ in t) not in table:
                    out.append((LOOKUP, li, row, 0))
        if self.mapping is not None:
            for j, col in enumerate(cs.permutation):
                for i in range(self.n):
                    cj, ci = (int(v) for v in self.mapping[j][i])
                    if (cj, ci) != (j, i) and self.cell(advice, instances, col, i) != self.cell(advice, instances, cs.permutation[cj], ci):
                        out.append((PERMUTATION, j, i, cj))
        return sorted(out)

    def tables(self, advice, instances):
        out = []
        for _, _, tabs in self.cs.lookups:
            table = set()
            for row in range(self.usable):
                t = [evaluate(e, self._query_at(advice, instances, row)) for e in tabs]
                if not any(p for _, p in t):
                    table.add(tuple(v for v, _ in t))
            out.append(table)
        return out

    def verify_near(self, clean_tables, clean_failures, advice, instances, changed_rows, tables_unchanged=False):
        """the complete list for a (circuit, witness) that differs from a reference pair -- whose tables are clean_tables and whose complete
        list is clean_failures -- only in cells (advice, instance or fixed) of `changed_rows`: rows that cannot read a changed cell keep their
        verdicts, unless a table changed (then everything is redone).  tables_unchanged: the caller knows that no table expression reads a
        changed cell (say: only advice changed and the tables read fixed columns), so the tables are not recomputed."""
        tables = clean_tables if tables_unchanged else self.tables(advice, instances)
        if tables != clean_tables:
            return self.verify(advice, instances, tables=tables)
        dirty = set(self.readers(changed_rows))
        kept = [f for f in clean_failures if f[0] != PERMUTATION and f[2] not in dirty]
        return sorted(kept + self.verify(advice, instances, rows=sorted(dirty), tables=tables))
