"""The reference's Goldilocks chips over AllChipConfig as a RECORDER (part 1 of the Halo2 verifier circuit): every method emits the
rows, selectors, fixed cells and copy constraints the Rust emits, in the same order, and at the same time
  * the static layout: fixed columns (selectors, round constants, the `constant` column, the range table) and the copy constraints, i.e. what
    gl355_plonk_keygen / gl355_plonk_check_witness take, with the number of rows used;
  * a tape (csrc/halo2_tape.h): chip-level entries that compute every advice cell from an input vector (the proof's words), replayed per proof by
    gl355_halo2_synthesize (device) or gl355_halo2_synthesize_host;
  * every value, eagerly, in Python integers: the third, independent formulation the tests compare the two interpreters with.

  RegionCtx                         context.rs (offset, next, set_offset, the registered constants of assign_constant)
  ArithmeticChip                    chip/native_chip/arithmetic_chip.rs:204-534
  AllChip.permute                   chip/native_chip/all_chip.rs:52-89 (the 69 Poseidon rows run beside the pack / unpack rows)
  GoldilocksChip                    chip/goldilocks_chip.rs:68-415
  HasherChip                        chip/hasher_chip.rs:30-171 (rate 8, overwrite mode)
  VectorChip.access                 chip/vector_chip.rs:26-48
  MerkleProofChip                   chip/merkle_proof_chip.rs:39-87
  GoldilocksExtensionChip           chip/goldilocks_extension_chip.rs:56-416
  TranscriptChip                    chip/transcript_chip.rs:17-74
  FriVerifierChip                   chip/fri_chip.rs:58-376

A term of `apply` is a Cell (Term::Assigned: copied into the row) or an unassigned value the prover derives: Input(i) (a proof word), BitOf(cell, i),
InvOf(cell); assign_value also takes InvExtOf(cell0, cell1, component), a component of a quadratic-extension inverse.  Cells that take part in Goldilocks arithmetic hold values below 2^64; only the packed scalars (pack's result, the Poseidon state)
are wider, and they only ever feed PACK / UNPACK / PERMUTE entries and copy constraints."""
import hashlib
import io

import numpy as np

from . import halo2 as h2
from . import halo2_chips as hc

P = hc.GOLDILOCKS_MODULUS
R = h2.R
(OP_CONST, OP_VALUE, OP_MULADD, OP_MULADD_EXT, OP_PACK, OP_UNPACK, OP_PERMUTE, OP_ASSERT_EQ) = range(1, 9)
K_CELL, K_INPUT, K_BIT, K_INV, K_INV_EXT = 1, 2, 3, 4, 5
W = 7                               # GF(p)[X] / (X^2 - W)
ENTRY_WORDS, N_ADVICE, PERMUTE_ROWS = 8, 19, 69
NO_FAILURE = (1 << 64) - 1


class Cell:
    """an assigned advice cell: column index, row, its eager value and the level of the tape entry that writes it"""
    __slots__ = ("col", "row", "value", "level")

    def __init__(self, col, row, value, level):
        self.col, self.row, self.value, self.level = col, row, value, level

    def word(self, kind=K_CELL, aux=0):
        return (kind << 60) | (aux << 48) | (self.col << 40) | self.row


class Input:
    def __init__(self, index):
        self.index = index


class BitOf:
    def __init__(self, cell, bit):
        self.cell, self.bit = cell, bit


class InvOf:
    def __init__(self, cell):
        self.cell = cell


class InvExtOf:
    """component `component` of 1 / (cell0 + cell1 X), (0, 0) for (0, 0): an assign_value term only (its VALUE entry names cell1 in a second word)"""

    def __init__(self, cell0, cell1, component):
        self.cell0, self.cell1, self.component = cell0, cell1, component


def ext_inverse(y0, y1):
    """(y0 - y1 X) / (y0^2 - 7 y1^2) in GF(p)[X] / (X^2 - 7): the norm is 0 only for (0, 0), which gives (0, 0)"""
    inv = pow((y0 * y0 - W * y1 * y1) % P, P - 2, P)
    return (y0 * inv % P, (P - y1) % P * inv % P)


class Recorder:
    """RegionCtx over one region that starts at row 0, plus the three outputs.  inputs: the input vector the eager values are computed from."""

    def __init__(self, k, inputs=()):
        self.k, self.n = k, 1 << k
        self.cs = h2.ConstraintSystem()
        self.cfg = hc.AllChipConfig.configure(self.cs)
        self.ar, self.po = self.cfg.arithmetic_config, self.cfg.poseidon_config
        assert self.cs.num_advice == N_ADVICE and self.ar.a.index == 0 and self.po.state[0].index == 14
        self.usable = self.n - (self.cs.blinding_factors() + 1)
        self.inputs = [int(v) for v in inputs]
        self.offset = 0
        self.rows_used = 0
        self.values = {}                # (advice column, row) -> integer
        self.fixed = {}                 # (fixed column, row) -> integer (the range table apart)
        self.copies = []                # ((Column, row), (Column, row))
        self.instance = []              # the instance column's values
        self.entries = []               # [level, sequence, op, row, operand words, failed]
        self.constants = {}             # value -> Cell (RegionCtx::get_fixed / register_fixed)
        self.table_loaded = False
        self._order = None
        self._advice_columns = [h2.Column(h2.ADVICE, i) for i in range(N_ADVICE)]

    # ---- RegionCtx ----------------------------------------------------------------------------------------------------------------------
    def next(self, rows=1):
        self.offset += rows
        self.rows_used = max(self.rows_used, self.offset)
        assert self.rows_used <= self.usable, "the circuit does not fit 2^%d rows" % self.k

    def set_offset(self, offset):
        self.offset = offset

    def shrink_to_fit(self, min_k=17):
        """the smallest k >= min_k (17 holds the 16-bit range table) whose usable rows hold what was recorded: the rows do not depend on k, so a
        circuit whose size is not known in advance is recorded under a large k and fixed afterwards"""
        k = min_k
        while (1 << k) - (self.cs.blinding_factors() + 1) < max(self.rows_used, len(self.instance)):
            k += 1
        assert k <= self.k
        self.k, self.n = k, 1 << k
        self.usable = self.n - (self.cs.blinding_factors() + 1)

    def enable(self, selector, row=None):
        self.fixed[(selector.index, self.offset if row is None else row)] = 1

    def set(self, col, row, value):
        assert (col, row) not in self.values, "advice cell (%d, %d) assigned twice" % (col, row)
        self.values[(col, row)] = value % R

    def copy(self, a, b):
        """constrain_equal on two cells given as Cell or (Column, row)"""
        cols = self._advice_columns
        self.copies.append(((cols[a.col], a.row) if isinstance(a, Cell) else a, (cols[b.col], b.row) if isinstance(b, Cell) else b))

    def emit(self, op, row, operands, level, failed=False):
        self._order = None
        self.entries.append([level, len(self.entries), op, row, list(operands), bool(failed)])

    def term(self, t):
        """-> (operand word, eager value, level of its writer)"""
        if isinstance(t, InvExtOf):
            y0, y1 = ((c.value & ((1 << 64) - 1)) % P for c in (t.cell0, t.cell1))
            return t.cell0.word(K_INV_EXT, t.component), ext_inverse(y0, y1)[t.component], max(t.cell0.level, t.cell1.level)
        if isinstance(t, Cell):
            return t.word(), t.value, t.level
        if isinstance(t, Input):
            return (K_INPUT << 60) | t.index, self.inputs[t.index], 0
        if isinstance(t, BitOf):
            return t.cell.word(K_BIT, t.bit), ((t.cell.value & ((1 << 64) - 1)) >> t.bit) & 1, t.cell.level
        assert isinstance(t, InvOf)
        v = (t.cell.value & ((1 << 64) - 1)) % P
        return t.cell.word(K_INV), pow(v, P - 2, P) if v else 0, t.cell.level

    # ---- the outputs ---------------------------------------------------------------------------------------------------------------------
    def _sorted(self):
        if self._order is None:
            self._order = sorted(self.entries, key=lambda e: (e[0], e[1]))
        return self._order

    def tape(self):
        es = self._sorted()
        out = np.zeros((len(es), ENTRY_WORDS), dtype=np.uint64)
        for i, (level, _, op, row, operands, _) in enumerate(es):
            out[i, 0], out[i, 1] = op | (level << 8), row
            for j, w in enumerate(operands):
                out[i, 2 + j] = w
        return out.reshape(-1)

    def status(self):
        """(the smallest failing entry of the tape or 2^64 - 1, the number of failing entries), from the eager values"""
        bad = [i for i, e in enumerate(self._sorted()) if e[5]]
        return (bad[0] if bad else NO_FAILURE, len(bad))

    def entry_rows(self, index):
        """(first row, number of rows) of entry `index` of the tape"""
        e = self._sorted()[index]
        return e[3], {OP_MULADD_EXT: 2, OP_PACK: 3, OP_UNPACK: 8, OP_PERMUTE: PERMUTE_ROWS, OP_ASSERT_EQ: 0}.get(e[2], 1)

    def level_widths(self):
        widths = {}
        for e in self.entries:
            widths[e[0]] = widths.get(e[0], 0) + 1
        return [widths[l] for l in sorted(widths)]

    def advice(self):
        out = np.zeros((N_ADVICE, self.n, 4), dtype=np.uint64)
        _fill(out, self.values)
        return out

    def layout(self):
        return Layout(self.k, len(self.inputs), self.rows_used, self.fixed, self.copies, self.table_loaded, len(self.instance), cs=self.cs, cfg=self.cfg)

    def artifact(self):
        return Artifact(self.layout(), self.tape())


def _fill(arr, cells):
    if not cells:
        return
    keys = np.array(list(cells.keys()), dtype=np.int64)
    vals = list(cells.values())
    for j in range(4):
        arr[keys[:, 0], keys[:, 1], j] = np.array([(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)


class Layout:
    """the circuit's side of a recorded circuit: what keygen and the witness check take"""

    def __init__(self, k, n_inputs, rows_used, fixed, copies, table_loaded, n_instance, cs=None, cfg=None):
        """cs, cfg: the recorder's constraint system and AllChipConfig (configured afresh when not given)"""
        self.k, self.n, self.n_inputs, self.rows_used, self.table_loaded, self.n_instance = k, 1 << k, n_inputs, rows_used, table_loaded, n_instance
        if cs is None:
            cs = h2.ConstraintSystem()
            cfg = hc.AllChipConfig.configure(cs)
        self.cs, self.cfg = cs, cfg
        perm = {col: i for i, col in enumerate(self.cs.permutation)}
        self.fixed_cells = np.zeros((len(fixed), 6), dtype=np.uint64)          # [column, row, four limbs], in recording order
        if fixed:
            self.fixed_cells[:, :2] = np.array(list(fixed.keys()), dtype=np.uint64)
            vals = list(fixed.values())
            for j in range(4):
                self.fixed_cells[:, 2 + j] = np.array([(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
        self.copy_cells = np.array([[perm[a[0]], a[1], perm[b[0]], b[1]] for a, b in copies] or np.zeros((0, 4)), dtype=np.uint32)

    def fixed_array(self):
        out = np.zeros((self.cs.num_fixed, self.n, 4), dtype=np.uint64)
        f = self.fixed_cells
        if len(f):
            out[f[:, 0].astype(np.int64), f[:, 1].astype(np.int64)] = f[:, 2:]
        if self.table_loaded:
            out[self.cfg.arithmetic_config.table.index, :1 << 16, 0] = np.arange(1 << 16, dtype=np.uint64)
        return out

    def mapping_array(self):
        """[n_perm][n][2] uint32 as Assembly.mapping_array: each class of cells the copy constraints join becomes one cycle, in (column, row)
        order (any cycle over a class states the same constraint; halo2's own order depends on the order of the constrain_equal calls)"""
        m, n = len(self.cs.permutation), self.n
        out = np.empty((m, n, 2), dtype=np.uint32)
        out[:, :, 0] = np.arange(m, dtype=np.uint32)[:, None]
        out[:, :, 1] = np.arange(n, dtype=np.uint32)[None, :]
        if not len(self.copy_cells):
            return out
        e = self.copy_cells.astype(np.int64)
        nodes, inv = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 2] * n + e[:, 3]]), return_inverse=True)      # a cell = column * n + row: (column, row) order
        a, b = inv[:len(e)], inv[len(e):]
        label = np.arange(len(nodes))
        while True:                                                  # the smallest cell of each class, by propagation over the edges and pointer jumping
            low = np.minimum(label[a], label[b])
            new = label.copy()
            np.minimum.at(new, a, low)
            np.minimum.at(new, b, low)
            new = new[new]
            if np.array_equal(new, label):
                break
            label = new
        order = np.lexsort((np.arange(len(nodes)), label))           # by class, then by cell
        lab = label[order]
        first = np.r_[True, lab[1:] != lab[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))
        nxt = np.r_[order[1:], order[:1]]
        last = np.r_[first[1:], True]
        nxt[last] = order[start[last]]
        src, dst = nodes[order], nodes[nxt]
        out[src // n, src % n, 0] = dst // n
        out[src // n, src % n, 1] = dst % n
        return out

    def arrays(self):
        return [np.array([self.k, self.n_inputs, self.rows_used, int(self.table_loaded), self.n_instance], dtype=np.uint64), self.fixed_cells, self.copy_cells]


class Artifact:
    """layout + tape of one recorded circuit, persisted with a digest over both (as the plonky2 side's artifacts are)"""

    def __init__(self, layout, tape):
        self.layout, self.tape = layout, np.ascontiguousarray(tape, dtype=np.uint64)

    def digest(self):
        h = hashlib.sha256()
        for a in self.layout.arrays() + [self.tape]:
            h.update(np.ascontiguousarray(a).tobytes())
            h.update(b"|")
        return h.hexdigest()

    def save(self, path):
        head, fixed, copies = self.layout.arrays()
        buf = io.BytesIO()
        np.savez(buf, head=head, fixed=fixed, copies=copies, tape=self.tape, digest=np.frombuffer(bytes.fromhex(self.digest()), dtype=np.uint8))
        with open(path, "wb") as f:
            f.write(buf.getvalue())

    @classmethod
    def load(cls, path):
        try:
            z = np.load(path, allow_pickle=False)
            head, fixed, copies, tape, digest = z["head"], z["fixed"], z["copies"], z["tape"], z["digest"]
        except Exception as e:
            raise ValueError("not a Halo2 layout artifact: %s" % e)
        lay = Layout.__new__(Layout)
        lay.k, lay.n_inputs, lay.rows_used, lay.table_loaded, lay.n_instance = int(head[0]), int(head[1]), int(head[2]), bool(head[3]), int(head[4])
        lay.n = 1 << lay.k
        lay.cs = h2.ConstraintSystem()
        lay.cfg = hc.AllChipConfig.configure(lay.cs)
        lay.fixed_cells, lay.copy_cells = fixed.astype(np.uint64), copies.astype(np.uint32)
        art = cls(lay, tape)
        if art.digest() != bytes(digest).hex():
            raise ValueError("the artifact's digest does not match its contents")
        return art


# ---- the interpreters -------------------------------------------------------------------------------------------------------------------
def synthesize_host(tape, k, inputs):
    """gl355_halo2_synthesize_host -> (advice [19][2^k][4], (first failing entry, failing entries)); needs no device"""
    from . import _lib
    lib = _lib.load()
    tape = np.ascontiguousarray(tape, dtype=np.uint64)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
    advice = np.empty((N_ADVICE, 1 << k, 4), dtype=np.uint64)
    status = np.zeros(2, dtype=np.uint64)
    rc = lib.gl355_halo2_synthesize_host(tape.ctypes.data, tape.size, inputs.size, k, N_ADVICE, inputs.ctypes.data if inputs.size else None, advice.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise _lib.Gl355Error(rc, "gl355_halo2_synthesize_host: the tape is not valid")
    return advice, (int(status[0]), int(status[1]))


class DeviceTape:
    """a tape validated and resident on one context (gl355_halo2_tape_load)"""

    def __init__(self, ctx, tape, k, n_inputs):
        import ctypes as C
        self.ctx, self.k, self.n_inputs = ctx, k, n_inputs
        tape = np.ascontiguousarray(tape, dtype=np.uint64)
        self.h = C.c_void_p()
        ctx.check(ctx.lib.gl355_halo2_tape_load(ctx.h, tape.ctypes.data, tape.size, n_inputs, k, N_ADVICE, C.byref(self.h)))

    def synthesize(self, inputs, out=None):
        """inputs: numpy words or a device pointer (int).  out: None (a new host array), a host array, or a device pointer (int) of
        19 * 2^k * 32 bytes, which then holds the columns for PlonkProver.prove / MockProver.check.  -> (out, (first failing entry, count))"""
        ctx = self.ctx
        if not isinstance(inputs, int):
            inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
            assert inputs.size == self.n_inputs
        if out is None:
            out = np.empty((N_ADVICE, 1 << self.k, 4), dtype=np.uint64)
        status = np.zeros(2, dtype=np.uint64)
        ptr = lambda a: a if isinstance(a, int) else (a.ctypes.data if a.size else None)      # noqa: E731
        ctx.check(ctx.lib.gl355_halo2_synthesize(ctx.h, self.h, ptr(inputs), ptr(out), status.ctypes.data))
        return out, (int(status[0]), int(status[1]))

    def launches(self):
        """-> {run_max, levels_in_runs, runs, launches}: what one synthesize() launches, from the list the library walks (gl355_halo2_tape_launches)"""
        out = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.gl355_halo2_tape_launches(self.h, out.ctypes.data))
        return dict(zip(("run_max", "levels_in_runs", "runs", "launches"), (int(v) for v in out)))

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.gl355_halo2_tape_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- ArithmeticChip ---------------------------------------------------------------------------------------------------------------------
class AssignedArithmetic:
    def __init__(self, a, b, c, r):
        self.a, self.b, self.c, self.r = a, b, c, r


def _limbs(v, count):
    return [(v >> (16 * i)) & 0xFFFF for i in range(count)]


class ArithmeticChip:
    def __init__(self, ctx):
        self.ctx, self.cfg = ctx, ctx.ar

    def _q_and_r(self, row, q, r):                                   # assign_q_and_r, arithmetic_chip.rs:511-534
        ctx, cfg = self.ctx, self.cfg
        for col, limb in zip(cfg.q_limbs, _limbs(q, hc.Q_LIMBS)):
            ctx.set(col.index, row, limb)
        for col, limb in zip(cfg.r_limbs, _limbs(r, 4)):
            ctx.set(col.index, row, limb)
        ctx.set(cfg.q.index, row, q)
        ctx.set(cfg.r.index, row, r)

    def expose_public(self, cell, row):                              # :204-211
        ctx = self.ctx
        while len(ctx.instance) <= row:
            ctx.instance.append(0)
        ctx.instance[row] = cell.value
        ctx.copy(cell, (self.cfg.instance, row))

    def assert_equal(self, a, b):                                    # :213-221; on the tape: fails when the values differ (an invalid proof)
        self.ctx.copy(a, b)
        self.ctx.emit(OP_ASSERT_EQ, 0, [a.word(), b.word()], 1 + max(a.level, b.level), failed=a.value != b.value)

    def assert_equal_ext(self, a, b):                                # :223-233
        for x, y in zip(a, b):
            self.assert_equal(x, y)

    def assign_constant(self, constant):                             # :236-253
        ctx, cfg = self.ctx, self.cfg
        constant %= R
        if constant in ctx.constants:
            return ctx.constants[constant]
        row = ctx.offset
        ctx.set(cfg.a.index, row, constant)
        ctx.fixed[(cfg.constant.index, row)] = constant
        ctx.emit(OP_CONST, row, [(constant >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)], 1)
        ctx.next()
        cell = Cell(cfg.a.index, row, constant, 1)
        ctx.copy(cell, (cfg.constant, row))
        ctx.constants[constant] = cell
        return cell

    def assign_value(self, unassigned):                              # :256-268; unassigned: Input, InvExtOf or a Cell whose value is taken
        ctx, cfg = self.ctx, self.cfg
        word, r, level = ctx.term(unassigned)
        words = [word, unassigned.cell1.word()] if isinstance(unassigned, InvExtOf) else [word]
        row = ctx.offset
        ctx.enable(cfg.s_limb)
        ctx.enable(cfg.s_range)
        self._q_and_r(row, (P - r) % R, r)
        ctx.emit(OP_VALUE, row, words, level + 1, failed=r >= P)
        ctx.next()
        return Cell(cfg.r.index, row, r, level + 1)

    def range_check(self, x):                                        # :271-279
        self.assert_equal(x, self.assign_value(x))

    def _copy_terms(self, terms, cells):
        for t, cell in zip(terms, cells):
            if isinstance(t, Cell):
                self.ctx.copy(t, cell)

    def apply(self, a, b, c):                                        # assign + apply, :281-308, :351-379
        ctx, cfg = self.ctx, self.cfg
        assert not any(isinstance(t, InvExtOf) for t in (a, b, c)), "an InvExtOf is a term of assign_value only"
        terms = [ctx.term(t) for t in (a, b, c)]
        vals = [t[1] for t in terms]
        assert all(v < (1 << 64) for v in vals), "a Goldilocks row takes values below 2^64"
        level = 1 + max(t[2] for t in terms)
        row = ctx.offset
        ctx.enable(cfg.s_base)
        ctx.enable(cfg.s_limb)
        q, r = divmod(vals[0] * vals[1] + vals[2], P)
        self._q_and_r(row, q, r)
        cells = [Cell(col.index, row, v, level) for col, v in zip((cfg.a, cfg.b, cfg.c), vals)]
        for cell in cells:
            ctx.set(cell.col, row, cell.value)
        ctx.emit(OP_MULADD, row, [t[0] for t in terms], level)
        ctx.next()
        self._copy_terms((a, b, c), cells)
        return AssignedArithmetic(cells[0], cells[1], cells[2], Cell(cfg.r.index, row, r, level))

    def apply_ext(self, a, b, c):                                    # assign_ext + apply_ext, :310-349, :381-411; a b c: pairs of terms
        ctx, cfg = self.ctx, self.cfg
        flat = [a[0], a[1], b[0], b[1], c[0], c[1]]
        terms = [ctx.term(t) for t in flat]
        a0, a1, b0, b1, c0, c1 = (t[1] for t in terms)
        assert all(t[1] < (1 << 64) for t in terms)
        level = 1 + max(t[2] for t in terms)
        row = ctx.offset
        out = []
        for i, (tmp, va, vb, vc) in enumerate(((a0 * b0 + 7 * a1 * b1 + c0, a0, b0, c0), (a0 * b1 + a1 * b0 + c1, a1, b1, c1))):
            if i == 0:
                ctx.enable(cfg.s_ext)                                 # the extension gate reads this row and the next
            ctx.enable(cfg.s_limb)
            q, r = divmod(tmp, P)
            self._q_and_r(row + i, q, r)
            cells = [Cell(col.index, row + i, v, level) for col, v in zip((cfg.a, cfg.b, cfg.c), (va, vb, vc))]
            for cell in cells:
                ctx.set(cell.col, row + i, cell.value)
            out.append(cells + [Cell(cfg.r.index, row + i, r, level)])
            if i == 0:
                ctx.emit(OP_MULADD_EXT, row, [t[0] for t in terms], level)
            ctx.next()
        self._copy_terms(flat, [out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2]])
        return AssignedArithmetic(*[[out[0][j], out[1][j]] for j in range(4)])

    def _no_mod_rows(self, row, xs, coeff, level):
        """inner_product_no_mod's rows (:414-451) on rows row ..: a = x_i, b = coeff_i, c = the sum so far, q = 0, r = the new sum"""
        ctx, cfg = self.ctx, self.cfg
        zero = self.assign_constant(0)
        acc = zero
        for i, (x, co) in enumerate(zip(xs, coeff)):
            ctx.enable(cfg.s_base, row + i)
            r = (x.value * co.value + acc.value) % R
            for col, v in ((cfg.a, x.value), (cfg.b, co.value), (cfg.c, acc.value), (cfg.q, 0), (cfg.r, r)):
                ctx.set(col.index, row + i, v)
            for src, col in ((x, cfg.a), (co, cfg.b), (acc, cfg.c), (zero, cfg.q)):
                ctx.copy(src, (col, row + i))
            acc = Cell(cfg.r.index, row + i, r, level)
        return acc

    def pack(self, x):                                               # :454-463
        ctx = self.ctx
        assert len(x) == 3 and all(c.value < (1 << 64) for c in x)
        coeff = [self.assign_constant(P ** i) for i in range(3)]
        self.assign_constant(0)
        level = 1 + max(c.level for c in x)
        row = ctx.offset
        ctx.emit(OP_PACK, row, [c.word() for c in x], level)
        acc = self._no_mod_rows(row, x, coeff, level)
        ctx.next(3)
        return acc

    def unpack(self, x):                                             # :466-486
        ctx, cfg = self.ctx, self.cfg
        coeff = [self.assign_constant(P ** i) for i in range(4)]
        self.assign_constant(0)
        level = 1 + x.level
        row = ctx.offset
        digits, v = [], x.value
        for _ in range(4):                                           # goldilocks_decompose, utils.rs:25-36
            v, d = divmod(v, P)
            digits.append(d)
        cells = []
        for i, d in enumerate(digits):
            ctx.enable(cfg.s_limb, row + i)
            ctx.enable(cfg.s_range, row + i)
            self._q_and_r(row + i, P - d, d)
            cells.append(Cell(cfg.r.index, row + i, d, level))
        ctx.emit(OP_UNPACK, row, [x.word()], level, failed=False)    # four base-p digits always recompose a value below r < p^4
        expected = self._no_mod_rows(row + 4, cells, coeff, level)
        ctx.next(8)
        ctx.copy(x, expected)
        return cells[:3]

    def load_table(self):                                            # :488-507
        self.ctx.table_loaded = True


# ---- AllChip ----------------------------------------------------------------------------------------------------------------------------
class AllChip:
    def __init__(self, ctx):
        self.ctx = ctx
        self.arithmetic_chip = ArithmeticChip(ctx)

    def apply_permute(self, state):                                  # PoseidonBn254Chip::apply_permute, poseidon_bn254_chip.rs:203-233
        ctx, cfg = self.ctx, self.ctx.po
        row0 = ctx.offset
        level = 1 + max(c.level for c in state)
        ctx.emit(OP_PERMUTE, row0, [c.word() for c in state], level)
        s = [c.value for c in state]
        for i, c in enumerate(state):
            ctx.copy(c, (cfg.state[i], row0))
        assert hc.T == 5
        last = row0 + hc.R_F + hc.R_P
        state_cols, constant_cols = [c.index for c in cfg.state], [c.index for c in cfg.constants]
        values, fixed, rc, mds = ctx.values, ctx.fixed, cfg.rc, cfg.mds
        assert not any((col, row) in values for col in state_cols for row in (row0, last)), "the permutation's rows are assigned already"
        for rnd in range(hc.R_F + hc.R_P):
            row = row0 + rnd
            full = rnd < hc.R_F // 2 or rnd >= hc.R_F // 2 + hc.R_P
            c = rc[rnd * 5:rnd * 5 + 5]
            for i in range(5):
                values[(state_cols[i], row)] = s[i]
                fixed[(constant_cols[i], row)] = c[i]
            ctx.enable(cfg.q_f if full else cfg.q_p, row)
            t0, t1, t2, t3, t4 = (s[0] + c[0]) % R, (s[1] + c[1]) % R, (s[2] + c[2]) % R, (s[3] + c[3]) % R, (s[4] + c[4]) % R
            t0 = pow(t0, 5, R)
            if full:
                t1, t2, t3, t4 = pow(t1, 5, R), pow(t2, 5, R), pow(t3, 5, R), pow(t4, 5, R)
            s = [(m[0] * t0 + m[1] * t1 + m[2] * t2 + m[3] * t3 + m[4] * t4) % R for m in mds]
        for i in range(5):
            values[(state_cols[i], last)] = s[i]
        ctx.set_offset(last)
        ctx.next()
        return [Cell(cfg.state[i].index, last, s[i], level) for i in range(hc.T)]

    def permute(self, state):                                        # all_chip.rs:52-89
        ctx, ar = self.ctx, self.arithmetic_chip
        assert len(state) == 12
        zero = ar.assign_constant(0)
        offset_start = ctx.offset
        encoded = [ar.pack(state[i:i + 3]) for i in range(0, 12, 3)]
        encoded.append(zero)
        offset_end_compose = ctx.offset
        ctx.set_offset(offset_start)
        out = self.apply_permute(encoded)
        offset_end_permute = ctx.offset
        ctx.set_offset(offset_end_compose)
        decoded = [d for x in out[:4] for d in ar.unpack(x)]
        ctx.set_offset(max(ctx.offset, offset_end_permute))
        return decoded

    def load_table(self):
        self.arithmetic_chip.load_table()


# ---- GoldilocksChip ---------------------------------------------------------------------------------------------------------------------
class GoldilocksChip:
    def __init__(self, ctx):
        self.ctx = ctx
        self.all_chip = AllChip(ctx)
        self.arithmetic_chip = self.all_chip.arithmetic_chip

    def assign_value(self, unassigned):                              # goldilocks_chip.rs:68-74
        return self.arithmetic_chip.assign_value(unassigned)

    def assign_constant(self, constant):                             # :76-83
        return self.arithmetic_chip.assign_constant(constant % P)

    def compose(self, terms, constant):                              # :85-103; terms: (coefficient cell, base constant)
        acc = self.assign_constant(constant)
        for coeff, base in terms:
            acc = self.mul_const_add(coeff, base, acc)
        return acc

    def add(self, lhs, rhs):                                         # :105-119
        one = self.assign_constant(1)
        return self.arithmetic_chip.apply(lhs, one, rhs).r

    def sub(self, lhs, rhs):                                         # :121-135
        neg_one = self.assign_constant(P - 1)
        return self.arithmetic_chip.apply(rhs, neg_one, lhs).r

    def mul(self, lhs, rhs):                                         # :137-144
        return self.mul_add_constant(lhs, rhs, 0)

    def mul_with_constant(self, lhs, rhs, constant):                 # :146-156
        constant = self.assign_constant(constant)
        return self.mul(self.mul(lhs, rhs), constant)

    def mul_add_constant(self, a, b, to_add):                        # :158-173
        to_add = self.assign_constant(to_add)
        return self.arithmetic_chip.apply(a, b, to_add).r

    def mul_add(self, a, b, c):                                      # :175-189
        return self.arithmetic_chip.apply(a, b, c).r

    def mul_const_add(self, a, constant, b):                         # :191-206
        constant = self.assign_constant(constant)
        return self.arithmetic_chip.apply(a, constant, b).r

    def add_constant(self, a, constant):                             # :208-216
        one = self.assign_constant(1)
        return self.mul_add_constant(a, one, constant)

    def assert_equal(self, lhs, rhs):                                # :218-225
        self.arithmetic_chip.assert_equal(lhs, rhs)

    def assert_one(self, a):                                         # :227-234
        self.assert_equal(a, self.assign_constant(1))

    def assert_zero(self, a):                                        # :236-243
        self.assert_equal(a, self.assign_constant(0))

    def assign_bit(self, bit):                                       # :245-264; bit: BitOf
        one, zero, neg_one = self.assign_constant(1), self.assign_constant(0), self.assign_constant(P - 1)
        assigned = self.arithmetic_chip.apply(bit, one, neg_one)
        b, b_minus_one = assigned.a, assigned.r
        should_zero = self.mul(b, b_minus_one)
        self.assert_equal(should_zero, zero)
        return b

    def select(self, a, b, cond):                                    # :266-276: (a - b) cond + b
        return self.mul_add(self.sub(a, b), cond, b)

    def is_zero(self, a):                                            # :279-306
        zero = self.assign_constant(0)
        assigned = self.arithmetic_chip.apply(a, InvOf(a), zero)
        a_a_inv, zero = assigned.r, assigned.c
        one = self.assign_constant(1)
        out = self.sub(one, a_a_inv)
        out_a = self.mul(out, a)
        self.assert_equal(out_a, zero)
        return out

    def to_bits(self, composed, number_of_bits):                     # :310-350: always all 64 bits, the first number_of_bits returned
        zero = self.assign_constant(0)
        bits = [self.assign_bit(BitOf(composed, i)) for i in range(64)]
        acc = zero
        for i, bit in enumerate(bits):
            c = self.assign_constant(1 << i)
            acc = self.arithmetic_chip.apply(bit, c, acc).r
        self.assert_equal(acc, composed)
        return bits[:number_of_bits]

    def from_bits(self, bits):                                       # :352-373
        acc = self.assign_constant(0)
        for i, bit in enumerate(bits):
            c = self.assign_constant(1 << i)
            acc = self.arithmetic_chip.apply(bit, c, acc).r
        return acc

    def exp_power_of_2(self, a, power_log):                          # :375-386
        result = a
        for _ in range(power_log):
            result = self.mul(result, result)
        return result

    def exp_from_bits(self, base, power_bits):                       # :388-404
        x = self.assign_constant(1)
        one = self.assign_constant(1)
        for i, bit in enumerate(power_bits):
            is_zero_bit = self.is_zero(bit)
            b = self.assign_constant(pow(base, 1 << i, P))
            x = self.mul(x, self.select(one, b, is_zero_bit))
        return x

    def is_equal(self, a, b):                                        # :406-414
        return self.is_zero(self.sub(a, b))

    def load_table(self):                                            # :416-421
        self.arithmetic_chip.load_table()


# ---- HasherChip -------------------------------------------------------------------------------------------------------------------------
RATE = 8


class HasherChip:
    def __init__(self, ctx):                                         # hasher_chip.rs:30-47
        self.ctx = ctx
        self.goldilocks_chip = GoldilocksChip(ctx)
        self.state = [self.goldilocks_chip.assign_constant(0) for _ in range(12)]
        self.absorbing, self.output_buffer = [], []

    def update(self, element):                                       # :51-59
        self.output_buffer = []
        self.absorbing.append(element)

    def _absorb_buffered_inputs(self):                               # :61-71
        buffered, self.absorbing = self.absorbing, []
        for off in range(0, len(buffered), RATE):
            self._duplexing(buffered[off:off + RATE])

    def squeeze(self, num_outputs):                                  # :73-89
        output = []
        for _ in range(num_outputs):
            self._absorb_buffered_inputs()
            if not self.output_buffer:
                self.permutation()
                self.output_buffer = list(self.state[:RATE])
            output.append(self.output_buffer.pop())
        return output

    def permutation(self):                                           # :101-105
        self.state = self.goldilocks_chip.all_chip.permute(self.state)

    def _duplexing(self, inputs):                                    # :107-120
        self.state[:len(inputs)] = inputs
        self.permutation()
        self.output_buffer = list(self.state[:RATE])

    def _outputs(self, num_outputs):
        outputs = []
        while True:
            for item in self.state[:RATE]:
                outputs.append(item)
                if len(outputs) == num_outputs:
                    return outputs
            self.permutation()

    def hash(self, inputs, num_outputs):                             # :122-148
        self.absorbing = []
        for off in range(0, len(inputs), RATE):
            chunk = inputs[off:off + RATE]
            self.state[:len(chunk)] = chunk
            self.permutation()
        return self._outputs(num_outputs)

    def permute(self, inputs, num_output):                           # :150-171
        self.state[:len(inputs)] = inputs
        self.permutation()
        return self._outputs(num_output)


# ---- VectorChip, MerkleProofChip -----------------------------------------------------------------------------------------------------------
class VectorChip:
    def __init__(self, ctx, vector):
        self.main_gate, self.vector = GoldilocksChip(ctx), vector

    def access(self, index):                                         # vector_chip.rs:26-48
        g = self.main_gate
        not_exists = g.assign_constant(1)
        zero = g.assign_constant(0)
        element = zero
        for i, v in enumerate(self.vector):
            assigned_i = g.assign_constant(i)
            i_minus_index = g.sub(assigned_i, index)
            not_exists = g.mul(not_exists, i_minus_index)
            is_same_index = g.is_equal(i_minus_index, zero)
            element = g.select(v, element, is_same_index)
        g.assert_zero(not_exists)
        return element


class MerkleProofChip:
    def __init__(self, ctx):
        self.ctx, self.goldilocks_chip = ctx, GoldilocksChip(ctx)

    def verify_merkle_proof_to_cap_with_cap_index(self, leaf_data, leaf_index_bits, cap_index, merkle_cap, siblings):
        """merkle_proof_chip.rs:39-87.  merkle_cap: a list of hashes (4 cells each); siblings: a list of hashes"""
        g = self.goldilocks_chip
        hasher = HasherChip(self.ctx)
        state = list(leaf_data) if len(leaf_data) <= 4 else hasher.hash(list(leaf_data), 4)
        for bit, sibling in zip(leaf_index_bits, siblings):
            hasher = HasherChip(self.ctx)
            inputs = [g.select(sibling[i], state[i], bit) for i in range(4)]
            inputs += [g.select(state[i], sibling[i], bit) for i in range(4)]
            state = hasher.permute(inputs, 4)
        for i in range(4):
            cap_i = VectorChip(self.ctx, [h[i] for h in merkle_cap]).access(cap_index)
            g.assert_equal(cap_i, state[i])


# ---- GoldilocksExtensionChip ---------------------------------------------------------------------------------------------------------------
class GoldilocksExtensionChip:
    """goldilocks_extension_chip.rs:56-416; an extension element is a list of two cells.  The wasteful forms are the reference's (a subtraction
    multiplies by one, exp multiplies `power` times): the layout is the reference's"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.goldilocks_chip = GoldilocksChip(ctx)
        self.arithmetic_chip = self.goldilocks_chip.arithmetic_chip

    def mul_add_extension(self, a, b, c):                            # :56-70
        return self.arithmetic_chip.apply_ext(a, b, c).r

    def div_extension(self, x, y):                                   # :72-106; y = (0, 0) fails the assert_one below instead of the Rust's assert!
        g = self.goldilocks_chip
        y_inv = [g.assign_value(InvExtOf(y[0], y[1], 0)), g.assign_value(InvExtOf(y[0], y[1], 1))]
        yy_inv = self.mul_extension(y, y_inv)
        self.assert_one_extension(yy_inv)
        return self.mul_extension(x, y_inv)

    def div_add_extension(self, x, y, z):                            # :108-117
        return self.add_extension(self.div_extension(x, y), z)

    def add_extension(self, addend_0, addend_1):                     # :119-133
        g = self.goldilocks_chip
        return [g.add(a, b) for a, b in zip(addend_0, addend_1)]

    def scalar_mul(self, multiplicand, scalar):                      # :135-149
        g = self.goldilocks_chip
        assigned_scalar = g.assign_constant(scalar)
        return [g.mul(v, assigned_scalar) for v in multiplicand]

    def arithmetic_extension(self, const_0, const_1, multiplicand_0, multiplicand_1, addend):      # :151-168
        term_1 = self.mul_extension(multiplicand_0, multiplicand_1)
        term_1 = self.scalar_mul(term_1, const_0)
        term_2 = self.scalar_mul(addend, const_1)
        return self.add_extension(term_1, term_2)

    def zero_extension(self):                                        # :170-179
        g = self.goldilocks_chip
        return [g.assign_constant(0) for _ in range(2)]

    def one_extension(self):                                         # :181-191
        g = self.goldilocks_chip
        return [g.assign_constant(1), g.assign_constant(0)]

    def two_extension(self):                                         # :193-203
        g = self.goldilocks_chip
        return [g.assign_constant(2), g.assign_constant(0)]

    def mul_extension_with_const(self, const_0, multiplicand_0, multiplicand_1):      # :205-221
        zero = self.zero_extension()
        return self.arithmetic_extension(const_0, 0, multiplicand_0, multiplicand_1, zero)

    def mul_extension(self, multiplicand_0, multiplicand_1):         # :223-231
        zero = self.zero_extension()
        return self.mul_add_extension(multiplicand_0, multiplicand_1, zero)

    def mul_sub_extension(self, a, b, c):                            # :233-242
        return self.arithmetic_extension(1, P - 1, a, b, c)

    def square_extension(self, x):                                   # :244-250
        return self.mul_extension(x, x)

    def exp_power_of_2_extension(self, base, power_log):             # :252-262
        for _ in range(power_log):
            base = self.square_extension(base)
        return base

    def exp(self, base, power):                                      # :264-281
        if power == 0:
            return self.one_extension()
        if power == 1:
            return list(base)
        if power == 2:
            return self.square_extension(base)
        product = self.one_extension()
        for _ in range(power):
            product = self.mul_extension(product, base)
        return product

    def mul_many_extension(self, terms):                             # :283-293
        result = self.one_extension()
        for term in terms:
            result = self.mul_extension(result, term)
        return result

    def sub_extension(self, lhs, rhs):                               # :295-304
        one_extension = self.one_extension()
        return self.arithmetic_extension(1, P - 1, lhs, one_extension, rhs)

    def constant_extension(self, constant):                          # :306-317
        g = self.goldilocks_chip
        return [g.assign_constant(c) for c in constant]

    def convert_to_extension(self, value):                           # :319-329
        return [value, self.goldilocks_chip.assign_constant(0)]

    def reduce_extension(self, base, terms):                         # :331-342
        result = self.zero_extension()
        for term in reversed(terms):
            result = self.mul_add_extension(result, base, term)
        return result

    def reduce_base_field_terms_extension(self, base, terms):        # :344-355
        terms = [self.convert_to_extension(t) for t in terms]
        return self.reduce_extension(base, terms)

    def reduce_extension_field_terms_base(self, base, terms):        # :357-365
        base = self.convert_to_extension(base)
        return self.reduce_extension(base, terms)

    def shift(self, factor, power, shifted):                         # :367-377: shifted * factor^power
        exp = self.exp(factor, power)
        return self.mul_extension(exp, shifted)

    def assert_equal_extension(self, lhs, rhs):                      # :379-389
        g = self.goldilocks_chip
        g.assert_equal(lhs[0], rhs[0])
        g.assert_equal(lhs[1], rhs[1])

    def assert_one_extension(self, a):                               # :391-400
        g = self.goldilocks_chip
        g.assert_one(a[0])
        g.assert_zero(a[1])

    def select(self, cond, a, b):                                    # :402-416: cond (a - b) + b
        a_minus_b = self.sub_extension(a, b)
        return self.arithmetic_extension(1, 1, cond, a_minus_b, b)


# ---- TranscriptChip -------------------------------------------------------------------------------------------------------------------------
class TranscriptChip:
    def __init__(self, ctx):                                         # transcript_chip.rs:17-23
        self.hasher_chip = HasherChip(ctx)

    def write_scalar(self, scalar):                                  # :26-32
        self.hasher_chip.update(scalar)

    def write_extension(self, extension):                            # :34-43
        for scalar in extension:
            self.write_scalar(scalar)

    def write_hash(self, hash_):                                     # :45-54
        for scalar in hash_:
            self.write_scalar(scalar)

    def write_cap(self, cap):                                        # :56-65
        for hash_ in cap:
            self.write_hash(hash_)

    def squeeze(self, num_outputs):                                  # :68-74
        return self.hasher_chip.squeeze(num_outputs)


# ---- FriVerifierChip ------------------------------------------------------------------------------------------------------------------------
GENERATOR = 7                                                        # GoldilocksField::MULTIPLICATIVE_GROUP_GENERATOR


def primitive_root_of_unity(bits):
    """MULTIPLICATIVE_GROUP_GENERATOR.exp_u64(NEG_ONE / 2^bits), as fri_chip.rs:162-163 and :182-183 derive their roots"""
    return pow(GENERATOR, (P - 1) >> bits, P)


class FriInstanceInfo:
    """types/fri.rs:49-72 with common_data's fri_oracles / fri_all_polys / fri_zs_polys: four oracles (constants and sigmas unblinded), every
    polynomial opened at zeta, the Zs also at g zeta.  widths: the polynomials of each oracle"""

    def __init__(self, zeta, zeta_next, widths, num_challenges):
        self.oracles_blinding = [False, True, True, True]
        self.batches = [(zeta, [(o, i) for o in range(4) for i in range(widths[o])]), (zeta_next, [(2, i) for i in range(num_challenges)])]


class FriVerifierChip:
    """fri_chip.rs:34-376.  A proof's parts come as cells: fri_proof = dict(commit_phase_merkle_caps, query_round_proofs, final_poly) with a
    round = dict(initial_trees=[(evals, siblings)], steps=[(evals as extension elements, siblings)]); a cap is a list of 4-cell hashes"""

    def __init__(self, ctx, offset, lde_bits, cap_height, reduction_arity_bits, hiding, proof_of_work_bits):      # construct, :35-46
        self.ctx, self.offset = ctx, offset
        if any(int(a) != 1 for a in reduction_arity_bits):      # next_eval is the reference's: two points per layer (:211)
            raise ValueError("FriVerifierChip supports arity-2 FRI only (reduction_arity_bits = 1), not %r" % (list(reduction_arity_bits),))
        self.lde_bits, self.cap_height, self.reduction_arity_bits = lde_bits, cap_height, list(reduction_arity_bits)
        self.hiding, self.proof_of_work_bits = hiding, proof_of_work_bits
        self.goldilocks_chip = GoldilocksChip(ctx)
        self.goldilocks_extension_chip = GoldilocksExtensionChip(ctx)
        self.round_rows = []

    def compute_reduced_openings(self, fri_alpha, fri_openings):     # :58-70; fri_openings: the batches' values
        return [self.goldilocks_extension_chip.reduce_extension(fri_alpha, values) for values in fri_openings]

    def calculate_cap_index(self, x_index_bits):                     # :72-82
        return self.goldilocks_chip.from_bits(x_index_bits[len(x_index_bits) - self.cap_height:])

    def verify_initial_merkle_proof(self, x_index_bits, cap_index, initial_merkle_caps, initial_trees_proof):      # :85-110
        merkle_proof_chip = MerkleProofChip(self.ctx)
        for (evals, merkle_proof), cap in zip(initial_trees_proof, initial_merkle_caps):
            merkle_proof_chip.verify_merkle_proof_to_cap_with_cap_index(evals, x_index_bits, cap_index, cap, merkle_proof)

    @staticmethod
    def unsalted_eval(initial_trees_proof, oracle_index, poly_index, salted):      # types/assigned.rs:58-71
        evals = initial_trees_proof[oracle_index][0]
        return evals[:len(evals) - (4 if salted else 0)][poly_index]

    def batch_initial_polynomials(self, fri_instance_info, fri_alpha, x, initial_trees_proof, reduced_openings):      # :112-149
        ge = self.goldilocks_extension_chip
        x = ge.convert_to_extension(x)
        total = ge.zero_extension()
        for (point, polynomials), reduced in zip(fri_instance_info.batches, reduced_openings):
            evals = [self.unsalted_eval(initial_trees_proof, o, i, self.hiding and fri_instance_info.oracles_blinding[o]) for o, i in polynomials]
            reduced_evals = ge.reduce_base_field_terms_extension(fri_alpha, evals)
            numerator = ge.sub_extension(reduced_evals, reduced)
            denominator = ge.sub_extension(x, point)
            total = ge.shift(fri_alpha, len(evals), total)
            total = ge.div_add_extension(numerator, denominator, total)
        return total

    def x_from_subgroup(self, x_index_bits):                         # :151-166
        return self.goldilocks_chip.exp_from_bits(primitive_root_of_unity(self.lde_bits), x_index_bits)

    def next_eval(self, x_index_within_coset_bits, x, evals, arity_bits, beta):      # :168-226
        g_chip, ge = self.goldilocks_chip, self.goldilocks_extension_chip
        assert arity_bits == 1, "only arity 2 is supported, as in the reference (:211)"
        g = primitive_root_of_unity(arity_bits)
        g_inv = pow(g, P - 2, P)
        g = g_chip.assign_constant(g)
        evals = list(evals)                                          # reverse_index_bits_in_place: the identity on two elements
        start = g_chip.exp_from_bits(g_inv, list(reversed(x_index_within_coset_bits)))
        coset_start = g_chip.mul(start, x)
        g_power = g_chip.assign_constant(1)
        points = []
        for ev in evals:
            xi = g_chip.mul(coset_start, g_power)
            xi = ge.convert_to_extension(xi)
            g_power = g_chip.mul(g_power, g)
            points.append((xi, ev))
        (a0, a1), (b0, b1) = points                                  # a1 + (beta - a0) (b1 - a1) / (b0 - a0)
        x_minus_a0 = ge.sub_extension(beta, a0)
        b1_minus_a1 = ge.sub_extension(b1, a1)
        numerator = ge.mul_extension(x_minus_a0, b1_minus_a1)
        denominator = ge.sub_extension(b0, a0)
        return ge.div_add_extension(numerator, denominator, a1)

    def check_consistency(self, initial_merkle_caps, fri_instance_info, fri_alpha, fri_betas, fri_proof, x_index, round_proof, reduced_openings):      # :228-327
        g_chip, ge = self.goldilocks_chip, self.goldilocks_extension_chip
        x_index_bits = g_chip.to_bits(x_index, 64)[:self.lde_bits]
        cap_index = self.calculate_cap_index(x_index_bits)
        self.verify_initial_merkle_proof(x_index_bits, cap_index, initial_merkle_caps, round_proof["initial_trees"])
        x_from_subgroup = self.x_from_subgroup(list(reversed(x_index_bits)))
        x_from_subgroup = g_chip.mul(self.offset, x_from_subgroup)
        prev_eval = self.batch_initial_polynomials(fri_instance_info, fri_alpha, x_from_subgroup, round_proof["initial_trees"], reduced_openings)
        for i, arity_bits in enumerate(self.reduction_arity_bits):
            evals, siblings = round_proof["steps"][i]
            coset_index_bits = x_index_bits[arity_bits:]
            x_index_within_coset_bits = x_index_bits[:arity_bits]
            x_index_within_coset = g_chip.from_bits(x_index_within_coset_bits)
            for j in range(2):
                next_eval_j = VectorChip(self.ctx, [ev[j] for ev in evals]).access(x_index_within_coset)
                g_chip.assert_equal(prev_eval[j], next_eval_j)
            prev_eval = self.next_eval(x_index_within_coset_bits, x_from_subgroup, evals, arity_bits, fri_betas[i])
            MerkleProofChip(self.ctx).verify_merkle_proof_to_cap_with_cap_index([c for ev in evals for c in ev], coset_index_bits, cap_index,
                                                                                fri_proof["commit_phase_merkle_caps"][i], siblings)
            x_from_subgroup = g_chip.exp_power_of_2(x_from_subgroup, arity_bits)
            x_index_bits = coset_index_bits
        final_poly_eval = ge.reduce_extension_field_terms_base(x_from_subgroup, fri_proof["final_poly"])
        ge.assert_equal_extension(prev_eval, final_poly_eval)

    def verify_fri_proof(self, initial_merkle_caps, fri_challenges, fri_openings, fri_proof, fri_instance_info):      # :329-362
        """fri_challenges: dict(fri_alpha, fri_betas, fri_pow_response, fri_query_indices).  round_rows gets one half-open row range per round"""
        self.fri_verify_proof_of_work(fri_challenges["fri_pow_response"])
        reduced_openings = self.compute_reduced_openings(fri_challenges["fri_alpha"], fri_openings)
        self.round_rows = []
        for i, round_proof in enumerate(fri_proof["query_round_proofs"]):
            start = self.ctx.offset
            self.check_consistency(initial_merkle_caps, fri_instance_info, fri_challenges["fri_alpha"], fri_challenges["fri_betas"], fri_proof,
                                   fri_challenges["fri_query_indices"][i], round_proof, reduced_openings)
            self.round_rows.append((start, self.ctx.offset))

    def fri_verify_proof_of_work(self, fri_pow_response):            # :364-376
        g_chip = self.goldilocks_chip
        bits = g_chip.to_bits(fri_pow_response, 64)
        for b in list(reversed(bits))[:self.proof_of_work_bits]:
            g_chip.assert_zero(b)
