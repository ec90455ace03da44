"""Host-side mirror of the halo2 front end the reference's SNARK finalisation goes through:
`ConstraintSystem` / `Expression` / `Rotation` / the permutation `Assembly` as `Circuit::configure` and `keygen_vk` / `keygen_pk` use
them (src/plonky2_verifier/verifier_api.rs:77-92; the reference's own gates and lookups: chip/native_chip/arithmetic_chip.rs:44-160,
poseidon_bn254_chip.rs:27-123), reduced to what the prover's data-parallel stages need: the column / query / gate / lookup /
permutation description of a circuit, compiled to the descriptor blob `gl355_plonk_keygen` takes (include/gl355.h) -- gates and
lookup expressions as small register programs.

halo2_proofs itself is an un-vendored dependency of the reference (Cargo.lock); names and semantics follow its published API
(`meta.advice_column()`, `meta.create_gate`, `meta.lookup`, `meta.enable_equality`, `Rotation::cur/next/prev`, `cs.degree()`,
`cs.blinding_factors()`).  Deviations, all on the host side of the boundary: selectors are plain fixed columns (halo2 compresses
simple selectors into fewer fixed columns at keygen), one phase, no challenges-as-expressions.
"""
import collections

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617     # bn256::Fr
S = 28
GENERATOR = 7
ROOT_OF_UNITY = pow(GENERATOR, (R - 1) >> S, R)
DELTA = pow(GENERATOR, 1 << S, R)                      # Fr::DELTA: generator of the t-order subgroup, separates the permutation's column cosets
ZETA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23        # Fr::ZETA, a primitive cube root of unity: the extended domain's coset shift
assert pow(ZETA, 3, R) == 1 and ZETA != 1

ADVICE, FIXED, INSTANCE = 0, 1, 2
KIND_NAMES = {ADVICE: "advice", FIXED: "fixed", INSTANCE: "instance"}


class Rotation(int):
    @staticmethod
    def cur():
        return Rotation(0)

    @staticmethod
    def next():
        return Rotation(1)

    @staticmethod
    def prev():
        return Rotation(-1)


class Column:
    def __init__(self, kind, index):
        self.kind, self.index = kind, index

    def __eq__(self, o):
        return isinstance(o, Column) and (self.kind, self.index) == (o.kind, o.index)

    def __hash__(self):
        return hash((self.kind, self.index))

    def __repr__(self):
        return "%s[%d]" % (KIND_NAMES[self.kind], self.index)


class Expression:
    """plonk::Expression: Constant | Query (advice / fixed / instance at a rotation) | Negated | Sum | Product | Scaled"""
    __slots__ = ("op", "a", "b")

    def __init__(self, op, a=None, b=None):
        self.op, self.a, self.b = op, a, b

    @staticmethod
    def constant(v):
        return Expression("const", int(v) % R)

    @staticmethod
    def _wrap(x):
        return x if isinstance(x, Expression) else Expression.constant(x)

    def __add__(self, o):
        return Expression("add", self, Expression._wrap(o))

    __radd__ = __add__

    def __sub__(self, o):
        return Expression("add", self, Expression("neg", Expression._wrap(o)))

    def __rsub__(self, o):
        return Expression._wrap(o) - self

    def __neg__(self):
        return Expression("neg", self)

    def __mul__(self, o):
        if isinstance(o, Expression):
            return Expression("mul", self, o)
        return Expression("scale", self, int(o) % R)

    __rmul__ = __mul__

    def degree(self):
        if self.op == "const":
            return 0
        if self.op == "query":
            return 1
        if self.op in ("neg", "scale"):
            return self.a.degree()
        if self.op == "add":
            return max(self.a.degree(), self.b.degree())
        return self.a.degree() + self.b.degree()

    def evaluate(self, query):
        """tree evaluation over Python integers; query(kind, query_index) -> value"""
        op = self.op
        if op == "const":
            return self.a
        if op == "query":
            return query(self.a, self.b)
        if op == "neg":
            return (-self.a.evaluate(query)) % R
        if op == "scale":
            return self.a.evaluate(query) * self.b % R
        if op == "add":
            return (self.a.evaluate(query) + self.b.evaluate(query)) % R
        return self.a.evaluate(query) * self.b.evaluate(query) % R


class ConstraintSystem:
    def __init__(self):
        self.num_advice = self.num_fixed = self.num_instance = 0
        self.selectors = []                      # fixed-column indices that were declared as selectors (bookkeeping only)
        self.queries = {ADVICE: [], FIXED: [], INSTANCE: []}     # per kind: [(column index, rotation)] in first-use order
        self.gates = []                          # (name, [Expression])
        self.lookups = []                        # (name, [input Expression], [table Expression])
        self.permutation = []                    # columns with equality enabled, in enable order
        self.minimum_degree = None

    # ---- columns -----------------------------------------------------------------------------------------------------
    def advice_column(self):
        self.num_advice += 1
        return Column(ADVICE, self.num_advice - 1)

    def fixed_column(self):
        self.num_fixed += 1
        return Column(FIXED, self.num_fixed - 1)

    def instance_column(self):
        self.num_instance += 1
        return Column(INSTANCE, self.num_instance - 1)

    def selector(self):
        c = self.fixed_column()
        self.selectors.append(c.index)
        return c

    def lookup_table_column(self):
        return self.fixed_column()

    def enable_equality(self, column):
        self._query(column, 0)                   # halo2: query_any_index(column, Rotation::cur()) -- the argument reads the column at x
        if column not in self.permutation:
            self.permutation.append(column)

    def enable_constant(self, column):
        self.enable_equality(column)

    # ---- queries -----------------------------------------------------------------------------------------------------
    def _query(self, column, rotation):
        q = self.queries[column.kind]
        key = (column.index, int(rotation))
        if key not in q:
            q.append(key)
        return Expression("query", column.kind, q.index(key))

    def query_advice(self, column, rotation=0):
        assert column.kind == ADVICE
        return self._query(column, rotation)

    def query_fixed(self, column, rotation=0):
        assert column.kind == FIXED
        return self._query(column, rotation)

    query_selector = query_fixed

    def query_instance(self, column, rotation=0):
        assert column.kind == INSTANCE
        return self._query(column, rotation)

    def query_any(self, column, rotation=0):
        return self._query(column, rotation)

    # ---- gates / lookups ---------------------------------------------------------------------------------------------
    def create_gate(self, name, polys):
        polys = list(polys)
        assert polys
        self.gates.append((name, polys))

    def lookup(self, name, pairs):
        pairs = list(pairs)
        ins = [p[0] for p in pairs]
        tabs = [p[1] if isinstance(p[1], Expression) else self.query_fixed(p[1]) for p in pairs]
        self.lookups.append((name, ins, tabs))

    # ---- derived shape (plonk::ConstraintSystem::degree / blinding_factors, permutation::Argument, lookup::Argument) --
    def degree(self):
        d = 3                                                           # permutation::Argument::required_degree: 3 with or without columns
        for _, ins, tabs in self.lookups:                               # lookup::Argument::required_degree
            di = max([1] + [e.degree() for e in ins])
            dt = max([1] + [e.degree() for e in tabs])
            d = max(d, 4, 2 + di + dt)
        for _, polys in self.gates:
            d = max([d] + [p.degree() for p in polys])
        return max(d, self.minimum_degree or 1)

    def blinding_factors(self):
        per_col = {}
        for col, _ in self.queries[ADVICE]:
            per_col[col] = per_col.get(col, 0) + 1
        factors = max([1] + list(per_col.values()))
        return max(3, factors) + 2

    def minimum_rows(self):
        return self.blinding_factors() + 3

    def chunk_len(self):
        return self.degree() - 2                                        # columns per permutation product polynomial

    def all_gate_polys(self):
        return [p for _, polys in self.gates for p in polys]


class Assembly:
    """permutation::keygen::Assembly: the copy-constraint cycles over the equality-enabled columns (halo2 book, "Permutation argument"):
    mapping[column][row] = the next cell of the cycle, aux = a representative of the cycle, sizes = its length (numpy arrays: a k = 23
    circuit has 10^8 cells)"""

    def __init__(self, n, columns):
        self.n, self.columns = n, list(columns)
        m = len(self.columns)
        ident = np.empty((m, n, 2), dtype=np.uint32)
        ident[:, :, 0] = np.arange(m, dtype=np.uint32)[:, None]
        ident[:, :, 1] = np.arange(n, dtype=np.uint32)[None, :]
        self.mapping = ident
        self.aux = ident.copy()
        self.sizes = np.ones((m, n), dtype=np.uint32)

    def copy(self, left_column, left_row, right_column, right_row):
        lc, rc = self.columns.index(left_column), self.columns.index(right_column)
        left, right = tuple(int(v) for v in self.aux[lc, left_row]), tuple(int(v) for v in self.aux[rc, right_row])
        if left == right:
            return
        if self.sizes[left] < self.sizes[right]:
            left, right = right, left
        self.sizes[left] += self.sizes[right]
        i = right
        while True:
            self.aux[i] = left
            i = tuple(int(v) for v in self.mapping[i])
            if i == right:
                break
        tmp = self.mapping[lc, left_row].copy()
        self.mapping[lc, left_row] = self.mapping[rc, right_row]
        self.mapping[rc, right_row] = tmp

    def mapping_array(self):
        """[n_perm][n][2] uint32: (column position in the permutation, row) each cell maps to"""
        return self.mapping


# ---- compilation of expressions to the register programs of the descriptor ------------------------------------------------------
OP_ADD, OP_SUB, OP_MUL, OP_EMIT, OP_NEG, OP_MOV = range(6)
K_REG, K_CONST, K_ADVICE, K_FIXED, K_INSTANCE = range(5)
MAX_REGS = 12
_KIND_OPERAND = {ADVICE: K_ADVICE, FIXED: K_FIXED, INSTANCE: K_INSTANCE}


class _Node:
    __slots__ = ("op", "kids", "val", "uses", "reg", "need")

    def __init__(self, op, kids, val):
        self.op, self.kids, self.val, self.uses, self.reg, self.need = op, kids, val, 0, None, 0


class ProgramBuilder:
    """Expression trees -> straight-line code over at most MAX_REGS 256-bit registers.  An instruction is four u32:
    (op, dst register, operand a, operand b), an operand = kind << 24 | index with kind in REG / CONST (pool index) / ADVICE / FIXED /
    INSTANCE (query index).  EMIT a: "this value is the next polynomial" -- the evaluator folds it into its running sum
    (sum * y + a for constraints, sum * theta + a for the expressions of a lookup).  Structurally equal subexpressions are computed
    once (halo2's GraphEvaluator does the same) and stay in their register until their last use."""

    def __init__(self, const_pool):
        self.code, self.pool, self.free, self.peak = [], const_pool, list(range(MAX_REGS - 1, -1, -1)), 0
        self.nodes, self.roots, self._memo = {}, [], {}

    def _const(self, v):
        v %= R
        if v not in self.pool:
            self.pool.append(v)
        return (K_CONST << 24) | self.pool.index(v)

    def _dag(self, e):
        m = self._memo.get(id(e))
        if m is not None:
            return m
        if e.op == "const":
            key, kids, val = ("c", e.a), (), e.a
        elif e.op == "query":
            key, kids, val = ("q", e.a, e.b), (), (e.a, e.b)
        elif e.op == "neg":
            k = self._dag(e.a)
            key, kids, val = ("n", id(k)), (k,), None
        elif e.op == "scale":
            k = self._dag(e.a)
            key, kids, val = ("s", id(k), e.b), (k,), e.b
        elif e.op == "add" and e.b.op == "neg":
            x, y = self._dag(e.a), self._dag(e.b.a)
            key, kids, val = ("-", id(x), id(y)), (x, y), None
        else:
            x, y = self._dag(e.a), self._dag(e.b)
            key, kids, val = ("+" if e.op == "add" else "*", id(x), id(y)), (x, y), None
        node = self.nodes.get(key)
        if node is None:
            node = self.nodes[key] = _Node(key[0], kids, val)
            node.need = 0 if not kids else max(1, max(k.need for k in kids) if len(kids) == 1 or kids[0].need != kids[1].need else kids[0].need + 1)
            for k in kids:
                k.uses += 1
        self._memo[id(e)] = node
        return node

    def emit(self, e):
        node = self._dag(e)
        node.uses += 1
        self.roots.append(node)

    def _alloc(self):
        if not self.free:
            raise ValueError("expression needs more than %d registers" % MAX_REGS)
        r = self.free.pop()
        self.peak = max(self.peak, MAX_REGS - len(self.free))
        return r

    def _done_with(self, node):
        node.uses -= 1
        if node.uses == 0 and node.reg is not None:
            self.free.append(node.reg)
            node.reg = None

    def _gen(self, node):
        if node.op == "c":
            return self._const(node.val)
        if node.op == "q":
            return (_KIND_OPERAND[node.val[0]] << 24) | node.val[1]
        if node.reg is not None:
            return (K_REG << 24) | node.reg
        kids = node.kids
        if len(kids) == 2 and kids[1].need > kids[0].need and kids[0] is not kids[1]:
            b = self._gen(kids[1])
            a = self._gen(kids[0])
        else:
            a = self._gen(kids[0])
            b = self._gen(kids[1]) if len(kids) == 2 else 0
        for k in kids:
            self._done_with(k)
        d = self._alloc()
        if node.op == "n":
            self.code.append((OP_NEG, d, a, 0))
        elif node.op == "s":
            self.code.append((OP_MUL, d, a, self._const(node.val)))
        else:
            self.code.append(({"+": OP_ADD, "-": OP_SUB, "*": OP_MUL}[node.op], d, a, b))
        node.reg = d
        return (K_REG << 24) | d

    def finish(self):
        if self.roots is None:
            return
        for node in self.roots:
            v = self._gen(node)
            self.code.append((OP_EMIT, 0, v, 0))
            self._done_with(node)
        self.roots = None

    def words(self):
        self.finish()
        return np.array(self.code, dtype=np.uint32).reshape(-1, 4)


MAGIC = 0x4B4C503535334C47          # "GL355PLK" little endian


def to_limbs(values):
    """Python integers -> [len][4] uint64 (little-endian limbs)"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        v = int(v) % R
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_limbs(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a]


def vk_digest(cs, k, fixed_commitments, sigma_commitments, keccak256):
    """the scalar the transcript starts from (halo2: vk.transcript_repr, a hash of the PINNED verifying key): Keccak-256 over the descriptor
    (digest field zero: shape, queries, permutation columns, gate and lookup programs) and the key's fixed and permutation commitments
    ([cols][8] uint64: x, y little-endian words; the identity = zeros), read as a big-endian integer mod r -- what gl355_plonk_keygen derives
    itself (include/gl355.h).  A stand-in with transcript_repr's role (halo2's Blake2b-of-debug-string cannot be restated); it binds the
    fixed values and the copy constraints through their commitments.  keccak256: bytes -> 32 bytes (the caller's implementation: the
    checker recomputes the digest with its own)."""
    pre = export_desc(cs, k, 0).tobytes()
    pre += np.ascontiguousarray(fixed_commitments, dtype=np.uint64).tobytes() + np.ascontiguousarray(sigma_commitments, dtype=np.uint64).tobytes()
    return int.from_bytes(keccak256(pre), "big") % R


def export_desc(cs, k, digest):
    """the descriptor blob of include/gl355.h (gl355_plonk_keygen): header, permutation columns, queries, constant pool, gate program,
    per lookup the input and the table program"""
    pool = []
    gate = ProgramBuilder(pool)
    for p in cs.all_gate_polys():
        gate.emit(p)
    lks = []
    for _, ins, tabs in cs.lookups:
        pi, pt = ProgramBuilder(pool), ProgramBuilder(pool)
        for e in ins:
            pi.emit(e)
        for e in tabs:
            pt.emit(e)
        lks.append((pi, pt))
    hdr = np.zeros(24, dtype=np.uint64)
    hdr[0], hdr[1], hdr[2] = MAGIC, 1, k
    hdr[3], hdr[4], hdr[5] = cs.num_advice, cs.num_fixed, cs.num_instance
    hdr[6], hdr[7], hdr[8], hdr[9] = len(cs.permutation), len(cs.lookups), cs.degree(), cs.blinding_factors()
    hdr[10], hdr[11], hdr[12] = len(cs.queries[ADVICE]), len(cs.queries[FIXED]), len(cs.queries[INSTANCE])
    for pb in [gate] + [x for pair in lks for x in pair]:
        pb.finish()
    hdr[13], hdr[14], hdr[15] = len(pool), len(gate.code), len(cs.all_gate_polys())
    hdr[16:20] = to_limbs([digest])[0]
    parts = [hdr]
    parts.append(np.array([(c.kind << 32) | c.index for c in cs.permutation], dtype=np.uint64))
    for kind in (ADVICE, FIXED, INSTANCE):
        parts.append(np.array([(col << 32) | (rot & 0xFFFFFFFF) for col, rot in cs.queries[kind]], dtype=np.uint64))
    parts.append(to_limbs(pool).reshape(-1))

    def prog_words(pb):
        w = pb.words().reshape(-1)
        return w.view(np.uint64) if w.size else np.zeros(0, dtype=np.uint64)
    parts.append(prog_words(gate))
    for pi, pt in lks:
        parts.append(np.array([len(pi.code), len(pt.code)], dtype=np.uint64))
        parts.append(prog_words(pi))
        parts.append(prog_words(pt))
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in parts])


# ---- the prover behind the C ABI (include/gl355.h: gl355_plonk_keygen / gl355_plonk_prove) -----------------------------------------------
STAGES = ("advice", "lookup_permute", "permutation", "lookup_product", "vanishing_random", "evaluate_h", "quotient_commit", "evaluations", "shplonk")


def kzg_setup(ctx, k, tau, lagrange=True):
    """ParamsKZG::<Bn256>::setup(k, rng) (verifier_api.rs:77) with the secret handed in: (g, g_lagrange) as [2^k][8] uint64 arrays"""
    n = 1 << k
    g = np.zeros((n, 8), dtype=np.uint64)
    gl = np.zeros((n, 8), dtype=np.uint64) if lagrange else None
    t = to_limbs([tau])[0]
    ctx.check(ctx.lib.gl355_kzg_setup(ctx.h, t.ctypes.data, k, g.ctypes.data, gl.ctypes.data if lagrange else None))
    return g, gl


def _points_ptr(a):
    """(void* value, number of points) of a [n][8] uint64 numpy array or torch tensor; (a, None) for a raw device pointer (int)"""
    if isinstance(a, int):
        return a, None
    if isinstance(a, np.ndarray):
        assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"] and a.ndim == 2 and a.shape[1] == 8, "need a C-contiguous [n][8] uint64 array"
        return a.ctypes.data, a.shape[0]
    assert a.is_contiguous() and a.dim() == 2 and a.shape[1] == 8 and a.element_size() == 8, "need a contiguous [n][8] 64-bit tensor"
    return a.data_ptr(), a.shape[0]


def g1_fft(ctx, points, inverse=False, log_n=None):
    """The Fr FFT of gl355_bn254_fr_ntt with G1 points as the elements: out[k] = sum_i [w^(ik)] points[i] (inverse: w^-1 and 1/n).
    A numpy array is transformed into a new array; a torch tensor or a device pointer (int, log_n required) in place, and returned."""
    ptr, n = _points_ptr(points)
    if n is None:
        assert log_n is not None, "a raw pointer needs log_n"
    else:
        log_n = n.bit_length() - 1 if log_n is None else log_n
        assert n == 1 << log_n, "g1_fft takes 2^log_n points"
    if isinstance(points, np.ndarray):
        points = points.copy()
        ptr = points.ctypes.data
    ctx.check(ctx.lib.gl355_bn254_g1_fft(ctx.h, ptr, log_n, 1 if inverse else 0))
    if not isinstance(points, np.ndarray):
        ctx.sync()                      # device results: done before the caller's own streams read them
    return points


def kzg_lagrange_from_powers(ctx, g, k, out=None, n_points=None):
    """ParamsKZG::downsize(k) / g_to_lagrange: the Lagrange bases of the 2^k domain from public monomial bases g[i] = [tau^i] G1
    (n_points >= 2^k of them, e.g. a larger ceremony's; only the prefix is read), with no knowledge of tau.  g: numpy [n][8] uint64,
    a torch tensor, or a device pointer (int, with n_points).  Returns `out`, or a new array / tensor of g's kind (2^k x 8): it goes
    straight into PlonkProver(ctx, cs, k, g[:2**k], g_lagrange, ...)."""
    ptr, n = _points_ptr(g)
    n = n_points if n is None else n
    assert n is not None, "a raw pointer needs n_points"
    if out is None:
        if isinstance(g, np.ndarray) or isinstance(g, int):
            out = np.zeros((1 << k, 8), dtype=np.uint64)
        else:
            import torch
            out = torch.empty((1 << k, 8), dtype=g.dtype, device=g.device)
    optr, on = _points_ptr(out)
    assert on is None or on == 1 << k, "out holds 2^k points"
    ctx.check(ctx.lib.gl355_kzg_lagrange_from_powers(ctx.h, ptr, n, k, optr))
    if not isinstance(out, np.ndarray):
        ctx.sync()
    return out


# ---- the pairing side (include/gl355.h: gl355_bn254_g2_mul / _pairing_check, gl355_plonk_vk_* / _verify*, gl355_kzg_params_check) ---------
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583     # bn256::Fq
# Ethereum's (EIP-197) / halo2curves' generator of G2: ((x.c0, x.c1), (y.c0, y.c1)) on y^2 = x^3 + 3 / (9 + u) over Fq[u] / (u^2 + 1)
G2_GENERATOR = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
                (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def _raw_limbs(values):
    """Python integers below 2^256 -> flat uint64 words, NOT reduced (coordinates, and values whose range the library is to check)"""
    out = np.zeros(4 * len(values), dtype=np.uint64)
    for i, v in enumerate(values):
        for j in range(4):
            out[4 * i + j] = (int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def g1_words(p):
    """(x, y) | None -> [8] uint64"""
    return np.zeros(8, dtype=np.uint64) if p is None else _raw_limbs([p[0], p[1]])


def g2_words(p):
    """((x.c0, x.c1), (y.c0, y.c1)) | None | a [16] uint64 array -> [16] uint64"""
    if isinstance(p, np.ndarray):
        assert p.dtype == np.uint64 and p.size == 16
        return np.ascontiguousarray(p).reshape(16)
    return np.zeros(16, dtype=np.uint64) if p is None else _raw_limbs([p[0][0], p[0][1], p[1][0], p[1][1]])


def g2_from_words(w):
    v = from_limbs(w)
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def _host_check(rc):
    if rc != 0:
        from . import _lib
        raise _lib.Gl355Error(rc, (_lib.load().gl355_plonk_verify_last_error() or b"").decode())


def g2_mul(scalar, point=None):
    """scalar * point on the G2 twist (point None: the generator) -> ((x.c0, x.c1), (y.c0, y.c1)) or None for the identity.  No GPU."""
    from . import _lib
    out = np.zeros(16, dtype=np.uint64)
    s = _raw_limbs([int(scalar) % (1 << 256)])
    pw = None if point is None else g2_words(point)
    _host_check(_lib.load().gl355_bn254_g2_mul(s.ctypes.data, None if pw is None else pw.ctypes.data, out.ctypes.data))
    return g2_from_words(out)


def pairing_check(g1s, g2s):
    """prod_i e(g1s[i], g2s[i]) == 1.  g1s: (x, y) | None; g2s: as g2_mul returns.  Raises Gl355Error (INVALID_ARG) for a point that is
    non-canonical, off its curve or (G2) outside the order-r subgroup.  No GPU."""
    import ctypes as C
    from . import _lib
    assert len(g1s) == len(g2s)
    a = np.concatenate([g1_words(p) for p in g1s]) if len(g1s) else np.zeros(8, dtype=np.uint64)
    b = np.concatenate([g2_words(p) for p in g2s]) if len(g2s) else np.zeros(16, dtype=np.uint64)
    ok = C.c_int32(0)
    _host_check(_lib.load().gl355_bn254_pairing_check(a.ctypes.data, b.ctypes.data, len(g1s), C.byref(ok)))
    return bool(ok.value)


def kzg_setup_g2(tau):
    """[tau] G2: the G2 half of ParamsKZG::setup (verifier_api.rs:77) for a known secret -- tests, and users of kzg_setup"""
    return g2_mul(int(tau) % R)


def kzg_params_check(ctx, g, s_g2, k, g_lagrange=None, seed=None):
    """Is g (numpy [n][8] uint64) a run of consecutive powers of the secret behind s_g2, and g_lagrange (optional, [2^k][8]) the Lagrange form of
    g[:2^k]?  Randomised (error <= 2^-128 per check); seed: 32 bytes, None = the OS's generator.  -> bool"""
    import ctypes as C
    g = np.ascontiguousarray(g, dtype=np.uint64)
    assert g.ndim == 2 and g.shape[1] == 8
    if g_lagrange is not None:
        g_lagrange = np.ascontiguousarray(g_lagrange, dtype=np.uint64)
        assert g_lagrange.shape == (1 << k, 8)
    s = g2_words(s_g2)
    ok = C.c_int32(0)
    rc = ctx.lib.gl355_kzg_params_check(ctx.h, g.ctypes.data, g.shape[0], None if g_lagrange is None else g_lagrange.ctypes.data, k, s.ctypes.data,
                                        None if seed is None else bytes(seed), C.byref(ok))
    _host_check(rc)
    return bool(ok.value)


class PlonkVerifier:
    """verify_proof::<_, VerifierSHPLONK<_>, _, _, SingleStrategy<_>> (chip/native_chip/test_utils.rs:82-93) through gl355_plonk_vk_* /
    gl355_plonk_verify*: the circuit description, the key's commitments ([cols][8] uint64) and the parameter set's [s] G2 -- never the secret.
    digest None: the pinned-key rule of keygen (vk_digest)."""

    def __init__(self, cs, k, fixed_commitments, sigma_commitments, s_g2, digest=None, _handle=None):
        import ctypes as C
        from . import _lib
        self.lib, self.cs, self.k = _lib.load(), cs, k
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
            return
        desc = export_desc(cs, k, 0)
        fc = np.ascontiguousarray(fixed_commitments, dtype=np.uint64).reshape(-1)
        sc = np.ascontiguousarray(sigma_commitments, dtype=np.uint64).reshape(-1)
        assert fc.size == 8 * cs.num_fixed and sc.size == 8 * len(cs.permutation)
        d = None if digest is None else to_limbs([digest])[0]
        s = g2_words(s_g2)
        _host_check(self.lib.gl355_plonk_vk_create(desc.ctypes.data, desc.size, fc.ctypes.data if fc.size else None, sc.ctypes.data if sc.size else None,
                                                   None if d is None else d.ctypes.data, s.ctypes.data, C.byref(self.h)))

    @property
    def last_error(self):
        return (self.lib.gl355_plonk_verify_last_error() or b"").decode()

    def _instances(self, instances):
        assert len(instances) == self.cs.num_instance
        flat = _raw_limbs([int(v) % R for col in instances for v in col] or [0])
        return flat, [len(c) for c in instances]

    def verify(self, instances, proof, ctx=None):
        """instances: per instance column a list of integers; proof: bytes.  -> bool (last_error names the failed step)"""
        import ctypes as C
        flat, lens = self._instances(instances)
        lens = np.array(lens + [0], dtype=np.uint32)
        proof = bytes(proof)
        ok = C.c_int32(0)
        _host_check(self.lib.gl355_plonk_verify(None if ctx is None else ctx.h, self.h, flat.ctypes.data, lens.ctypes.data, proof, len(proof), C.byref(ok)))
        return bool(ok.value)

    def verify_batch(self, ctx, instances_list, proofs, seed=None, want_first_bad=False):
        """many proofs under this key, one pairing-product check; ctx (or None): where the combined MSM may run.  -> bool (, first bad index or -1)"""
        import ctypes as C
        assert len(instances_list) == len(proofs)
        parts = [self._instances(i) for i in instances_list]
        flat = np.concatenate([np.zeros(0, dtype=np.uint64)] + [f for f, l in parts if sum(l)] + [np.zeros(4, dtype=np.uint64)])
        lens = np.array([x for _, l in parts for x in l] + [0], dtype=np.uint32)
        proofs = [bytes(p) for p in proofs]
        ptrs = (C.c_char_p * max(1, len(proofs)))(*proofs)
        plens = np.array([len(p) for p in proofs] + [0], dtype=np.uint64)
        ok, first = C.c_int32(0), C.c_int32(-1)
        _host_check(self.lib.gl355_plonk_verify_batch(None if ctx is None else ctx.h, self.h, len(proofs), flat.ctypes.data, lens.ctypes.data, ptrs, plens.ctypes.data,
                                                      None if seed is None else bytes(seed), C.byref(ok), C.byref(first) if want_first_bad else None))
        return (bool(ok.value), first.value) if want_first_bad else bool(ok.value)

    def stage_ms(self):
        """the last verify / verify_batch of this thread: dict(host=transcript + expressions, msm, pairing) in milliseconds"""
        ms = np.zeros(3, dtype=np.float64)
        _host_check(self.lib.gl355_plonk_verify_stage_ms(ms.ctypes.data))
        return dict(host=float(ms[0]), msm=float(ms[1]), pairing=float(ms[2]))

    def close(self):
        if getattr(self, "h", None):
            self.lib.gl355_plonk_vk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- MockProver (include/gl355.h: gl355_plonk_check_witness) ------------------------------------------------------------------------------
FAIL_GATE, FAIL_GATE_POISONED, FAIL_LOOKUP, FAIL_PERMUTATION = range(4)
FAIL_KIND_NAMES = ("gate", "gate (poisoned)", "lookup", "permutation")
Failure = collections.namedtuple("Failure", "kind index row aux name position")
Failure.__doc__ = """one record of gl355_plonk_check_witness (kind, index, row, aux) with, resolved on the host from the constraint system, `name`: the
gate's or the lookup's name / the permutation column, and `position`: the polynomial's place within its gate (None for the other kinds)"""


class NotSatisfied(AssertionError):
    def __init__(self, failures, total, shown=8):
        self.failures, self.total = failures, total
        lines = [describe_failure(f) for f in failures[:shown]]
        if total > len(lines):
            lines.append("... and %d more" % (total - len(lines)))
        super().__init__("the witness does not satisfy the circuit (%d failure%s):\n  %s" % (total, "" if total == 1 else "s", "\n  ".join(lines)))


def describe_failure(f):
    if f.kind in (FAIL_GATE, FAIL_GATE_POISONED):
        what = "reads a blinding row (poisoned)" if f.kind == FAIL_GATE_POISONED else "is not zero"
        return "gate '%s', polynomial %d (ordinal %d) %s at row %d" % (f.name, f.position, f.index, what, f.row)
    if f.kind == FAIL_LOOKUP:
        return "lookup '%s' (index %d): the input at row %d %s" % (f.name, f.index, f.row, "reads a blinding row (poisoned)" if f.aux else "is not in the table")
    return "copy constraint: %s (permutation column %d) row %d differs from its partner in permutation column %d" % (f.name, f.index, f.row, f.aux)


class MockProver:
    """halo2's MockProver::run(k, &circuit, instances) + verify / assert_satisfied (verifier_api.rs:34-52, :72-73) on one GPU context through
    gl355_plonk_check_witness: no SRS, no key.  fixed: [num_fixed][n][4] uint64, mapping: Assembly.mapping_array() or None (copy constraints
    are then not checked); both numpy arrays or device pointers (ints)."""

    def __init__(self, ctx, cs, k, fixed, mapping=None):
        self.ctx, self.cs, self.k, self.n = ctx, cs, k, 1 << k
        self.desc = export_desc(cs, k, 0)
        if not isinstance(fixed, int):
            fixed = np.ascontiguousarray(fixed, dtype=np.uint64)
            assert fixed.shape == (cs.num_fixed, self.n, 4)
        if mapping is not None and not isinstance(mapping, int):
            mapping = np.ascontiguousarray(mapping, dtype=np.uint32)
            assert mapping.shape == (len(cs.permutation), self.n, 2)
        self.fixed, self.mapping = fixed, mapping
        self.usable = self.n - (cs.blinding_factors() + 1)
        self._polys = [(name, j) for name, polys in cs.gates for j in range(len(polys))]
        self.stage_ms = None

    def _resolve(self, rec):
        kind, index, row, aux = (int(v) for v in rec)
        if kind in (FAIL_GATE, FAIL_GATE_POISONED):
            name, pos = self._polys[index]
        elif kind == FAIL_LOOKUP:
            name, pos = self.cs.lookups[index][0], None
        else:
            name, pos = repr(self.cs.permutation[index]), None
        return Failure(kind, index, row, aux, name, pos)

    @classmethod
    def from_artifact(cls, ctx, artifact):
        """the checker of a recorded circuit (halo2_goldilocks.Artifact)"""
        lay = artifact.layout
        return cls(ctx, lay.cs, lay.k, lay.fixed_array(), lay.mapping_array())

    def check(self, advice, instances, capacity=1 << 16):
        """-> (the first min(capacity, total) records as a [.][4] uint32 array in (kind, index, row) order, the exact total)"""
        import ctypes as C
        ctx = self.ctx
        if not isinstance(advice, int):
            advice = np.ascontiguousarray(advice, dtype=np.uint64)
            assert advice.shape == (self.cs.num_advice, self.n, 4)
        assert len(instances) == self.cs.num_instance
        flat = to_limbs([v for col in instances for v in col]) if any(len(c) for c in instances) else np.zeros((1, 4), dtype=np.uint64)
        lens = np.array([len(c) for c in instances] + [0], dtype=np.uint32)
        out = np.zeros((max(1, capacity), 4), dtype=np.uint32)
        total = C.c_uint64(0)
        ms = np.zeros(3, dtype=np.float64)
        ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)       # noqa: E731
        ctx.check(ctx.lib.gl355_plonk_check_witness(ctx.h, self.desc.ctypes.data, self.desc.size, ptr(self.fixed), ptr(self.mapping), ptr(advice), flat.ctypes.data,
                                                    lens.ctypes.data, out.ctypes.data if capacity else None, capacity, C.byref(total), ms.ctypes.data))
        self.stage_ms = dict(gates=float(ms[0]), lookups=float(ms[1]), permutation=float(ms[2]))
        return out[:min(capacity, total.value)], total.value

    def verify(self, advice, instances, capacity=1 << 16):
        """MockProver::verify: the failures (at most `capacity` of them), [] for a satisfied witness"""
        recs, _ = self.check(advice, instances, capacity)
        return [self._resolve(r) for r in recs]

    def assert_satisfied(self, advice, instances):
        recs, total = self.check(advice, instances, 8)
        if total:
            raise NotSatisfied([self._resolve(r) for r in recs], total)


class PlonkProver:
    """keygen_pk + create_proof of one circuit on one GPU context (chip/native_chip/test_utils.rs:57-95 through gl355_plonk_*).
    g / g_lagrange: numpy arrays (copied to the device) or device pointers (ints; must outlive the prover)."""

    def __init__(self, ctx, cs, k, g, g_lagrange, fixed, mapping, digest=None, checkable=False):
        """checkable: keep `fixed` and `mapping` (host arrays or device pointers) so that prove(check=True) can run the MockProver"""
        import ctypes as C
        self.ctx, self.cs, self.k, self.n = ctx, cs, k, 1 << k
        self.desc = export_desc(cs, k, 0 if digest is None else digest)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint64)
        mapping = np.ascontiguousarray(mapping, dtype=np.uint32)
        assert fixed.shape == (cs.num_fixed, self.n, 4) and mapping.shape == (len(cs.permutation), self.n, 2)
        self._keep = (g, g_lagrange)
        # prove(check=True) needs the circuit's side again: kept only on request (at k = 23 the host arrays are several GB a caller may want to free)
        self._check_args = (fixed, mapping) if checkable else None
        self._mock = None
        self.tape = None            # from_artifact: the recorded circuit's tape on this context (prove_from_inputs)
        self._cols = None           # prove_from_inputs' device buffer for the advice columns, kept until close()
        ptr = lambda a: a if isinstance(a, int) else a.ctypes.data       # noqa: E731
        self.h = C.c_void_p()
        ctx.check(ctx.lib.gl355_plonk_keygen(ctx.h, self.desc.ctypes.data, self.desc.size, ptr(g), ptr(g_lagrange), fixed.ctypes.data, mapping.ctypes.data, C.byref(self.h)))
        info = np.zeros(8, dtype=np.uint64)
        ctx.check(ctx.lib.gl355_plonk_pk_info(self.h, info.ctypes.data))
        self.info = dict(k=int(info[0]), extended_k=int(info[1]), n_sets=int(info[2]), n_pieces=int(info[3]), usable=int(info[4]), proof_bytes=int(info[5]))
        self.fixed_commitments = np.zeros((cs.num_fixed, 8), dtype=np.uint64)
        self.sigma_commitments = np.zeros((len(cs.permutation), 8), dtype=np.uint64)
        ctx.check(ctx.lib.gl355_plonk_pk_commitments(self.h, self.fixed_commitments.ctypes.data, self.sigma_commitments.ctypes.data))
        if digest is None:          # derived by keygen from the descriptor and the commitments above
            d = np.zeros(4, dtype=np.uint64)
            ctx.check(ctx.lib.gl355_plonk_pk_digest(self.h, d.ctypes.data))
            self.digest = from_limbs(d)[0]
        else:
            self.set_digest(digest)

    def set_digest(self, digest):
        d = to_limbs([digest])[0]
        self.ctx.check(self.ctx.lib.gl355_plonk_pk_set_digest(self.h, d.ctypes.data))
        self.digest = digest

    def mock_prover(self):
        """the MockProver of this prover's circuit (a prover built with checkable=True), made on first use"""
        if self._mock is None:
            if self._check_args is None:
                raise ValueError("prove(check=True) needs a PlonkProver built with checkable=True (it keeps the fixed columns and the mapping)")
            self._mock = MockProver(self.ctx, self.cs, self.k, *self._check_args)
        return self._mock

    def prove(self, advice, instances, seed, want_trace=False, timed=False, check=False):
        """advice: [num_advice][n][4] uint64 (numpy, or a device pointer as int); instances: per instance column a list of integers;
        seed: 32 bytes.  check (a prover built with checkable=True): run MockProver.assert_satisfied on the witness first and raise
        NotSatisfied instead of proving.
        -> proof bytes (, trace dict)(, {stage: ms})"""
        import ctypes as C
        ctx = self.ctx
        if check:
            self.mock_prover().assert_satisfied(advice, instances)
        if not isinstance(advice, int):
            advice = np.ascontiguousarray(advice, dtype=np.uint64)
            assert advice.shape == (self.cs.num_advice, self.n, 4)
        flat = to_limbs([v for col in instances for v in col]) if any(len(c) for c in instances) else np.zeros((1, 4), dtype=np.uint64)
        lens = np.array([len(c) for c in instances] + [0], dtype=np.uint32)
        buf = np.zeros(self.info["proof_bytes"], dtype=np.uint8)
        out_len = C.c_uint64(0)
        trace = np.zeros(32, dtype=np.uint64)
        ms = np.zeros(len(STAGES), dtype=np.float64)
        seed = bytes(seed)
        assert len(seed) == 32
        ctx.check(ctx.lib.gl355_plonk_prove(ctx.h, self.h, advice if isinstance(advice, int) else advice.ctypes.data, flat.ctypes.data, lens.ctypes.data, seed,
                                            buf.ctypes.data, buf.size, C.byref(out_len), trace.ctypes.data if want_trace else None, ms.ctypes.data if timed else None))
        out = [bytes(buf[:out_len.value])]
        if want_trace:
            t = from_limbs(trace.reshape(8, 4))
            out.append(dict(zip(("theta", "beta", "gamma", "y", "x", "shplonk_y", "shplonk_v", "shplonk_u"), t)))
        if timed:
            out.append(dict(zip(STAGES, (float(v) for v in ms))))
        return out[0] if len(out) == 1 else tuple(out)

    @classmethod
    def from_artifact(cls, ctx, artifact, g, g_lagrange, digest=None, checkable=False):
        """the prover of a recorded circuit (halo2_goldilocks.Artifact: layout + tape): keygen from the layout's fixed columns and copy constraints,
        the tape loaded on the context for prove_from_inputs"""
        from . import halo2_goldilocks as hg
        lay = artifact.layout
        self = cls(ctx, lay.cs, lay.k, g, g_lagrange, lay.fixed_array(), lay.mapping_array(), digest=digest, checkable=checkable)
        self.tape = hg.DeviceTape(ctx, artifact.tape, lay.k, lay.n_inputs)
        return self

    def prove_from_inputs(self, inputs, instances, seed, **kw):
        """gl355_halo2_synthesize -> gl355_plonk_prove on the resident columns: inputs (the proof's words, numpy or a device pointer) -> the advice
        columns in device memory -> the proof.  -> (what prove() returns, (first failing tape entry or 2^64 - 1, failing entries))"""
        import ctypes as C
        ctx = self.ctx
        if self.tape is None:
            raise ValueError("prove_from_inputs needs a PlonkProver made by from_artifact (it loads the tape)")
        if self._cols is None:
            cols = C.c_void_p()
            ctx.check(ctx.lib.gl355_malloc(ctx.h, self.cs.num_advice * self.n * 32, C.byref(cols)))
            self._cols = cols
        _, status = self.tape.synthesize(inputs, out=self._cols.value)
        return self.prove(self._cols.value, instances, seed, **kw), status

    def verifying_key(self, s_g2):
        """the PlonkVerifier of this key (its descriptor, commitments and current digest) under the parameter set's [s] G2"""
        import ctypes as C
        h = C.c_void_p()
        s = g2_words(s_g2)
        _host_check(self.ctx.lib.gl355_plonk_vk_from_pk(self.h, s.ctypes.data, C.byref(h)))
        return PlonkVerifier(self.cs, self.k, None, None, None, _handle=h)

    def close(self):
        if getattr(self, "tape", None) is not None:
            self.tape.close()
            self.tape = None
        if getattr(self, "_cols", None) is not None:
            self.ctx.lib.gl355_free(self.ctx.h, self._cols)
            self._cols = None
        if getattr(self, "h", None):
            self.ctx.lib.gl355_plonk_pk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
