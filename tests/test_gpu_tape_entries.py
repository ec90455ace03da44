"""GPU: every witness-tape opcode and every kind of data failure, at a known entry of a hand-written tape, through both interpreters
(the host replay of csrc/witness_tape.cpp and tape_replay_kernel of csrc/witness_tape_dev.hip, which share csrc/witness_tape.h).

The tape hangs on a small built circuit (only its tables are needed to load an artifact) and has a sequential part and two
segments, each opcode's row or wires to itself, so that the final rows show every entry's result: 13 rows of 135 wires and 295
entries, most of them the INPUT entries that fill the operands of the wide rows (a REDUCING row of 43 coefficients, a
CosetInterpolationGate of 16 points).  Three units with different inputs must give equal rows and public inputs on host and device;
each data failure, injected through the inputs of unit 1 alone, must be refused by both with GL355_E_WITNESS at the injected entry,
and of two failures in different parts the smaller entry is the one reported."""
import importlib

import numpy as np
import pytest

from oracle_lib import rand_field
from test_gpu_prover import make_access_set

pytestmark = pytest.mark.gpu

gad = importlib.import_module("stark-verifier_amd.gadgets")
NW = 135
P = (1 << 64) - (1 << 32) + 1
REDUCING_CASES = ((1, 0), (43, 0), (1, 1), (32, 1))      # (coefficients, extension variant); 43 and 32 are the largest that fit 135 wires
COSET_CASES = ((2, 2), (4, 2))                           # (subgroup bits, degree)


def w(row, col):
    return NW * row + col


class HandTape:
    """entries, and the recipe of an input vector: each input has a kind, from which draw() makes a unit's value"""

    def __init__(self):
        self.entries, self.kinds, self.at = [], [], {}

    def add(self, op, a, b=0, c=0, d=0, name=None):
        self.entries.append((op, a, b, c, d))
        if name is not None:
            self.at[name] = len(self.entries) - 1

    def input(self, wire, kind="field"):
        """an INPUT entry into `wire`; -> the input's index"""
        self.kinds.append(kind)
        self.add(gad.TAPE_INPUT, wire, len(self.kinds) - 1)
        return len(self.kinds) - 1

    def inputs(self, wire, count):
        for k in range(count):
            self.input(wire + k)

    def draw(self, rng):
        out = np.zeros(len(self.kinds), dtype=np.uint64)
        for i, kind in enumerate(self.kinds):
            f = int(rand_field(rng, 1)[0])
            if isinstance(kind, tuple):                       # ("same", j): the value of input j
                out[i] = out[kind[1]]
            elif isinstance(kind, int):
                out[i] = kind
            else:
                out[i] = {"field": f, "nonzero": f or 1, "bit": f & 1, "u63": f >> 1, "idx16": f & 15, "above_p": P + f % ((1 << 32) - 1)}[kind]
        return out


def hand_tape():
    t, ix = HandTape(), {}
    # sequential part, on row 0
    t.add(gad.TAPE_CONST, w(0, 0), P + 5)                     # a constant is canonicalised
    ix["above_p"] = t.input(w(0, 1), "above_p")               # and so is an input
    t.input(w(0, 2))
    t.add(gad.TAPE_COPY, w(0, 4), w(0, 1))
    t.add(gad.TAPE_LO32, w(0, 5), w(0, 2))
    t.add(gad.TAPE_HI32, w(0, 6), w(0, 2))
    t.inputs(w(0, 8), 3)
    t.add(gad.TAPE_ARITH, w(0, 8), 3, P - 2)
    t.inputs(w(0, 12), 6)
    t.add(gad.TAPE_ARITH_EXT, w(0, 12), 5, P - 7)
    ix["inv"] = (t.input(w(0, 22), "nonzero"), t.input(w(0, 23)))
    t.add(gad.TAPE_EXT_INV, w(0, 20), w(0, 21), w(0, 22), w(0, 23), name="ext_inv")
    t.add(gad.TAPE_ASSERT_EQ, w(0, 4), w(0, 1))               # true whatever the inputs
    lhs = t.input(w(0, 24))
    ix["eq"] = t.input(w(0, 25), ("same", lhs))
    t.add(gad.TAPE_ASSERT_EQ, w(0, 24), w(0, 25), name="assert_eq")
    n_seq = len(t.entries)
    # segment 1: rows 1 .. 5
    t.inputs(w(1, 0), 12)
    t.input(w(1, 24), 0)
    t.add(gad.TAPE_POSEIDON, w(1, 0))
    for k in range(12):
        t.add(gad.TAPE_COPY, w(2, k), w(1, 12 + k))           # the second permutation takes the first one's outputs
    ix["swap"] = t.input(w(2, 24), 1)
    t.add(gad.TAPE_POSEIDON, w(2, 0), name="poseidon")
    t.inputs(w(3, 0), 24)
    t.add(gad.TAPE_MDS_EXT, w(3, 0))
    ix["sum1"] = t.input(w(4, 0), 1)
    t.add(gad.TAPE_BASE_SUM, w(4, 0), 1, name="base_sum_1")
    ix["sum63"] = t.input(w(5, 0), "u63")
    t.add(gad.TAPE_BASE_SUM, w(5, 0), 63, name="base_sum_63")
    n_seg1 = len(t.entries) - n_seq
    # segment 2: rows 6 .. 12
    for copy in (0, 3):
        ix["index", copy] = t.input(w(6, 18 * copy), "idx16")
        t.inputs(w(6, 18 * copy + 2), 16)
        t.add(gad.TAPE_RANDOM_ACCESS, w(6, 0), copy, name=("random_access", copy))
    for k, (n, ext) in enumerate(REDUCING_CASES):
        t.inputs(w(7 + k, 2), 4 + (2 * n if ext else n))      # alpha, the old accumulator, the coefficients
        t.add(gad.TAPE_REDUCING, w(7 + k, 0), n, ext)
    for k, (bits, degree) in enumerate(COSET_CASES):
        ix["shift", k] = t.input(w(11 + k, 0), "nonzero")
        t.inputs(w(11 + k, 1), (2 << bits) + 2)               # the values, the evaluation point
        t.add(gad.TAPE_COSET_INTERP, w(11 + k, 0), bits, degree, name=("coset", k))
    n_seg2 = len(t.entries) - n_seq - n_seg1
    pi_pos = [w(0, 1), w(0, 11), w(0, 20), w(2, 12), w(3, 24), w(8, 0), w(12, 2 * 16 + 3)]      # the last: evaluation_value of the 16-point gate
    return t, ix, (n_seq, [n_seg1, n_seg2]), np.array(pi_pos, dtype=np.uint64), 13


@pytest.fixture(scope="module")
def data(gl, ctx):
    """a small built circuit for the tapes to hang on"""
    aset, _, _ = make_access_set(gl, ctx, 4, 0x7A9E)
    return aset.build(None)[0]


@pytest.fixture(scope="module")
def loaded(gl, ctx, data):
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    t, ix, layout, pi_pos, n_rows = hand_tape()
    tape = np.array(t.entries, dtype=np.uint64)
    assert set(tape[:, 0].tolist()) == set(range(15))         # every opcode is there
    nat = plonk.NativeCircuit(ctx, data.export_blob(np.arange(n_rows), tape=tape, pi_pos=pi_pos, n_inputs=len(t.kinds), tape_layout=layout))
    rng = np.random.default_rng(0x7A9F)
    inputs = np.stack([t.draw(rng) for _ in range(3)])
    return nat, t, ix, layout, inputs


def test_rows_of_every_opcode_agree(gl, ctx, loaded):
    nat, t, ix, layout, inputs = loaded
    h_rows, h_pis = nat.witness_rows(ctx, inputs, on_device=False)
    d_rows, d_pis = nat.witness_rows(ctx, inputs, on_device=True)
    if not np.array_equal(h_rows, d_rows):
        bad = np.argwhere(h_rows != d_rows)
        raise AssertionError("device rows differ from host rows at %d positions, first (unit, row, wire) = %s" % (len(bad), bad[0]))
    assert np.array_equal(h_pis, d_pis) and np.array_equal(d_pis[:, 0], d_rows[:, 0, 1])
    assert int(d_rows.max()) < P
    for u in range(3):
        assert int(inputs[u, ix["above_p"]]) >= P and int(d_rows[u, 0, 1]) == int(inputs[u, ix["above_p"]]) - P
        assert int(d_rows[u, 0, 0]) == 5 and d_rows[u, 0, 4] == d_rows[u, 0, 1]
        assert np.any(d_rows[u, 2, 25:29] != 0)               # swap = 1: the delta wires are in use
        assert len({d_rows[u, r].tobytes() for r in range(13)}) == 13 and all(d_rows[u, r].any() for r in range(13))
    assert len({d_rows[u].tobytes() for u in range(3)}) == 3


def poseidon_row_cases():
    """(state, swap) of the PoseidonGate rows below: the edges of the field and of its 32-bit halves, both deltas of the swap wrapping
    (lhs = lanes 0..3 against rhs = lanes 4..7), and four random states, each with swap 0 and swap 1"""
    rng = np.random.default_rng(0x7AA0)
    e = (1 << 32) - 1
    states = [[0] * 12, [P - 1] * 12, [e] * 12, [P - e - 1] * 12, [0] * 4 + [P - 1] * 4 + [0] * 4, [P - 1] * 4 + [0] * 4 + [P - 1] * 4]
    states += [rand_field(rng, 12).tolist() for _ in range(4)]
    return [(np.array(s, dtype=np.uint64), swap) for swap in (0, 1) for s in states]


@pytest.fixture(scope="module")
def poseidon_rows(ctx, data):
    """a tape of one POSEIDON entry per case behind its INPUT entries, all in the sequential part (one wave per unit); unit 1 takes the
    cases in reverse order.  -> (circuit, inputs [2][20 * 13], the host's gate witness [2][20][135])"""
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    cases = poseidon_row_cases()
    assert len(cases) == 20
    t = HandTape()
    for k in range(len(cases)):
        t.inputs(w(k, 0), 12)
        t.input(w(k, 24))
        t.add(gad.TAPE_POSEIDON, w(k, 0))
    tape = np.array(t.entries, dtype=np.uint64)
    nat = plonk.NativeCircuit(ctx, data.export_blob(np.arange(len(cases)), tape=tape, pi_pos=np.array([w(0, 12)], dtype=np.uint64), n_inputs=len(t.kinds)))
    orders = (cases, cases[::-1])
    inputs = np.stack([np.concatenate([np.append(s, np.uint64(swap)) for s, swap in order]) for order in orders])
    want = np.stack([np.stack([plonk.poseidon_gate_witness(s, swap) for s, swap in order]) for order in orders])
    return nat, inputs, want


@pytest.mark.parametrize("units", (1, 2))
def test_poseidon_rows_equal_the_host_gate_witness(ctx, poseidon_rows, units):
    """tape_poseidon_row (the swap, psd_lane_round thirty times, the S-box-input and output wires) against gl355_poseidon_gate_witness: all 135
    wires of every row"""
    nat, inputs, want = poseidon_rows
    rows, pis = nat.witness_rows(ctx, inputs[:units], on_device=True)
    assert rows.shape == (units, 20, NW)
    if not np.array_equal(rows, want[:units]):
        bad = np.argwhere(rows != want[:units])
        raise AssertionError("device rows differ from the host gate witness at %d positions, first (unit, row, wire) = %s" % (len(bad), bad[0]))
    assert np.array_equal(pis[:, 0], want[:units, 0, 12])
    assert np.any(want[0, 10:, 25:29] != 0) and not np.any(want[0, :10, 25:29])      # the delta wires are in use exactly under swap = 1


def refused_at(gl, ctx, nat, inputs):
    """the entry at which both replays refuse `inputs`"""
    entries = []
    for dev in (False, True):
        with pytest.raises(gl.Gl355Error) as ei:
            nat.witness_rows(ctx, inputs, on_device=dev)
        assert ei.value.code == -6
        entries.append(ei.value.failed_entry)
    assert entries[0] == entries[1], "host refuses at entry %d, device at entry %d" % tuple(entries)
    return entries[0]


def failures(ix):
    """name of the refused entry -> {input: value}"""
    return {"assert_eq": {ix["eq"]: None}, "poseidon": {ix["swap"]: 2}, "base_sum_1": {ix["sum1"]: 2}, "base_sum_63": {ix["sum63"]: 1 << 63},
            ("random_access", 0): {ix["index", 0]: 16}, ("random_access", 3): {ix["index", 3]: 16}, "ext_inv": {ix["inv"][0]: P, ix["inv"][1]: 0},
            ("coset", 0): {ix["shift", 0]: 0}, ("coset", 1): {ix["shift", 1]: P}}


def inject(inputs, changes):
    bad = inputs.copy()
    for i, v in changes.items():
        bad[1, i] = bad[1, i] ^ np.uint64(1) if v is None else np.uint64(v)
    return bad


def test_each_data_failure_is_refused_at_its_entry(gl, ctx, loaded):
    nat, t, ix, layout, inputs = loaded
    for name, changes in failures(ix).items():
        assert refused_at(gl, ctx, nat, inject(inputs, changes)) == t.at[name], name


def test_the_smaller_of_two_failing_entries_is_reported(gl, ctx, loaded):
    nat, t, ix, layout, inputs = loaded
    f = failures(ix)
    n_seq, (n_seg1, _) = layout
    assert t.at["ext_inv"] < n_seq <= t.at["base_sum_63"] < n_seq + n_seg1 <= t.at["coset", 1]
    for first, second in (("base_sum_63", ("coset", 1)), ("poseidon", ("random_access", 0)), ("ext_inv", "base_sum_1")):
        assert refused_at(gl, ctx, nat, inject(inputs, {**f[first], **f[second]})) == t.at[first]
