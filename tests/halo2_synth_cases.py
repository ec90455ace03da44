"""Recorded circuits the CPU and the GPU tests of the Halo2 witness tape share (test_halo2_goldilocks.py, test_halo2_synth_host.py,
test_gpu_halo2_synth.py): each case records a few chip calls at k = 17 (the 16-bit range table needs 2^16 rows) with edge operands and
returns the Recorder, whose eager values are the reference the two interpreters are compared with.  Cases are built once per process."""
import functools
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hg = importlib.import_module("stark-verifier_amd.halo2_goldilocks")
h2 = importlib.import_module("stark-verifier_amd.halo2")
import pymodel_bn254 as pm  # noqa: E402

K = 17
P = hg.P
# an Fr whose three 64-bit pieces include one >= p (the middle one): unpack works in base p, not base 2^64, so it decomposes like any other
WIDE_FR = (P - 5) | ((P + 7) << 64) | (3 << 128)
# circomlib's known-answer input of Poseidon t = 5 is (0, 1, 2, 3, 4) as scalars; through pack a state can only reach scalars below p^3, so
# the KAT state here packs to (0, 1, 2, 3) with the capacity element 0 that AllChip::permute appends
KAT_STATE = [0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0, 0]


def values(rec, idxs):
    g = hg.GoldilocksChip(rec)
    return [g.assign_value(hg.Input(i)) for i in idxs]


@functools.lru_cache(maxsize=None)
def arithmetic_case():
    """every ArithmeticChip / GoldilocksChip / VectorChip method once, on 0, 1, p - 1 and products at their maximum"""
    inputs = [0, 1, P - 1, 0x123456789ABCDEF, P - 2, 2, 3, 5]
    rec = hg.Recorder(K, inputs)
    g = hg.GoldilocksChip(rec)
    ar = g.arithmetic_chip
    g.load_table()
    zero, one, m1, x, m2, two, three, five = values(rec, range(8))
    out = {}
    out["add"] = g.add(m1, m1)
    out["sub"] = g.sub(zero, one)
    out["mul_max"] = g.mul_add(m1, m1, m1)                       # (p - 1)^2 + (p - 1): the largest a b + c
    out["mul"] = g.mul(x, m2)
    out["mul_with_constant"] = g.mul_with_constant(x, two, P - 1)
    out["add_constant"] = g.add_constant(m1, 1)
    out["ext_max"] = ar.apply_ext([m1, m1], [m1, m1], [m1, m1]).r   # 8 (p - 1)^2 + (p - 1): q needs its fifth limb
    out["ext"] = ar.apply_ext([x, two], [three, five], [one, zero]).r
    out["select1"] = g.select(x, m2, one)
    out["select0"] = g.select(x, m2, zero)
    out["is_zero_0"] = g.is_zero(zero)
    out["is_zero_x"] = g.is_zero(x)
    out["is_equal"] = g.is_equal(x, x)
    out["is_not_equal"] = g.is_equal(x, m2)
    bits = g.to_bits(m1, 64)                                     # p - 1 = 0xFFFFFFFF00000000
    out["bits"] = bits
    out["from_bits"] = g.from_bits(bits[:40])
    out["exp2"] = g.exp_power_of_2(x, 5)
    out["exp_bits"] = g.exp_from_bits(7, g.to_bits(five, 3))
    out["compose"] = g.compose([(x, 3), (m1, P - 1)], 11)
    ar.range_check(out["mul"])
    g.assert_one(out["is_zero_0"])
    g.assert_zero(out["is_zero_x"])
    packed = ar.pack([zero, one, m1])
    out["packed"] = packed
    out["unpacked"] = ar.unpack(packed)
    ar.assert_equal_ext(out["unpacked"][:2], [zero, one])
    out["unpacked_wide"] = ar.unpack(ar.assign_constant(WIDE_FR))
    vec = [x, m2, m1, three]
    out["access_first"] = hg.VectorChip(rec, vec).access(zero)
    out["access_last"] = hg.VectorChip(rec, vec).access(three)
    ar.expose_public(out["mul"], 0)
    ar.expose_public(out["access_last"], 1)
    return rec, out


@functools.lru_cache(maxsize=None)
def failing_value_case():
    """an assign_value of a word that is not below p, between good ones; the later rows that use it are still written"""
    rec = hg.Recorder(K, [7, (1 << 64) - 1, P, 9])
    g = hg.GoldilocksChip(rec)
    g.load_table()
    a, bad, bad2, b = values(rec, range(4))
    g.mul_add(a, bad, b)
    g.add(bad2, a)
    return rec


@functools.lru_cache(maxsize=None)
def failing_assert_case():
    rec = hg.Recorder(K, [5, 6])
    g = hg.GoldilocksChip(rec)
    g.load_table()
    a, b = values(rec, range(2))
    s = g.add(a, b)
    g.assert_equal(s, a)                                         # 11 != 5
    g.assert_zero(g.sub(s, s))                                   # holds
    g.assert_one(b)                                              # 6 != 1
    return rec


def permute_states():
    rng = np.random.default_rng(0x4A10)
    return [[0] * 12, list(KAT_STATE), [int(v) for v in rng.integers(0, P, 12, dtype=np.uint64)]]


@functools.lru_cache(maxsize=None)
def permute_case():
    """AllChip.permute on three states -> (recorder, [(state, output cells, offset before, offset after)])"""
    states = permute_states()
    rec = hg.Recorder(K, [v for s in states for v in s])
    g = hg.GoldilocksChip(rec)
    g.load_table()
    runs = []
    for j, s in enumerate(states):
        cells = values(rec, range(12 * j, 12 * j + 12))
        g.assign_constant(0)
        before = rec.offset
        out = g.all_chip.permute(cells)
        runs.append((s, out, before, rec.offset))
    return rec, runs


@functools.lru_cache(maxsize=None)
def deep_case(depth=40):
    """`depth` chained permutations: one entry wide, 3 levels per link (pack, permute, unpack)"""
    rec = hg.Recorder(K, list(range(1, 13)))
    g = hg.GoldilocksChip(rec)
    g.load_table()
    state = values(rec, range(12))
    for _ in range(depth):
        state = g.all_chip.permute(state)
    return rec, state


@functools.lru_cache(maxsize=None)
def wide_case(width=4096 + 37):
    """`width` independent MULADD entries on one level (64 lanes per wave: a partial last wave), over three input words each"""
    rng = np.random.default_rng(0x51DE)
    inputs = [int(v) for v in rng.integers(0, P, 3 * width, dtype=np.uint64)]
    inputs[:6] = [P - 1] * 3 + [0] * 3
    rec = hg.Recorder(K, inputs)
    ar = hg.ArithmeticChip(rec)
    ar.load_table()
    out = [ar.apply(hg.Input(3 * i), hg.Input(3 * i + 1), hg.Input(3 * i + 2)).r for i in range(width)]
    return rec, out


# ---- Merkle proofs under the BN254-Poseidon hasher -----------------------------------------------------------------------------------------
def merkle_tree(bn, leaves, cap_height):
    """-> (cap, proofs): plonky2's MerkleTree over hash_or_noop leaves with the oracle's hasher `bn` (oracle_lib.Bn254Oracle)"""
    layer = [[int(v) for v in (leaf if len(leaf) <= 4 else bn.hash_no_pad(np.array(leaf, dtype=np.uint64)))] for leaf in leaves]
    layer = [h + [0] * (4 - len(h)) for h in layer]
    proofs = [[] for _ in leaves]
    span = 1
    while len(layer) > (1 << cap_height):
        for i in range(len(leaves)):
            proofs[i].append(layer[(i // span) ^ 1])
        layer = [[int(v) for v in bn.two_to_one(np.array(layer[i], dtype=np.uint64), np.array(layer[i + 1], dtype=np.uint64))] for i in range(0, len(layer), 2)]
        span *= 2
    return layer, proofs


def merkle_case(bn, depth, leaf_len, index, mutate=None):
    """verify_merkle_proof_to_cap_with_cap_index of leaf `index` of a 2^depth-leaf tree with cap height 1.  mutate: None, "sibling" (one word
    of the first sibling changed; depth 0: one word of the leaf) or "cap_index" (the other cap entry).
    -> the recorder"""
    rng = np.random.default_rng(0xCA9 + depth)
    n_leaves = 1 << depth
    leaves = [[int(v) for v in rng.integers(0, P, leaf_len, dtype=np.uint64)] for _ in range(n_leaves)]
    cap, proofs = merkle_tree(bn, leaves, 1 if depth else 0)
    if depth == 0:                                              # "a depth-0 proof": a two-entry cap, the leaf index selects the entry only
        other = [int(v) for v in rng.integers(0, P, leaf_len, dtype=np.uint64)]
        leaves = [leaves[0], other] if index == 0 else [other, leaves[0]]
        cap, proofs = merkle_tree(bn, leaves, 1)
        n_leaves = 2
    sib = [list(h) for h in proofs[index]]
    leaf = list(leaves[index])
    n_low = len(sib)
    cap_index = index >> n_low
    if mutate == "sibling":
        if sib:
            sib[0][2] ^= 1
        else:
            leaf[1] ^= 1
    elif mutate == "cap_index":
        cap_index ^= 1
    inputs = leaf + [v for h in sib for v in h] + [v for h in cap for v in h] + [index & ((1 << n_low) - 1), cap_index]
    rec = hg.Recorder(K, inputs)
    g = hg.GoldilocksChip(rec)
    g.load_table()
    it = iter(values(rec, range(len(inputs))))
    take = lambda m: [next(it) for _ in range(m)]      # noqa: E731
    leaf_c = take(len(leaf))
    sib_c = [take(4) for _ in sib]
    cap_c = [take(4) for _ in cap]
    low, cap_idx = take(2)
    bits = g.to_bits(low, n_low)
    hg.MerkleProofChip(rec).verify_merkle_proof_to_cap_with_cap_index(leaf_c, bits, cap_idx, cap_c, sib_c)
    return rec


def ints_of(arr):
    """[columns][rows][4] uint64 -> per column a list of Python integers"""
    return [h2.from_limbs(arr[c]) for c in range(arr.shape[0])]


def selector_rows(rec):
    """every row with a selector on (the only rows at which a gate can be non-zero or a lookup input non-zero)"""
    sel = set(rec.cs.selectors)
    return sorted({row for (col, row) in rec.fixed if col in sel})


class LazyColumns:
    """[columns][rows][4] uint64 read as [column][row] -> Python integer, converted on demand (the mock model touches a few hundred rows)"""

    class _Col:
        def __init__(self, a):
            self.a = a

        def __getitem__(self, r):
            w = self.a[r]
            return int(w[0]) | (int(w[1]) << 64) | (int(w[2]) << 128) | (int(w[3]) << 192)

    def __init__(self, arr):
        self.cols = [self._Col(arr[c]) for c in range(arr.shape[0])]

    def __getitem__(self, c):
        return self.cols[c]


def copy_failures(cs_, mapping, advice, fixed, instance):
    """the mock model's copy-constraint rule (halo2_mock_model.py: every cell against the cell its mapping names), vectorised over the columns:
    -> sorted [(PERMUTATION, j, i, partner's j)]"""
    n = advice.shape[1]
    inst = np.zeros((1, n, 4), dtype=np.uint64)
    for i, v in enumerate(instance):
        for j in range(4):
            inst[0, i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    src = {h2.ADVICE: advice, h2.FIXED: fixed, h2.INSTANCE: inst}
    cols = np.stack([src[c.kind][c.index] for c in cs_.permutation])                 # [m][n][4]
    partner = cols[mapping[:, :, 0].astype(np.int64), mapping[:, :, 1].astype(np.int64)]
    bad = np.argwhere((cols != partner).any(axis=2))
    return sorted((3, int(j), int(i), int(mapping[j, i, 0])) for j, i in bad)
