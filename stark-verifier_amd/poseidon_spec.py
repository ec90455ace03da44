"""The constant tables of the Goldilocks Poseidon (width 12, 8 full and 22 partial rounds, x^7) in the two optimised forms the Halo2 verifier
circuit restates, derived once per process from the round constants in data/ and the circulant MDS matrix.  Modular matrix algebra only.

  fast_partial_tables()   plonky2's fast partial rounds, what PoseidonGate's constraints are written over (chip/plonk/gates/poseidon.rs:127-319
                          carries them as literals: FAST_PARTIAL_FIRST_ROUND_CONSTANT, _ROUND_CONSTANTS, _ROUND_VS, _ROUND_W_HATS,
                          _ROUND_INITIAL_MATRIX); tests/golden/poseidon_fast_partial_tables.json and csrc/poseidon_fast_tables.h hold the same numbers
  optimized_spec()        Spec::new(8, 22) of chip/poseidon_spec/spec.rs:307-407, what PublicInputsHasherChip walks: the constants moved
                          behind the S-box (start, partial, end), the pre-sparse MDS and the 22 sparse matrices (row, col_hat)
They are right exactly when the permutations below agree with the dense rounds (permute_dense), which is plonky2's permutation."""
import functools
import os

P = (1 << 64) - (1 << 32) + 1
T, HALF_F, R_P = 12, 4, 22
MDS_MATRIX_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_MATRIX_DIAG = [8] + [0] * 11


@functools.lru_cache(maxsize=None)
def round_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "poseidon_goldilocks_round_constants.txt")
    with open(path) as f:
        vals = [int(line, 16) for line in f.read().split("\n") if line and not line.startswith("#")]
    assert len(vals) == T * (2 * HALF_F + R_P)
    return [vals[T * r:T * (r + 1)] for r in range(2 * HALF_F + R_P)]


def mds_matrix():
    """new[r] = sum_i CIRC[i] old[(i + r) % 12] + DIAG[r] old[r] (poseidon.rs:450-486)"""
    m = [[0] * T for _ in range(T)]
    for r in range(T):
        for i in range(T):
            m[r][(i + r) % T] = (m[r][(i + r) % T] + MDS_MATRIX_CIRC[i]) % P
        m[r][r] = (m[r][r] + MDS_MATRIX_DIAG[r]) % P
    return m


def mat_mul(a, b):
    return [[sum(a[i][x] * b[x][j] for x in range(len(b))) % P for j in range(len(b[0]))] for i in range(len(a))]


def mat_vec(a, v):
    return [sum(x * y for x, y in zip(row, v)) % P for row in a]


def transpose(a):
    return [list(col) for col in zip(*a)]


def mat_inv(a):
    n = len(a)
    aug = [list(row) + [int(i == j) for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        piv = next(r for r in range(c, n) if aug[r][c] % P)
        aug[c], aug[piv] = aug[piv], aug[c]
        inv = pow(aug[c][c], P - 2, P)
        aug[c] = [x * inv % P for x in aug[c]]
        for r in range(n):
            if r != c and aug[r][c]:
                f = aug[r][c]
                aug[r] = [(x - f * y) % P for x, y in zip(aug[r], aug[c])]
    return [row[n:] for row in aug]


def permute_dense(state):
    """the 30 rounds as written: constants, S-box (all words, or the first), MDS"""
    rc, m = round_constants(), mds_matrix()
    s = [x % P for x in state]
    for r in range(2 * HALF_F + R_P):
        s = [(x + c) % P for x, c in zip(s, rc[r])]
        if r < HALF_F or r >= HALF_F + R_P:
            s = [pow(x, 7, P) for x in s]
        else:
            s[0] = pow(s[0], 7, P)
        s = mat_vec(m, s)
    return s


# ---- plonky2's fast partial rounds ----------------------------------------------------------------------------------------------------------
def derive_fast_partial(rc):
    """round constants [30][12] -> dict(first [12], post [22] (the last is 0), vs [22][11], w_hats [22][11], init [11][11]
    (result[c] += init[r - 1][c - 1] state[r]), m00 (the MDS matrix's corner, lane 0's own factor in a fast partial round)).  The one
    derivation: tools/gen_poseidon_tables.py writes csrc/poseidon_fast_tables.h from it"""
    m = mds_matrix()
    minv = mat_inv(m)
    part = rc[HALF_F:HALF_F + R_P]
    acc = list(part[R_P - 1])                                        # each round's constants pushed back through the round before
    post = [0] * R_P
    for r in range(R_P - 2, -1, -1):
        back = mat_vec(minv, acc)
        post[r] = back[0]
        back[0] = 0
        acc = [(x + y) % P for x, y in zip(part[r], back)]
    first = acc
    a = [row[:] for row in m]                                        # A = S blockdiag(1, A_hat): the block factor joins the MDS before it
    vs, w_hats = [None] * R_P, [None] * R_P
    for r in range(R_P - 1, -1, -1):
        a_hat = [row[1:] for row in a[1:]]
        vs[r] = [a[i][0] for i in range(1, T)]
        w_hats[r] = mat_mul([a[0][1:]], mat_inv(a_hat))[0]
        d = [[1] + [0] * (T - 1)] + [[0] + a_hat[i] for i in range(T - 1)]
        a = mat_mul(d, m)
    init = [[d[c][r] for c in range(1, T)] for r in range(1, T)]
    return dict(first=first, post=post, vs=vs, w_hats=w_hats, init=init, m00=m[0][0])


@functools.lru_cache(maxsize=None)
def fast_partial_tables():
    return derive_fast_partial(round_constants())


# ---- Spec::new(8, 22) -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def optimized_spec():
    """-> dict(mds, pre_sparse_mds [12][12], sparse [(row [12], col_hat [11])] * 22, start [5][12], partial [22], end [3][12])"""
    rc, mds = round_constants(), mds_matrix()
    inv = mat_inv(mds)
    # calculate_optimized_constants, spec.rs:328-385
    start = [list(rc[0])] + [mat_vec(inv, rc[i]) for i in range(1, HALF_F)]
    acc = list(rc[HALF_F + R_P])
    partial = [0] * R_P
    for j, constants in zip(range(R_P - 1, -1, -1), reversed(rc[HALF_F:HALF_F + R_P])):
        tmp = mat_vec(inv, acc)
        partial[j] = tmp[0]
        tmp[0] = 0
        acc = [(x + y) % P for x, y in zip(tmp, constants)]
    start.append(mat_vec(inv, acc))
    end = [mat_vec(inv, rc[i]) for i in range(HALF_F + R_P + 1, 2 * HALF_F + R_P)]
    # calculate_sparse_matrices with factorise, spec.rs:195-224, :387-406
    mds_t = transpose(mds)
    acc = mds_t
    sparse = []
    for _ in range(R_P):
        w = [row[0] for row in acc[1:]]
        m_hat = [row[1:] for row in acc[1:]]
        w_hat = mat_vec(mat_inv(m_hat), w)
        sparse.append(([acc[0][0]] + w_hat, list(acc[0][1:])))      # (prime_prime)^T as (row, col_hat)
        m_prime = [[1] + [0] * (T - 1)] + [[0] + row for row in m_hat]
        acc = mat_mul(mds_t, m_prime)
    sparse.reverse()
    return dict(mds=mds, pre_sparse_mds=transpose(acc), sparse=sparse, start=start, partial=partial, end=end)


def permute_optimized(state):
    """PublicInputsHasherChip::permutation (public_inputs_hasher_chip.rs:265-298) on integers"""
    sp = optimized_spec()
    s = [(x + c) % P for x, c in zip(state, sp["start"][0])]
    full = lambda s, cs, m: mat_vec(m, [(pow(x, 7, P) + c) % P for x, c in zip(s, cs)])      # noqa: E731
    for cs in sp["start"][1:HALF_F]:
        s = full(s, cs, sp["mds"])
    s = full(s, sp["start"][-1], sp["pre_sparse_mds"])
    for c, (row, col_hat) in zip(sp["partial"], sp["sparse"]):
        s[0] = (pow(s[0], 7, P) + c) % P
        s = [sum(x * y for x, y in zip(row, s)) % P] + [(e * s[0] + x) % P for e, x in zip(col_hat, s[1:])]
    for cs in sp["end"]:
        s = full(s, cs, sp["mds"])
    return full(s, [0] * T, sp["mds"])
