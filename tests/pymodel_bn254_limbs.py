"""Plain-integer restatement of the BN254 limb arithmetic the device runs (stark-verifier_amd/csrc/bn254_field.cuh, bn254_f29.cuh, the point
formulas of bn254_g1.cuh and bn254_msm_acc.cuh) and the operands that sit at the edges of its lazy bounds.  Used by tests/test_bn254_limbs.py
(the restatement itself, on the CPU) and tests/test_gpu_bn254_arith.py (the device functions against it, through the test hooks of
include/gl355.h).  Nothing here is shared with the kernels: moduli and constants are derived from the two primes."""
import ctypes as C

import numpy as np

from pymodel_bn254_curve import Q, R

MOD = {"fr": R, "fq": Q}
M32 = (1 << 32) - 1
M29 = (1 << 29) - 1
R256 = 1 << 256
R261 = 1 << 261
N0 = {f: (-pow(m, -1, 1 << 32)) % (1 << 32) for f, m in MOD.items()}          # -m^-1 mod 2^32 (CIOS)
N0_29 = {f: (-pow(m, -1, 1 << 29)) % (1 << 29) for f, m in MOD.items()}       # -m^-1 mod 2^29 (f29_mul_mod)

# ---- the hooks' op codes and record layouts (include/gl355.h, "test hooks") --------------------------------------------------------------
M_MUL, M_ADD, M_SUB, M_CANON, M_FROM_INT, M_TO_INT, M_INV, M_IS_ZERO, M_EQ = range(9)
FQ = 16
(F29_MUL, F29_MUL_FR, F29_ADD_NORM, F29_SUB_C2, F29_SUB_C4, F29_SUB_C8, F29_SUB_C16, F29_NEG_C2, F29_FROM_U256, F29_TO_U256, F29_LIFT,
 F29_LIFT_INL, F29_LOWER, F29_IS_ZERO_MOD, F29_TABLE_FORM, F29_NORM, HASH_FR_ENTER, HASH_FR_LEAVE) = range(32, 50)
F29_SUB_K = {F29_SUB_C2: 2, F29_SUB_C4: 4, F29_SUB_C8: 8, F29_SUB_C16: 16}
CHAIN_XYZZ, CHAIN_JAC29, CHAIN_JAC, CHAIN_RED29_LIFT, CHAIN_RED29_RAW, CHAIN_J = range(6)
STEP_ADD, STEP_DOUBLE, STEP_ACC, STEP_SELF, STEP_MADD = range(5)
OPND_WORDS, REC_WORDS = 28, 40
NEG = 1 << 31


def step(kind, k=0):
    return kind << 28 | k


# ---- limb packing ------------------------------------------------------------------------------------------------------------------
def pack8(v):
    """an integer < 2^256 as the 8 x 32-bit form's record (word 8 = 0)"""
    assert 0 <= v < R256
    return [(v >> (32 * j)) & M32 for j in range(8)] + [0]


def val8(w):
    return sum(int(w[j]) << (32 * j) for j in range(8))


def pack29(v):
    """normalised 29-bit limbs (the top one takes what is left)"""
    assert v >= 0
    l = [(v >> (29 * j)) & M29 for j in range(8)] + [v >> 232]
    assert l[8] <= M32
    return l


def val29(w):
    return sum(int(w[j]) << (29 * j) for j in range(9))


def is_norm29(w):
    return all(int(w[j]) <= M29 for j in range(8))


def vals8(arr):
    """the integers of an (n, 9) uint32 array's words 0..7"""
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(arr[:, :8], dtype="<u4")]


def vals29(arr):
    a = arr.astype(object)
    v = a[:, 8]
    for j in range(7, -1, -1):
        v = (v << 29) + a[:, j]
    return list(v)


def lent(k):
    """f29_sub's constant C_k: k q with 2^29 lent to each low limb from the one above (bn254_f29.cuh FQ29_C2 .. C16)"""
    l = pack29(k * Q)
    for j in range(8):
        l[j] += 1 << 29
        l[j + 1] -= 1
    assert val29(l) == k * Q and l[8] >= 0
    return l


# ---- the 8 x 32-bit CIOS (m_mul's C form, bn254_field.cuh), limb by limb --------------------------------------------------------------
def cios(a, b, f, stats=None):
    """m_mul<F>'s plain C form on the integers a, b (< 2^256), returning its 256-bit result.  stats counts the rare events:
    't9' a row whose ninth-word carry t9 is non-zero, 'red_top' a reduction half-row whose top carry is non-zero, 'ge_m' a result in [m, 2m)."""
    m = MOD[f]
    M = [(m >> (32 * j)) & M32 for j in range(8)]
    A = [(a >> (32 * j)) & M32 for j in range(8)]
    B = [(b >> (32 * j)) & M32 for j in range(8)]
    n0 = N0[f]
    t = [0] * 9
    for i in range(8):
        c = 0
        for j in range(8):
            c = A[j] * B[i] + (t[j] + c)
            t[j] = c & M32
            c >>= 32
        c += t[8]
        t[8] = c & M32
        t9 = c >> 32
        if stats is not None and t9:
            stats["t9"] += 1
        mm = (t[0] * n0) & M32
        c = (mm * M[0] + t[0]) >> 32
        for j in range(1, 8):
            c = mm * M[j] + (t[j] + c)
            t[j - 1] = c & M32
            c >>= 32
        c += t[8]
        t[7] = c & M32
        if stats is not None and (c >> 32):
            stats["red_top"] += 1
        t[8] = (t9 + (c >> 32)) & M32
    r = sum(t[j] << (32 * j) for j in range(8))
    if stats is not None and m <= r:
        stats["ge_m"] += 1
    return r


def new_stats():
    return {"t9": 0, "red_top": 0, "ge_m": 0}


def m_from_int(a, f):
    """m_from_int: five conditional subtractions of m (2^256 < 6 m), then the product by R^2"""
    m = MOD[f]
    for _ in range(5):
        if a >= m:
            a -= m
    return cios(a, R256 * R256 % m, f)


def f29_mul_mod(a_l, b_l, f):
    """f29_mul_mod on limb lists; returns (limbs, largest 64-bit column value seen).  The 64-bit accumulators of the device are Python
    integers here, so an overflow there shows up as a column above 2^64 - 1."""
    m = MOD[f]
    M = pack29(m)
    n0 = N0_29[f]
    t = [0] * 10
    top = 0
    for i in range(9):
        for j in range(9):
            t[j] += a_l[j] * b_l[i]
        mm = ((t[0] & M32) * n0) & M29
        for j in range(9):
            t[j] += mm * M[j]
        top = max(top, max(t))
        c = t[0] >> 29
        t = t[1:] + [0]
        t[0] += c
    r = [0] * 9
    for j in range(8):
        r[j] = t[j] & M29
        t[j + 1] += t[j] >> 29
    top = max(top, max(t))
    r[8] = t[8]
    return r, top


# ---- documented bounds, once, next to the comment they come from (multiples of the modulus unless said otherwise) ---------------------------
BOUNDS = {
    # bn254_field.cuh: "a * b * R^-1 (mod m), result < 2m for a, b < 2m"; "Sums and differences (results < 2m for operands < 2m)";
    # m_canon "< 2m -> < m"; m_from_int "any 256-bit integer -> Montgomery form (< 2m)"; m_to_int: canonical
    "m_mul": 2, "m_add": 2, "m_sub": 2, "m_canon": 1, "m_from_int": 2, "m_to_int": 1,
    # bn254_f29.cuh f29_mul_mod: "a's limbs < 2^30.6, b's < 2^29.  Result: limbs < 2^29 ..., value < a b / 2^261 + m"
    "f29_mul_a_limb": 2 ** 30.6, "f29_mul_b_limb": 1 << 29,
    # f29_is_zero_mod: "a product's result (normalised, < 1.3 q, = 0 mod q)  <=>  it is 0 or q" -- valid below 2 q
    "f29_is_zero_mod": 2,
    # f29_lower: "any value below 2^261 -> < 1.3 q"
    "f29_lower_in": R261,
}
# bn254_msm_acc.cuh, per coordinate, "n" = limbs normalised:
#   struct jac29: "x < 5.2 n, y < 3.3 n, z < 1.3 n" (the bucket accumulators, Jacobian and XYZZ: "ZZ, ZZZ are products: < 1.3")
#   jac29_same_x: x3 "< 5.1", y = y3 * one and z = (2 y) * one are products
#   reduction: "inputs (X, Y, Z) < 12 q give X3 < 5.2, Y3 < 3.3, Z3 < 1.1 (addition) and X3 < 9.3, Y3 < 1.2, Z3 < 3.8 (doubling: ... < 2.1 for
#   the Y < 3.3, Z < 2.2 these formulas and the lifted items give the levels)"
BUCKET_BOUND = (5.2, 3.3, 1.3, 1.3)
RED_INPUT = 12
RED_ADD_BOUND = (5.2, 3.3, 1.1)
RED_DBL_BOUND = (9.3, 1.2, 3.8)
RED_DBL_BOUND_LEVELS = (9.3, 1.2, 2.1)
PRODUCT_BOUND = 1.3


def below(v, k):
    """v < k q exactly (k a decimal of one place)"""
    return 10 * v < round(10 * k) * Q


# ---- operand generators ------------------------------------------------------------------------------------------------------------------
def edge8(f, extra=()):
    """8 x 32-bit operands below 2m: the edges, powers of two and their neighbours, 0 / 0xffffffff limb patterns"""
    m = MOD[f]
    s = {0, 1, 2, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1, m // 2, m // 2 + 1, (m + 1) // 2 + m}
    for k in range(256):
        for v in ((1 << k) - 1, 1 << k, (1 << k) + 1, m + (1 << k), 2 * m - (1 << k), m - (1 << k)):
            if 0 <= v < 2 * m:
                s.add(v)
    for pat in range(1, 256):
        v = sum(M32 << (32 * j) for j in range(8) if (pat >> j) & 1)
        if v < 2 * m:
            s.add(v)
        w = (R256 - 1) ^ v
        if w < 2 * m:
            s.add(w)
    s.update(x for x in extra if 0 <= x < 2 * m)
    return sorted(s)


def from_int_edges(f):
    """m_from_int's domain [0, 2^256): k m + {-1, 0, 1} for every k, and the top"""
    m = MOD[f]
    s = {R256 - 1, R256 - 2, R256 - m, R256 - 2 * m}
    k = 0
    while k * m <= R256:
        s.update(v for v in (k * m - 1, k * m, k * m + 1, k * m + m // 2) if 0 <= v < R256)
        k += 1
    for j in range(8):
        s.add((R256 - 1) ^ (M32 << (32 * j)))
    return sorted(s)


def f29_normal_values():
    """normalised 29-bit operands: the edges of every multiple of q the formulas reach (up to the 12 q of the reduction inputs), powers of two,
    every low limb at 2^29 - 1"""
    s = {0, 1, 2, M29, 1 << 29, R256 - 1}
    for k in range(0, 13):
        s.update(v for v in (k * Q - 1, k * Q, k * Q + 1) if v >= 0)
    for x in (1.1, 1.2, 1.3, 2.2, 3.3, 3.9, 4.1, 5.1, 5.2, 5.3, 5.6, 6.2, 9.3, 11.9):
        s.add(int(x * 10) * Q // 10 - 1)
    for k in range(0, 257, 7):
        s.update({(1 << k) - 1, 1 << k})
    all_low = sum(M29 << (29 * j) for j in range(8))                 # every low limb 2^29 - 1
    for top in (0, 1, 0x30644e, 0x30644e * 5, 0x30644e * 11):
        s.add(all_low + (top << 232))
    return sorted(s)


def subtrahends(k):
    """f29_sub's subtrahends for the constant C_k: normalised, value < k q -- k q - 1, and every low limb at 2^29 - 1 with the largest top limb
    that stays below k q"""
    all_low = sum(M29 << (29 * j) for j in range(8))
    top = (k * Q - 1 - all_low) >> 232
    out = {0, 1, k * Q - 1, k * Q - 2, all_low + (top << 232), all_low, (k * Q) // 2}
    return sorted(v for v in out if 0 <= v < k * Q)


def lazy_first_operands():
    """the first operands of f29_mul the formulas form without a re-normalisation: f29_sub(a, b, C_k) with a's limbs at their maximum"""
    out = []
    all_low = [M29] * 8
    for k in (2, 4, 8, 16):
        C = lent(k)
        for a_top in (0, 0x30644e, 0x30644e * 5):
            a = all_low + [a_top]
            for b in (0, 1, k * Q - 1):
                bl = pack29(b)
                r = [a[j] + C[j] - bl[j] for j in range(9)]
                if r[8] >= 0:                                        # (f29_sub's condition on the top limb, bn254_f29.cuh)
                    out.append(r)
    return out


def f29_mul_ok(a_l, b_l, r_l, f):
    """f29_mul_mod's claim for one product: limbs 0..7 < 2^29, value < a b / 2^261 + m, congruent to a b 2^-261"""
    m = MOD[f]
    a, b, r = val29(a_l), val29(b_l), val29(r_l)
    return is_norm29(r_l) and r * R261 < a * b + m * R261 and (r * R261 - a * b) % m == 0


# ---- points ------------------------------------------------------------------------------------------------------------------------------
def affine_of(x, y, z, form):
    """the affine point of raw coordinates (integers): 'r' = 8 x 32 Jacobian in R = 2^256, '29' = Jacobian in R' = 2^261, 'xyzz' = XYZZ in R'
    (x, y, zz, zzz given as z = (zz, zzz)).  None for the identity."""
    if form == "xyzz":
        zz, zzz = z
        k = pow(R261, -1, Q)
        zz, zzz = zz * k % Q, zzz * k % Q
        if zz == 0:
            return None
        return x * k * pow(zz, -1, Q) % Q, y * k * pow(zzz, -1, Q) % Q
    k = pow(R256 if form == "r" else R261, -1, Q)
    X, Y, Z = x * k % Q, y * k % Q, z * k % Q
    if Z == 0:
        return None
    zi = pow(Z, -1, Q)
    return X * zi * zi % Q, Y * zi * zi * zi % Q


def jac_of(p, z, form):
    """raw Jacobian coordinates (integers, canonical) of the affine point p with the given z (plain value)"""
    if p is None:
        return 0, 0, 0
    k = R256 if form == "r" else R261
    x, y = p
    return x * z * z * k % Q, y * z * z * z * k % Q, z * k % Q


def operand_record(x, y, z, ident=0, form="r"):
    """a 28-word operand record: three 9-word slots (8 x 32 or 29-bit limbs) and the identity flag"""
    pk = pack8 if form == "r" else pack29
    return pk(x) + pk(y) + pk(z) + [ident]


def trace_coords(rec, form):
    """(coordinates as integers, identity flag, accumulator) of one trace record"""
    v = vals8 if form == "r" else vals29
    slots = np.asarray(rec, dtype=np.uint32).reshape(1, -1)
    cs = [v(slots[:, 9 * i:9 * i + 9])[0] for i in range(4)]
    return cs, int(rec[36]), int(rec[37])


# ---- the hooks through ctypes (uint32 records; the Context's handle) ---------------------------------------------------------------------
def arith(ctx, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    n = a.shape[0]
    out = np.zeros((n, 9), dtype=np.uint32)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.uint32)
    ctx.check(ctx.lib.gl355_bn254_arith_batch(ctx.h, op, a.ctypes.data_as(C.c_void_p), None if bb is None else bb.ctypes.data_as(C.c_void_p),
                                              out.ctypes.data_as(C.c_void_p), n))
    return out


def chain(ctx, form, operands, steps):
    """steps: (n_chains, n_steps) -> trace (n_chains, n_steps, 40)"""
    ops = np.ascontiguousarray(operands, dtype=np.uint32).reshape(-1, OPND_WORDS)
    st = np.ascontiguousarray(steps, dtype=np.uint32)
    nc, ns = st.shape
    tr = np.zeros((nc, ns, REC_WORDS), dtype=np.uint32)
    ctx.check(ctx.lib.gl355_bn254_g1_chain(ctx.h, form, ops.ctypes.data_as(C.c_void_p), ops.shape[0], st.ctypes.data_as(C.c_void_p), nc, ns,
                                           tr.ctypes.data_as(C.c_void_p)))
    return tr
