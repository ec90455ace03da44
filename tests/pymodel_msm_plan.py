"""Restatement in Python integers of the arithmetic that turns a bit length into an MSM configuration: msm_plan's windows (csrc/bn254_msm.hip; the
prepared bases' window width from csrc/bn254_kzg.hip), msm_signed_digit, and the classing of commit_columns (csrc/plonk_bn254.hip).  Nothing is
shared with the library: tests/test_msm_plan_model.py checks the arithmetic on its own, tests/test_gpu_msm_bits.py holds the library to it."""
MSM_FINE_BITS = 10


def lg_of(n):
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return lg


def plain_c(lg):
    return 4 if lg <= 6 else (lg - 2 if lg <= 18 else (17 if lg <= 22 else 20))


def prepared_c(lg):
    for c in range(min(22, max(13, lg) - 1), 12, -1):
        if 254 - c * (253 // c) >= (c + 2) // 3:
            return c
    return 12


def table_wps(lg):
    """windows a prepared table holds (gl355_bn254_g1_msm_prepare)"""
    return 256 // prepared_c(lg) + 1


def plan(lg, max_bits, prepared=False):
    """[c, wps, one_window, two_level] as gl355_bn254_g1_msm_bits reports them"""
    c = prepared_c(lg) if prepared else plain_c(lg)
    one_window = (not prepared) and max_bits + 1 < c and max_bits + 1 >= 12
    if one_window:
        c = max_bits + 1
    wps = 256 // c + 1
    if max_bits < 256:
        wps = min(wps, (max(1, max_bits) + c - 1) // c + 1)
    if one_window:
        wps = 1
    return [c, wps, int(one_window), int(c - 1 > MSM_FINE_BITS)]


def plan_of(n, max_bits, prepared=False):
    return plan(lg_of(n), max_bits, prepared)


def signed_digits(k, c, wps):
    """the wps signed digits of c bits msm_signed_digit gives for the 256-bit scalar k (|digit| <= 2^(c-1)), and whether they fail to hold k:
    a carry left after the last window, or bits of k at and above wps * c"""
    digits, carry = [], 0
    for w in range(wps):
        raw = ((k >> (w * c)) & ((1 << c) - 1) if w * c < 256 else 0) + carry
        carry = int(raw >= 1 << (c - 1))
        digits.append(raw - (carry << c))
    return digits, bool(carry) or (wps * c < 256 and (k >> (wps * c)) != 0)


def recombine(digits, c):
    return sum(d << (c * w) for w, d in enumerate(digits))


def largest(c, wps):
    """the largest scalar wps signed digits of c bits hold: every digit 2^(c-1) - 1 (a raw digit of 2^(c-1) already turns negative and carries)"""
    return recombine([(1 << (c - 1)) - 1] * wps, c)


def unrepresentable(lg, max_bits, prepared=False):
    """one scalar below 2^256 that the plan's digits cannot hold, or None when every 256-bit scalar fits"""
    c, wps, one_window, _ = plan(lg, max_bits, prepared)
    if one_window:
        return 1 << max_bits
    if wps * c < 256:
        return 1 << (wps * c)
    return 1 << 255 if wps * c == 256 else None        # 256 bits of digits and no carry window: a top digit of 2^(c-1) carries out


def column_runs(bits, n, have_tables):
    """commit_columns' MSM calls over columns of the given measured bit lengths (0 = an all-zero column): (first column, columns, max_bits, prepared)"""
    per = max(1, min(16, (1 << 27) // n))
    nbits = [max(1, b) for b in bits]
    cls = [(b + 19) // 20 for b in nbits]
    runs, s0 = [], 0
    while s0 < len(bits):
        max_m = max(1, 72 // (cls[s0] + 1))
        m = 1
        while s0 + m < len(bits) and m < per and m < max_m and cls[s0 + m] == cls[s0]:
            m += 1
        wide = cls[s0] >= 2
        runs.append((s0, m, min(256, 20 * cls[s0]) if wide else max(nbits[s0:s0 + m]), bool(have_tables and wide)))
        s0 += m
    return runs
