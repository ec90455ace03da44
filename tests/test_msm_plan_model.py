"""CPU: the window arithmetic behind the bit-length-planned MSMs (tests/pymodel_msm_plan.py, a restatement of msm_plan, msm_signed_digit and
commit_columns' classing) on its own terms, for every size class lg = 0 .. 26, every max_bits = 0 .. 256, plain and prepared bases: the plan's
signed digits hold every scalar below 2^max_bits with no carry left, the first scalar past them is reported, and a prepared plan never asks for
more windows than its table holds.  (tests/test_gpu_msm_bits.py holds the library to the same model.)"""
import random

import pymodel_msm_plan as mp

_checked = {}


def scalars_below(max_bits, rng):
    top = (1 << max_bits) - 1
    pat5, patA = int("55" * 32, 16), int("AA" * 32, 16)
    return [0, min(1, top), top, pat5 & top, patA & top] + [rng.getrandbits(max_bits) if max_bits else 0 for _ in range(200)]


def check_plan(lg, max_bits, prepared):
    c, wps, one_window, two_level = mp.plan(lg, max_bits, prepared)
    assert 2 <= c <= 22 and wps >= 1 and two_level == int(c > 11)
    assert one_window == int(not prepared and 12 <= max_bits + 1 < (mp.plain_c(lg)))
    if one_window:
        assert (c, wps) == (max_bits + 1, 1) and two_level           # always sorted in two levels
    if prepared:
        assert c == mp.prepared_c(lg) and wps <= mp.table_wps(lg) == 256 // c + 1
    key = (c, wps, max_bits)                                         # the digits depend on the size class through these alone
    if key in _checked:
        return
    _checked[key] = True
    rng = random.Random(0x355 * 1000 + 257 * c + max_bits)
    for k in scalars_below(max_bits, rng):
        digits, over = mp.signed_digits(k, c, wps)
        assert not over and len(digits) == wps and mp.recombine(digits, c) == k, (lg, max_bits, prepared, hex(k))
        assert all(abs(d) <= 1 << (c - 1) for d in digits)
        if one_window:
            assert digits[0] == k                                    # nothing negative, nothing carried
    if wps * c < 256:
        assert mp.signed_digits(1 << (wps * c), c, wps)[1]
        assert mp.signed_digits((1 << 256) - 1, c, wps)[1]
    elif wps * c == 256:                                             # (c divides 256 and the carry window was cut: the top digit may still carry out)
        assert max_bits < 256 and mp.signed_digits(1 << 255, c, wps)[1] and not mp.signed_digits(1 << 254, c, wps)[1]
    else:
        assert not mp.signed_digits((1 << 256) - 1, c, wps)[1]       # every plan this wide: the check can never fire
    if max_bits == 256:
        assert wps * c > 256
    largest = mp.largest(c, wps)                                     # the plan's last scalar
    assert largest >= (1 << max_bits) - 1 and not mp.signed_digits(min(largest, (1 << 256) - 1), c, wps)[1]
    assert largest + 1 >= 1 << 256 or mp.signed_digits(largest + 1, c, wps)[1]
    if one_window:
        assert mp.signed_digits(1 << max_bits, c, wps)[1]            # the carry out of the only window
    bad = mp.unrepresentable(lg, max_bits, prepared)
    assert (bad is None) == (wps * c > 256) and (bad is None or (bad < 1 << 256 and mp.signed_digits(bad, c, wps)[1]))


def test_every_plan_holds_its_scalars():
    for prepared in (False, True):
        for lg in range(27):
            for max_bits in range(257):
                check_plan(lg, max_bits, prepared)
    assert len(_checked) > 3000


def test_plan_values_at_the_sizes_the_gpu_tests_use():
    assert [mp.plain_c(mp.lg_of(n)) for n in (64, 300, 4096, (1 << 14) + 1, 1 << 16, (1 << 18) + 1, (1 << 22) + 1)] == [4, 7, 10, 13, 14, 17, 20]
    assert mp.plan_of((1 << 14) + 1, 11) == [12, 1, 1, 1] and mp.plan_of((1 << 14) + 1, 12) == [13, 2, 0, 1] and mp.plan_of((1 << 14) + 1, 10) == [13, 2, 0, 1]
    assert mp.plan_of(1 << 16, 12) == [13, 1, 1, 1] and mp.plan_of(1 << 16, 13) == [14, 2, 0, 1]
    assert mp.plan_of((1 << 18) + 1, 15) == [16, 1, 1, 1] and mp.plan_of((1 << 18) + 1, 16) == [17, 2, 0, 1]
    assert mp.plan_of((1 << 22) + 1, 16) == [17, 1, 1, 1]            # the product's k = 23 range-check columns
    assert mp.plan_of(4096, 256, True) == [12, 22, 0, 1] and mp.plan_of(4096, 24, True) == [12, 3, 0, 1]
    assert mp.plan_of(300, 256) == [7, 37, 0, 0] and mp.plan_of(300, 0) == [7, 2, 0, 0] and mp.plan_of(300, 7) == [7, 2, 0, 0] and mp.plan_of(300, 8) == [7, 3, 0, 0]
    assert (mp.prepared_c(23), mp.prepared_c(22), mp.prepared_c(20), mp.prepared_c(18)) == (22, 20, 19, 17)      # the widths csrc/bn254_kzg.hip records


def test_column_runs():
    bits = [0, 1, 1, 11, 12, 16, 13, 19, 20, 21, 39, 40, 41, 60, 64, 65, 200] + [253] * 6 + [16] * 17
    runs = mp.column_runs(bits, 1 << 12, False)
    assert runs == [(0, 9, 20, False), (9, 3, 40, False), (12, 2, 60, False), (14, 2, 80, False), (16, 1, 200, False), (17, 5, 256, False), (22, 1, 256, False),
                    (23, 16, 16, False), (39, 1, 16, False)]
    assert [r[3] for r in mp.column_runs(bits, 1 << 12, True)] == [False, True, True, True, True, True, True, False, False]
    assert sum(r[1] for r in runs) == len(bits)
    # a run of short columns gets the longest one's exact length; at 2^23 rows a call takes 16 columns, at 2^26 two
    assert mp.column_runs([12, 16, 5], 1 << 16, True) == [(0, 3, 16, False)]
    assert [r[1] for r in mp.column_runs([16] * 20, 1 << 23, True)] == [16, 4] and [r[1] for r in mp.column_runs([16] * 5, 1 << 26, True)] == [2, 2, 1]
    assert mp.column_runs([0], 8, False) == [(0, 1, 1, False)] and mp.column_runs([254, 254], 8, True) == [(0, 2, 256, True)]
