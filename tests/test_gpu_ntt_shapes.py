"""Goldilocks NTT / LDE at the shapes the parity tests leave out: column strides above n (the words between columns must keep their
values), batches that fill, overflow and nearly fill the 4096-element tile of the small-row kernels, canonical outputs at every size
from n = 1, and small LDEs with many columns at every supported rate.  Integer arithmetic: every comparison is exact.

The reference is the CPU oracle (orc.ntt / orc.lde / orc.reverse_index_bits); for n <= 64 a direct O(n^2) DFT in Python integers with
omega_n = 7^((p-1)/n) (include/gl355.h) is a second witness.  Which route (csrc/ntt_route.h) each size takes is recorded in
docs/history/ntt_shapes.md and, instance by instance, in docs/history/ntt_route.md."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import P, rand_field

pytestmark = pytest.mark.gpu

U64 = np.uint64
SHIFTS = (7, 0x123456789ABCDEF)
# name -> (inverse, shift)
DIRECTIONS = [("fft", False, None), ("ifft", True, None)] + [("coset_fft %x" % s, False, s) for s in SHIFTS] + \
             [("coset_ifft %x" % s, True, s) for s in SHIFTS]
FOUR = DIRECTIONS[:3] + DIRECTIONS[4:5]          # forward, inverse, coset forward and coset inverse at shift 7
HASH_KAT = 0xD110AA6A46373941                    # hash_no_pad(1..8)[0], as in test_error_codes


def eq(a, b, what=""):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: mismatch at %d/%d positions, first %s: got %x want %x" % (
            what, len(bad), a.size, bad[0], int(a[tuple(bad[0])]), int(b[tuple(bad[0])])))


def dft(col, inverse=False, shift=None):
    """one column, directly from the definition, in Python integers"""
    x = [int(v) % P for v in col]
    n = len(x)
    w = pow(7, (P - 1) // n, P)
    s = 1 if shift is None else shift % P
    if inverse:
        w, s = pow(w, P - 2, P), pow(s, P - 2, P)
    wp = [pow(w, k, P) for k in range(n)]
    if not inverse:
        x = [v * pow(s, i, P) % P for i, v in enumerate(x)]
    y = [sum(v * wp[i * j % n] for i, v in enumerate(x)) % P for j in range(n)]
    if inverse:
        ninv = pow(n, P - 2, P)
        y = [v * ninv * pow(s, j, P) % P for j, v in enumerate(y)]
    return np.array(y, dtype=U64)


def dft_cols(x, inverse, shift):
    return np.stack([dft(c, inverse, shift) for c in x])


def sentinel(batch, stride):
    """[batch][stride] words, all distinct; two of three are non-canonical (0xFFFFFFFF........ with a non-zero low half is >= p)"""
    idx = np.arange(batch * stride, dtype=U64).reshape(batch, stride)
    return np.where(idx % U64(3) != 0, U64(0xFFFFFFFFA5A5A5A5), U64(0xA5A5A5A5A5A5A5A5)) ^ idx


def reduce_p(x):
    x = np.asarray(x, dtype=U64)
    return np.where(x >= U64(P), x - U64(P), x)


# ---- 1. strided columns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 3, 12, 13, 14, 15, 16])
def test_strided_columns(ctx, orc, log_n):
    """gl355_ntt / gl355_coset_ntt with stride > n: the first n words of each row are the oracle's transform of that column, and the
    stride - n words behind them come back bit for bit.  Sizes: small rows (1, 3), one full tile (12), the single-pass 64 / 128 KB
    tiles (13, 14) and the first two two-pass sizes (15, 16: forward = two column passes through scratch; coset forward = columns,
    rows, in-place bit reversal; inverse = bit reversal, rows, columns)."""
    n = 1 << log_n
    rng = np.random.default_rng(0x5710 + log_n)
    x = rand_field(rng, (5, n))
    want = {name: orc.ntt(x, inverse=inv, shift=s) for name, inv, s in DIRECTIONS}
    if n <= 64:
        for name, inv, s in DIRECTIONS:
            eq(want[name], dft_cols(x, inv, s), "oracle vs direct DFT, %s" % name)
    wrong = []                                              # every call is checked, so a failure lists the forms that are wrong
    for batch in (1, 2, 5):
        for stride in sorted({n + 1, n + 8, 2 * n}):
            buf = sentinel(batch, stride)
            pad = buf[:, n:].copy()
            assert (pad >= U64(P)).any() and len(np.unique(pad)) == pad.size
            buf[:, :n] = x[:batch]
            for name, inv, s in DIRECTIONS:
                what = "log_n %d batch %d stride %d %s" % (log_n, batch, stride, name)
                got = ctx.fft(buf, inverse=inv, shift=s, stride=stride, log_n=log_n)
                for part, g, w in (("columns", got[:, :n], want[name][:batch]), ("padding", got[:, n:], pad)):
                    try:
                        eq(g, w, what + ", " + part)
                    except AssertionError as e:
                        wrong.append(str(e))
    assert not wrong, "%d wrong results:\n%s" % (len(wrong), "\n".join(wrong))


# ---- 2. tile edges of the small-row kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(1, 13))
def test_batch_fills_tiles(ctx, orc, log_n):
    """n < 4096: rpt = 4096 / n transforms share one LDS tile and the last tile is guarded by row < total_rows.  One column, an exactly
    full tile, the first row of a second tile, a short last tile after two full ones; n = 4096: seven whole tiles."""
    n, rpt = 1 << log_n, 4096 >> log_n
    batches = [7] if log_n == 12 else sorted({1, rpt, rpt + 1, 3 * rpt - 1})
    rng = np.random.default_rng(0x5720 + log_n)
    x = rand_field(rng, (max(batches), n))
    probe = sorted({0, min(rpt, len(x)) - 1, min(rpt, len(x) - 1), len(x) - 1})
    for name, inv, s in FOUR:
        want = orc.ntt(x, inverse=inv, shift=s)
        if n <= 64:
            eq(want[probe], dft_cols(x[probe], inv, s), "oracle vs direct DFT, %s" % name)
        for batch in batches:
            eq(ctx.fft(x[:batch], inverse=inv, shift=s), want[:batch], "log_n %d batch %d %s" % (log_n, batch, name))


# ---- 3. canonical outputs, n = 1 included -----------------------------------------------------------------------------------------
def edge_columns(rng, n):
    """three columns: the edge words in turn; random words of [p, 2^64); random words of the whole u64 range"""
    edges = np.array([(1 << 64) - 1, P, P + 1, 0xFFFFFFFF00000000], dtype=U64)
    return np.stack([np.resize(edges, n),
                     U64(0xFFFFFFFF00000000) | rng.integers(1, 1 << 32, n, dtype=U64),
                     rng.integers(0, 1 << 64, n, dtype=U64)])


@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 11, 12, 13, 14, 15, 17])
def test_outputs_are_canonical_at_every_size(ctx, orc, log_n):
    """include/gl355.h: inputs may be any u64, every output word is < p.  At the parent commit n = 1 returned its input untouched:
    'log_n 0 fft, set 0: mismatch at 2/3 positions, first [0 0]: got ffffffffffffffff want fffffffe'."""
    n = 1 << log_n
    rng = np.random.default_rng(0x5730 + log_n)
    sets = [edge_columns(rng, n)]
    if n == 1:
        sets.append(np.array([[P], [P + 1], [0xFFFFFFFF00000000]], dtype=U64))
    for k, x in enumerate(sets):
        assert (x[:2] >= U64(P - 1)).all()              # nothing but edges and non-canonical words in the first two columns
        xr = reduce_p(x)
        for name, inv, s in FOUR:
            what = "log_n %d %s, set %d" % (log_n, name, k)
            want = orc.ntt(xr, inverse=inv, shift=s)
            if n <= 64:
                eq(want, dft_cols(x, inv, s), "oracle vs direct DFT, " + what)
            got = ctx.fft(x, inverse=inv, shift=s)
            eq(got, want, what)
            assert (got < U64(P)).all(), what
            if n == 1:
                buf = sentinel(3, 3)
                pad = buf[:, 1:].copy()
                buf[:, :1] = x
                got = ctx.fft(buf, inverse=inv, shift=s, stride=3, log_n=0)
                eq(got[:, :1], want, what + ", stride 3, columns")
                eq(got[:, 1:], pad, what + ", stride 3, padding")


# ---- 4. LDE: small sizes, many columns, every rate --------------------------------------------------------------------------------
def lde_direct(col, rate_bits, shift):
    n, N = len(col), len(col) << rate_bits
    g = pow(7, (P - 1) // N, P)
    pts = [shift * pow(g, j, P) % P for j in range(N)]
    c = [int(v) for v in col]
    return np.array([sum(v * pow(z, i, P) for i, v in enumerate(c)) % P for z in pts], dtype=U64)


@pytest.mark.parametrize("rate_bits", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 11, 12])
def test_lde_small_sizes_many_columns(gl, ctx, orc, log_n, rate_bits):
    """one column more than a tile of the small-row kernels holds (at most 300), 1 to 16 cosets, natural and bit-reversed output; at
    (6, 2) and (12, 4) two shifts alternate twice on one fresh context, so each is served once cold and once from the table cache"""
    batch = min((4096 >> log_n) + 1, 300)
    rng = np.random.default_rng(0x5740 + 8 * log_n + rate_bits)
    c = rand_field(rng, (batch, 1 << log_n))
    want = orc.lde(c, rate_bits)
    if log_n <= 6:
        for col in (0, batch - 1):
            eq(want[col], lde_direct(c[col], rate_bits, 7), "oracle vs direct evaluation, column %d" % col)
    eq(ctx.lde(c, rate_bits), want, "natural")
    eq(ctx.lde(c, rate_bits, bitrev=True), orc.reverse_index_bits(want.T.copy()).T, "bit-reversed")
    if (log_n, rate_bits) in ((6, 2), (12, 4)):
        wants = {7: want, 49: orc.lde(c, rate_bits, shift=49)}
        c2 = gl.Context(0)
        try:
            for shift in (7, 49, 7, 49):
                eq(c2.lde(c, rate_bits, shift=shift), wants[shift], "shift %d natural" % shift)
                eq(c2.lde(c, rate_bits, shift=shift, bitrev=True), orc.reverse_index_bits(wants[shift].T.copy()).T,
                   "shift %d bit-reversed" % shift)
        finally:
            c2.close()


# the kernel instances of the route table (csrc/ntt_route.h) that no other case reaches, each at the smallest shape that does
# (docs/history/ntt_route.md has the instance of every case): radix-8 columns with a pre table over 4, 64, 128 and 256 points (one coset),
# general radix-16 columns over 64 points (16 cosets: the full pre tables would pass 2^21 words), all-cosets radix-8 columns over 256 points
@pytest.mark.parametrize("log_n,rate_bits", [(14, 0), (18, 0), (19, 0), (20, 0), (18, 4), (20, 1)])
def test_lde_column_kernels_without_another_case(ctx, orc, log_n, rate_bits):
    rng = np.random.default_rng(0x5760 + 8 * log_n + rate_bits)
    c = rand_field(rng, (2, 1 << log_n))
    want = orc.lde(c, rate_bits)
    eq(ctx.lde(c, rate_bits), want, "natural")
    eq(ctx.lde(c, rate_bits, bitrev=True), orc.reverse_index_bits(want.T.copy()).T, "bit-reversed")


def test_inverse_2p19(ctx, orc):
    """the only size whose inverse has a 128-point column pass (general radix-16 columns, step twiddle at the load)"""
    rng = np.random.default_rng(0x5761)
    x = rand_field(rng, (2, 1 << 19))
    eq(ctx.ifft(x), orc.ntt(x, inverse=True), "inverse")


def test_ntt_lde_refusals(ctx):
    """unsupported or inconsistent shapes come back as codes whose message names the unit, and the context stays usable"""
    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def refused(rc, code, unit):
        assert rc == code, (rc, code)
        msg = (ctx.lib.gl355_last_error(ctx.h) or b"").decode()
        assert msg.startswith(unit + ":"), msg
        assert ctx.hash_no_pad(np.arange(1, 9, dtype=U64))[0] == HASH_KAT

    lib, h = ctx.lib, ctx.h
    c, out = np.ones((1, 4), dtype=U64), np.zeros((1, 4 << 5), dtype=U64)
    refused(lib.gl355_lde(h, vp(c), 2, 5, 7, 1, vp(out)), -5, "lde")           # 32 cosets
    refused(lib.gl355_lde(h, vp(c), 0, 1, 7, 1, vp(out)), -5, "lde")           # constants
    d = np.ones((2, 8), dtype=U64)
    refused(lib.gl355_ntt(h, vp(d), 3, 2, 7, 0), -1, "ntt")                    # stride = n - 1
    refused(lib.gl355_ntt(h, vp(d), 25, 1, 1 << 25, 0), -5, "ntt")             # refused before the buffer is looked at
    assert (d == 1).all() and (out == 0).all()
    assert lib.gl355_ntt(h, None, 3, 0, 8, 0) == 0                             # nothing to do
    assert ctx.hash_no_pad(np.arange(1, 9, dtype=U64))[0] == HASH_KAT


# ---- 5. a device-resident view with a row pitch -----------------------------------------------------------------------------------
def test_device_tensor_with_row_pitch(ctx, orc):
    """a torch tensor [4][2^13 + 64] used in place: forward equals the oracle, inverse brings the input back, the 64 trailing words
    of each row never change"""
    import torch
    n, stride = 1 << 13, (1 << 13) + 64
    rng = np.random.default_rng(0x5750)
    x = rand_field(rng, (4, n))
    buf = sentinel(4, stride)
    pad = buf[:, n:].copy()
    buf[:, :n] = x
    t = torch.from_numpy(buf.view(np.int64)).cuda()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.gl355_ntt(ctx.h, C.c_void_p(t.data_ptr()), 13, 4, stride, 0))
    ctx.sync()
    fwd = t.cpu().numpy().view(U64)
    eq(fwd[:, :n], orc.ntt(x), "forward")
    eq(fwd[:, n:], pad, "padding after forward")
    ctx.check(ctx.lib.gl355_ntt(ctx.h, C.c_void_p(t.data_ptr()), 13, 4, stride, 1))
    ctx.sync()
    back = t.cpu().numpy().view(U64)
    eq(back[:, :n], x, "round trip")
    eq(back[:, n:], pad, "padding after inverse")
