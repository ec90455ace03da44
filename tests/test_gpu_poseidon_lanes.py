"""The 16-lane Poseidon permutation (psd_permute_lanes<0> and <3>, poseidon_lanes.cuh) through the test hook gl355_poseidon_permute_lanes, against
the oracle's naive permutation.  The product paths reach it only through Merkle nodes (eight pseudo-random digest words, capacity zero) and FRI leaves.

Two sets of states:
  * the 65 536 patterned states of test_poseidon_permute_many_states (whole u64 range, non-canonical words, empty / saturated halves, lone and empty
    word 0), also at counts that leave a wave partly filled;
  * steered states (tests/poseidon_steer.py): for every round, states whose S-box argument at that round is an edge value of the product's carry chain.
    Steering pins the FIRST product of the chosen S-box -- gl_mul_fill(s, s) in form 3's rounds 4..25, the first square of psd_sbox elsewhere -- and
    everything downstream of an edge value in the hand-scheduled round (the MDS row inside the S-box, the recombination).  The LATER products of that
    S-box see x^2, x^3 and x^4 of the edge value, which are not edges: those are pinned by tests/test_gpu_gl_arith.py, not here.
The steered states also go through the one-lane block form (gl355_poseidon_permute), which no other test steers either."""
import numpy as np
import pytest

import poseidon_steer as st
from test_gpu_gl_arith import family_v, mul_events

gpu = pytest.mark.gpu          # the condition of the steered set is checked without a GPU too

P = st.P
EVENTS = ("middle carry", "borrow", "final carry")


def eq(a, b, what):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError("%s: %d of %d words differ, first at %s: got %x want %x" % (what, len(bad), a.size, bad[0], int(a[tuple(bad[0])]), int(b[tuple(bad[0])])))


@pytest.fixture(scope="module")
def patterned(orc):
    """the states of test_poseidon_permute_many_states and their permutation"""
    rng = np.random.default_rng(0x3A6)
    s = rng.integers(0, 1 << 64, (1 << 16, 12), dtype=np.uint64)
    s[:4096] &= np.uint64(0xFFFFFFFF00000000)
    s[4096:8192] |= np.uint64(0x00000000FFFFFFFF)
    s[8192:12288, 1:] = 0
    s[12288:16384, 0] = 0
    want = orc.permute(s)
    s.setflags(write=False)
    want.setflags(write=False)
    return s, want


def steer_values():
    """S: the values of V mod p that are >= 2^32 and whose square fires a carry step, and 0, 1, p - 1.  None of those squares carries out of the middle sum
    (the members of V that do are all >= p and reduce below 2^32), so p - 1 - 2^k, k < 32, are added: high word 2^32 - 2, low word 2^32 - 2^k"""
    s = {v % P for v in family_v() if v % P >= 1 << 32 and any(mul_events(v % P, v % P))} | {0, 1, P - 1}
    return sorted(s | {P - 1 - (1 << k) for k in range(32)})


@pytest.fixture(scope="module")
def steered(orc):
    """(round of each state, its steered words, argument vectors, states, their permutation): S at word 0 of every round, a 16-value subset of S at words 5 and 11 of the full rounds,
    the other words seeded random"""
    import random
    rng = random.Random(0x57A)
    s_vals = steer_values()
    sub = s_vals[::max(1, len(s_vals) // 16)][:16]
    assert len(sub) == 16
    rounds, words, args = [], [], []
    for r in range(st.N_ROUNDS):
        for x in s_vals:
            arg = [rng.randrange(P) for _ in range(12)]
            arg[0] = x
            rounds.append(r)
            words.append((0,))
            args.append(arg)
        if st.is_full(r):
            for i in range(16):
                arg = [rng.randrange(P) for _ in range(12)]
                arg[5], arg[11] = sub[i], sub[(i + 5) % 16]
                rounds.append(r)
                words.append((5, 11))
                args.append(arg)
    states = np.array([st.preimage(r, a) for r, a in zip(rounds, args)], dtype=np.uint64)
    want = orc.permute(states)
    states.setflags(write=False)
    want.setflags(write=False)
    return rounds, words, args, states, want


def test_every_round_meets_every_carry_step(steered):
    """the condition of the steered set: at least 16 states per (round, step), counted on the canonical argument at the state's steered words; arguments below
    2^32 - 1 do not count, the device may hold them as x + p"""
    rounds, words, args, states, _ = steered
    count = np.zeros((st.N_ROUNDS, 3), dtype=int)
    for r, ws, a in zip(rounds, words, args):
        count[r] += np.array([mul_events(a[w], a[w]) for w in ws if a[w] >= (1 << 32) - 1] + [(0, 0, 0)]).any(axis=0)
    print("steered states: %d, per round %s" % (len(rounds), sorted(set(np.bincount(rounds).tolist()))))
    print("states per (round, step), minimum over the rounds: %s" % dict(zip(EVENTS, count.min(axis=0).tolist())))
    assert (count >= 16).all(), count
    # and the steering itself, on a sample: the naive model shows the argument at the round
    for i in range(0, len(rounds), 97):
        assert st.sbox_args(states[i].tolist(), rounds[i]) == args[i]


@gpu
@pytest.mark.parametrize("form", [0, 3])
def test_lane_forms_on_patterned_states(ctx, patterned, form):
    s, want = patterned
    eq(ctx.poseidon_permute_lanes(form, s), want, "form %d, all states" % form)
    for count in (1, 3, 4, 5, 63, 65):          # waves with empty groups: those clamp to state 0 and store nothing
        eq(ctx.poseidon_permute_lanes(form, s[-count:]), want[-count:], "form %d, %d states" % (form, count))


@gpu
def test_a_group_past_the_end_stores_nothing(ctx, patterned):
    """five states in a buffer of eight: the three groups of the second block that have no state leave the words behind the fifth alone"""
    s, want = patterned
    import torch
    for form in (0, 3):
        buf = torch.from_numpy(s[:8].astype(np.int64)).to("cuda:0")
        torch.cuda.synchronize()            # a device buffer is used in place, on the context's own stream
        ctx.check(ctx.lib.gl355_poseidon_permute_lanes(ctx.h, form, buf.data_ptr(), 5))
        ctx.sync()
        got = buf.cpu().numpy().astype(np.uint64)
        eq(got[:5], want[:5], "form %d" % form)
        eq(got[5:], s[5:8], "form %d, behind the end" % form)


@gpu
@pytest.mark.parametrize("form", [0, 3, "block"])
def test_steered_states(ctx, steered, form):
    _, _, _, states, want = steered
    got = ctx.poseidon_permute(states) if form == "block" else ctx.poseidon_permute_lanes(form, states)
    eq(got, want, "form %s" % form)
