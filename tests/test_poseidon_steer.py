"""CPU: tests/poseidon_steer.py inverts the rounds it says it inverts -- a steered state, run forward through the naive model, shows the chosen
argument vector at the chosen round, and the oracle-independent permutation of it is the one the naive model gives."""
import random

import poseidon_steer as st

P = st.P


def test_inverse_mds_and_seventh_root():
    ident = st.gpt.mat_mul(st.MDS, st.MDS_INV)
    assert ident == [[int(i == j) for j in range(12)] for i in range(12)]
    rng = random.Random(0x57E)
    for x in [0, 1, P - 1, 1 << 32, (1 << 32) - 1] + [rng.randrange(P) for _ in range(20)]:
        assert pow(pow(x, 7, P), st.D, P) == x and pow(pow(x, st.D, P), 7, P) == x


def test_steered_states_round_trip_at_every_round():
    rng = random.Random(0x57F)
    edges = [0, 1, P - 1, 1 << 32, (1 << 32) - 1, 0xFFFFFFFE00000001 % P]
    for r in range(st.N_ROUNDS):
        for k in range(6):
            arg = [rng.randrange(P) for _ in range(12)]
            arg[0] = edges[k]
            if st.is_full(r):
                arg[5], arg[11] = edges[(k + 1) % 6], edges[(k + 2) % 6]
            state = st.preimage(r, arg)
            assert all(0 <= x < P for x in state)
            assert st.sbox_args(state, r) == arg, (r, k)
    # round 0's argument is the input plus the first constants
    assert st.preimage(0, [0] * 12) == [(-c) % P for c in st.RC[0]]
