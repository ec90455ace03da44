"""Steering a Poseidon round's S-box by inverting the rounds before it (pure Python over tools/gen_poseidon_tables.py).

preimage(r, arg) is the input state for which the state after round r's constants -- the argument vector of round r's S-boxes -- is `arg`.  Rounds
r - 1 .. 0 are undone one by one: subtract the constants of the round that follows, multiply by the inverse MDS matrix (Gaussian elimination mod p),
take the 7th root x^D, D = 7^-1 mod (p - 1), of every word of a full round and of word 0 of a partial round."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_poseidon_tables as gpt  # noqa: E402

P = gpt.P
N_ROUNDS = 2 * gpt.HALF_F + gpt.R_P
D = pow(7, -1, P - 1)
assert D == 10540996611094048183
RC = gpt.load_rc()
MDS = gpt.mds_matrix()
MDS_INV = gpt.mat_inv(MDS)


def is_full(r):
    return r < gpt.HALF_F or r >= gpt.HALF_F + gpt.R_P


def sbox_args(state, r):
    """the state after round r's constants, by the naive model run forward"""
    s = [x % P for x in state]
    for q in range(r + 1):
        s = [(x + c) % P for x, c in zip(s, RC[q])]
        if q == r:
            return s
        s = [gpt.sbox(x) for x in s] if is_full(q) else [gpt.sbox(s[0])] + s[1:]
        s = gpt.mat_vec(MDS, s)


def preimage(r, arg):
    s = [x % P for x in arg]
    for q in range(r - 1, -1, -1):
        s = gpt.mat_vec(MDS_INV, [(x - c) % P for x, c in zip(s, RC[q + 1])])      # the S-box outputs of round q
        s = [pow(x, D, P) for x in s] if is_full(q) else [pow(s[0], D, P)] + s[1:]
    return [(x - c) % P for x, c in zip(s, RC[0])]
