"""Part 1 of the Halo2 verifier circuit: every Merkle opening of a plonky2 proof's FRI query rounds, verified in circuit against
its caps under Bn254PoseidonHash, recorded over the chips of halo2_goldilocks.py.

  the proof's shape                 types/proof.rs:317-403 (caps, openings, the FRI proof), types/fri.rs:50-73 (query rounds, steps)
  the Merkle calls and the indices  chip/fri_chip.rs:72-110 (cap index, the four initial trees), :228-327 (check_consistency: to_bits on the
                                    index, one proof per layer with the index shifted by the layer's arity bits)

The input vector is the flat proof of gl355_prove (include/gl355.h; plonk.parse_proof reads the same layout) followed by the circuit's
constants_sigmas cap, which the proof does not carry.  The caps and the query indices are exposed through the instance column, caps first: the
circuit is sound on its own until part 2's transcript derives them.  The arithmetic of batch_initial_polynomials / next_eval, the transcript and
the gate constraints are part 2 and reuse the recorder and the tape unchanged."""
import numpy as np

from . import halo2_goldilocks as hg

SALT_SIZE = 4


class FriOpeningsCircuit:
    def __init__(self, common_data):
        cd = common_data
        self.cd = cd
        assert cd["hasher"] == 1, "the circuit hashes with Bn254PoseidonHash"
        self.arity_bits = [int(a) for a in cd["arity_bits"]]
        assert all(a == 1 for a in self.arity_bits), "the flat proof holds one evaluation pair per layer (arity 2)"
        self.cap_height, self.n_cap = cd["cap_height"], 1 << cd["cap_height"]
        self.lde_bits = cd["degree_bits"] + cd["rate_bits"]
        self.n_queries, self.n_layers = cd["num_query_rounds"], len(self.arity_bits)
        nch, zk = cd["num_challenges"], bool(cd["hiding"])
        n_const = cd["num_selectors"] + cd["num_constants"]
        widths = [n_const + cd["num_routed_wires"], cd["num_wires"], nch * (1 + cd["num_partial_products"]), nch * cd["quotient_degree_factor"]]
        self.leaf_len = [w + (SALT_SIZE if (zk and o > 0) else 0) for o, w in enumerate(widths)]
        # positions in the flat proof, in the order plonk.parse_proof reads them
        pos = [8]

        def take(count):
            pos[0] += count
            return list(range(pos[0] - count, pos[0]))
        cap = lambda: [take(4) for _ in range(self.n_cap)]                                           # noqa: E731
        proof_caps = [cap() for _ in range(3)]                                                         # wires, zs and partial products, quotient
        n_openings = n_const + cd["num_routed_wires"] + cd["num_wires"] + nch * (2 + cd["num_partial_products"] + cd["quotient_degree_factor"])
        take(2 * n_openings)
        self.layer_caps = [cap() for _ in range(self.n_layers)]
        take(2 * ((1 << cd["degree_bits"]) >> self.n_layers) + 1)                                     # the final polynomial, the proof-of-work witness
        depth0 = self.lde_bits - self.cap_height
        self.queries = []
        for _ in range(self.n_queries):
            index = take(1)[0]
            initial = [(take(ll), [take(4) for _ in range(depth0)]) for ll in self.leaf_len]
            steps = []
            depth = depth0
            for a in self.arity_bits:
                depth -= a
                steps.append((take(4), [take(4) for _ in range(depth)]))
            self.queries.append((index, initial, steps))
        self.proof_words = pos[0]
        self.initial_caps = [cap()] + proof_caps                                                      # constants_sigmas first (fri_chip.rs:94-97 zips in oracle order)
        self.n_inputs = pos[0]
        self.round_rows = []

    def inputs(self, flat):
        """the input vector of one proof: its flat words, then the constants_sigmas cap"""
        flat = np.ascontiguousarray(flat, dtype=np.uint64).reshape(-1)
        assert flat.size == self.proof_words == int(flat[0]), "not a proof of this circuit"
        out = np.concatenate([flat, np.asarray(self.cd["constants_sigmas_cap"], dtype=np.uint64).reshape(-1)])
        assert out.size == self.n_inputs
        return out

    def record(self, inputs, min_k=17):
        """-> the Recorder of the circuit (layout, tape, eager values from `inputs`) at the smallest k that holds its rows and the 16-bit range
        table; round_rows[i] is the half-open row range of query round i"""
        rec = hg.Recorder(28, inputs)
        g = hg.GoldilocksChip(rec)
        ar = g.arithmetic_chip
        g.load_table()
        value = lambda words: [g.assign_value(hg.Input(w)) for w in words]                            # noqa: E731
        initial_caps = [[value(h) for h in cap] for cap in self.initial_caps]
        layer_caps = [[value(h) for h in cap] for cap in self.layer_caps]
        public = [c for cap in initial_caps + layer_caps for h in cap for c in h]
        self.round_rows = []
        for index_word, initial, steps in self.queries:
            start = rec.offset
            x_index = g.assign_value(hg.Input(index_word))
            public.append(x_index)
            initial = [(value(leaf), [value(s) for s in siblings]) for leaf, siblings in initial]
            steps = [(value(evals), [value(s) for s in siblings]) for evals, siblings in steps]
            x_index_bits = g.to_bits(x_index, 64)[:self.lde_bits]                                     # fri_chip.rs:245-250
            cap_index = g.from_bits(x_index_bits[len(x_index_bits) - self.cap_height:])               # calculate_cap_index, :72-82
            merkle = hg.MerkleProofChip(rec)
            for (leaf, siblings), cap in zip(initial, initial_caps):                                  # verify_initial_merkle_proof, :85-110
                merkle.verify_merkle_proof_to_cap_with_cap_index(leaf, x_index_bits, cap_index, cap, siblings)
            for i, arity_bits in enumerate(self.arity_bits):                                          # :275-316
                coset_index_bits = x_index_bits[arity_bits:]
                evals, siblings = steps[i]
                hg.MerkleProofChip(rec).verify_merkle_proof_to_cap_with_cap_index(evals, coset_index_bits, cap_index, layer_caps[i], siblings)
                x_index_bits = coset_index_bits
            self.round_rows.append((start, rec.offset))
        for row, cell in enumerate(public):
            ar.expose_public(cell, row)
        rec.shrink_to_fit(min_k)
        return rec
