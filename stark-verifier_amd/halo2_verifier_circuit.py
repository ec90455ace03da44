"""The Halo2 verifier circuit, recorded over the chips of halo2_goldilocks.py.

FriOpeningsCircuit (part 1): every Merkle opening of a plonky2 proof's FRI query rounds, verified in circuit against its caps under
Bn254PoseidonHash.

  the proof's shape                 types/proof.rs:317-403 (caps, openings, the FRI proof), types/fri.rs:50-73 (query rounds, steps)
  the Merkle calls and the indices  chip/fri_chip.rs:72-110 (cap index, the four initial trees), :228-327 (check_consistency: to_bits on the
                                    index, one proof per layer with the index shifted by the layer's arity bits)

The input vector is the flat proof of gl355_prove (include/gl355.h; plonk.parse_proof reads the same layout) followed by the circuit's
constants_sigmas cap, which the proof does not carry.  The caps and the query indices are exposed through the instance column, caps first: the
circuit is sound on its own until part 2's transcript derives them.  The arithmetic of batch_initial_polynomials / next_eval, the transcript and
the gate constraints come after it.

FriVerifierCircuit (part 2): the reference's get_challenges followed by FriVerifierChip::verify_fri_proof, i.e. the transcript derives alpha, the
betas, the proof-of-work response and the query indices from the proof itself, and the committed polynomials are proved to open to the claimed
values at zeta and g zeta.

  the order of assignment           verifier_circuit.rs:81-127 (assign_proof_with_pis, assign_verification_key), types/proof.rs:58-109, :237-280,
                                    :345-377 (openings; a round's evaluations before its Merkle proofs; caps, rounds, final polynomial, witness)
  the challenges                    chip/plonk/plonk_verifier_chip.rs:55-154
  FRI                               chip/plonk/plonk_verifier_chip.rs:212-240, chip/fri_chip.rs:329-376

Plonky2VerifierCircuit (part 3): the whole of Verifier::synthesize.  The public inputs are the instances and are hashed in circuit
(PublicInputsHasherChip), the plonk betas, gammas and alphas are kept, eval_vanishing_poly with the 12 gate constrainers gives the vanishing
polynomial at zeta, the quotient identity is asserted, and FRI follows: a Halo2 proof over this circuit proves that the plonky2 proof verifies.

  the order of synthesis            verifier_circuit.rs:148-200
  the public-inputs hash            chip/plonk/plonk_verifier_chip.rs:42-53, chip/public_inputs_hasher_chip.rs
  the vanishing identity            chip/plonk/plonk_verifier_chip.rs:156-210, chip/plonk/vanishing_poly.rs, chip/plonk/gates/ (halo2_plonk_chips.py)

The two earlier circuits stay as recorded artifacts may depend on them; the three share the helpers of FriVerifierCircuit."""
import numpy as np

from . import halo2_goldilocks as hg
from . import halo2_plonk_chips as hp

SALT_SIZE = 4


class FriOpeningsCircuit:
    def __init__(self, common_data):
        cd = common_data
        self.cd = cd
        assert cd["hasher"] == 1, "the circuit hashes with Bn254PoseidonHash"
        self.arity_bits = [int(a) for a in cd["arity_bits"]]
        if any(a != 1 for a in self.arity_bits):      # as the reference's FriChip (fri_chip.rs:211)
            raise ValueError("the Halo2 verifier circuit supports arity-2 FRI only (reduction_arity_bits = 1), not %r" % (self.arity_bits,))
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


class FriVerifierCircuit:
    """The input vector is the flat proof of gl355_prove followed by the four words of the public-inputs hash; the circuit digest and the
    constants_sigmas cap are constants of the recording (they are fixed per plonky2 circuit, and so is the recording).  Neither the proof's
    stored index words nor a stored proof-of-work response are read: both come out of the transcript."""

    def __init__(self, common_data):
        cd = common_data
        self.cd = cd
        shape = FriOpeningsCircuit(cd)                                # the positions of the flat proof's parts
        self.arity_bits, self.cap_height, self.n_cap, self.lde_bits = shape.arity_bits, shape.cap_height, shape.n_cap, shape.lde_bits
        self.n_queries, self.n_layers, self.leaf_len = shape.n_queries, shape.n_layers, shape.leaf_len
        self.proof_caps, self.layer_caps, self.queries, self.proof_words = shape.initial_caps[1:], shape.layer_caps, shape.queries, shape.proof_words
        nch = self.nch = cd["num_challenges"]
        n_const = cd["num_selectors"] + cd["num_constants"]
        self.widths = [n_const + cd["num_routed_wires"], cd["num_wires"], nch * (1 + cd["num_partial_products"]), nch * cd["quotient_degree_factor"]]
        pos = self.proof_caps[-1][-1][-1] + 1                        # the openings follow the three caps, in plonk.parse_proof's order
        self.openings = {}
        for name, count in (("constants", n_const), ("plonk_sigmas", cd["num_routed_wires"]), ("wires", cd["num_wires"]), ("plonk_zs", nch),
                            ("partial_products", nch * cd["num_partial_products"]), ("quotient_polys", nch * cd["quotient_degree_factor"]), ("plonk_zs_next", nch)):
            self.openings[name] = [[pos + 2 * i, pos + 2 * i + 1] for i in range(count)]
            pos += 2 * count
        assert pos == self.layer_caps[0][0][0] if self.n_layers else True
        pos += 4 * self.n_cap * self.n_layers
        n_final = (1 << cd["degree_bits"]) >> self.n_layers
        self.final_poly = [[pos + 2 * i, pos + 2 * i + 1] for i in range(n_final)]
        self.pow_witness = pos + 2 * n_final
        assert self.pow_witness + 1 == self.queries[0][0]
        self.pi_hash = list(range(self.proof_words, self.proof_words + 4))
        self.n_inputs = self.proof_words + 4
        self.round_rows, self.challenge_cells = [], {}

    def inputs(self, flat, public_inputs_hash):
        flat = np.ascontiguousarray(flat, dtype=np.uint64).reshape(-1)
        assert flat.size == self.proof_words == int(flat[0]), "not a proof of this circuit"
        out = np.concatenate([flat, np.asarray(public_inputs_hash, dtype=np.uint64).reshape(-1)])
        assert out.size == self.n_inputs
        return out

    # ---- the parts of Verifier::synthesize that FriVerifierCircuit and Plonky2VerifierCircuit share ----
    def _assign_proof(self, g):
        """assign_proof_with_pis after the public inputs (verifier_circuit.rs:95-100) -> the proof's cells"""
        value = lambda words: [g.assign_value(hg.Input(w)) for w in words]                            # noqa: E731
        wires_cap, zs_cap, quotient_cap = [[value(h) for h in cap] for cap in self.proof_caps]
        op = {name: [value(e) for e in self.openings[name]]
              for name in ("constants", "plonk_sigmas", "wires", "plonk_zs", "plonk_zs_next", "partial_products", "quotient_polys")}
        layer_caps = [[value(h) for h in cap] for cap in self.layer_caps]
        rounds = []
        for _, initial, steps in self.queries:
            evals = [value(leaf) for leaf, _ in initial]
            proofs = [[value(s) for s in siblings] for _, siblings in initial]
            steps = [([value(ev[0:2]), value(ev[2:4])], [value(s) for s in siblings]) for ev, siblings in steps]
            rounds.append(dict(initial_trees=list(zip(evals, proofs)), steps=steps))
        final_poly = [value(e) for e in self.final_poly]
        pow_witness = g.assign_value(hg.Input(self.pow_witness))
        fri_proof = dict(commit_phase_merkle_caps=layer_caps, query_round_proofs=rounds, final_poly=final_poly)
        return dict(wires_cap=wires_cap, zs_cap=zs_cap, quotient_cap=quotient_cap, openings=op, fri_proof=fri_proof, pow_witness=pow_witness)

    def _assign_verification_key(self, g):
        """assign_verification_key (verifier_circuit.rs:113-127) -> (constants_sigmas_cap, circuit_digest) as constants"""
        cd = self.cd
        constants_sigmas_cap = [[g.assign_constant(int(w)) for w in h] for h in np.asarray(cd["constants_sigmas_cap"], dtype=np.uint64).reshape(-1, 4)]
        circuit_digest = [g.assign_constant(int(w)) for w in cd["circuit_digest"]]
        return constants_sigmas_cap, circuit_digest

    def _get_challenges(self, rec, proof, circuit_digest, public_inputs_hash):
        """get_challenges, plonk_verifier_chip.rs:55-154 -> every challenge's cells and the FRI openings"""
        op, fri_proof = proof["openings"], proof["fri_proof"]
        tr = hg.TranscriptChip(rec)
        for e in circuit_digest + public_inputs_hash:
            tr.write_scalar(e)
        tr.write_cap(proof["wires_cap"])
        plonk_betas = tr.squeeze(self.nch)
        plonk_gammas = tr.squeeze(self.nch)
        tr.write_cap(proof["zs_cap"])
        plonk_alphas = tr.squeeze(self.nch)
        tr.write_cap(proof["quotient_cap"])
        plonk_zeta = tr.squeeze(2)
        fri_openings = [op["constants"] + op["plonk_sigmas"] + op["wires"] + op["plonk_zs"] + op["partial_products"] + op["quotient_polys"],
                        op["plonk_zs_next"]]                         # to_fri_openings, types/assigned.rs:26-44
        for values in fri_openings:
            for e in values:
                tr.write_extension(e)
        fri_alpha = tr.squeeze(2)
        fri_betas = []
        for cap in fri_proof["commit_phase_merkle_caps"]:
            tr.write_cap(cap)
            fri_betas.append(tr.squeeze(2))
        for e in fri_proof["final_poly"]:
            tr.write_extension(e)
        tr.write_scalar(proof["pow_witness"])
        fri_pow_response = tr.squeeze(1)[0]
        fri_query_indices = tr.squeeze(self.n_queries)
        return dict(plonk_betas=plonk_betas, plonk_gammas=plonk_gammas, plonk_alphas=plonk_alphas, plonk_zeta=plonk_zeta, fri_openings=fri_openings,
                    fri_alpha=fri_alpha, fri_betas=fri_betas, fri_pow_response=fri_pow_response, fri_query_indices=fri_query_indices)

    def _verify_fri(self, rec, g, ge, proof, constants_sigmas_cap, ch):
        """verify_proof_with_challenges from zeta_next on, plonk_verifier_chip.rs:212-240; sets round_rows"""
        cd = self.cd
        merkle_caps = [constants_sigmas_cap, proof["wires_cap"], proof["zs_cap"], proof["quotient_cap"]]
        zeta_next = ge.scalar_mul(ch["plonk_zeta"], hg.primitive_root_of_unity(cd["degree_bits"]))
        info = hg.FriInstanceInfo(ch["plonk_zeta"], zeta_next, self.widths, self.nch)
        offset = g.assign_constant(hg.GENERATOR)
        fri = hg.FriVerifierChip(rec, offset, self.lde_bits, self.cap_height, self.arity_bits, bool(cd["hiding"]), cd["pow_bits"])
        fri.verify_fri_proof(merkle_caps, dict(fri_alpha=ch["fri_alpha"], fri_betas=ch["fri_betas"], fri_pow_response=ch["fri_pow_response"],
                                               fri_query_indices=ch["fri_query_indices"]), ch["fri_openings"], proof["fri_proof"], info)
        self.round_rows = fri.round_rows

    def record(self, inputs, min_k=17):
        """-> the Recorder of the circuit at the smallest k that holds it; round_rows[i] is the half-open row range of query round i and
        challenge_cells holds the cells of fri_alpha, fri_betas, pow_response and indices"""
        rec = hg.Recorder(28, inputs)
        g = hg.GoldilocksChip(rec)
        ge = hg.GoldilocksExtensionChip(rec)
        g.load_table()
        # assign_proof_with_pis (the public inputs' place is taken by their hash), then assign_verification_key
        public_inputs_hash = [g.assign_value(hg.Input(w)) for w in self.pi_hash]
        proof = self._assign_proof(g)
        constants_sigmas_cap, circuit_digest = self._assign_verification_key(g)
        ch = self._get_challenges(rec, proof, circuit_digest, public_inputs_hash)      # the plonk betas, gammas and alphas are not used here
        self.challenge_cells = dict(fri_alpha=ch["fri_alpha"], fri_betas=ch["fri_betas"], pow_response=ch["fri_pow_response"], indices=ch["fri_query_indices"])
        self._verify_fri(rec, g, ge, proof, constants_sigmas_cap, ch)
        for row, cell in enumerate(public_inputs_hash):
            g.arithmetic_chip.expose_public(cell, row)
        rec.shrink_to_fit(min_k)
        return rec


class Plonky2VerifierCircuit(FriVerifierCircuit):
    """The whole of Verifier::synthesize (verifier_circuit.rs:148-200).  The input vector is the flat proof of gl355_prove followed by the
    public inputs themselves, which are the instances; their hash, every challenge, the vanishing polynomial at zeta and the quotient identity
    are computed and asserted in circuit.  The number of public inputs is a property of the plonky2 circuit that common_data does not carry:
    it is given here, or taken from the first input vector."""

    def __init__(self, common_data, num_public_inputs=None):
        super().__init__(common_data)
        del self.pi_hash
        self.num_public_inputs = num_public_inputs
        self.vanishing_cells, self.identity_rows = [], []
        self._set_inputs()

    def _set_inputs(self):
        n = self.num_public_inputs or 0
        self.public_inputs = list(range(self.proof_words, self.proof_words + n))
        self.n_inputs = self.proof_words + n

    def inputs(self, flat, public_inputs):
        flat = np.ascontiguousarray(flat, dtype=np.uint64).reshape(-1)
        public_inputs = np.asarray(public_inputs, dtype=np.uint64).reshape(-1)
        assert flat.size == self.proof_words == int(flat[0]) and int(flat[4]) == public_inputs.size, "not a proof of this circuit"
        if self.num_public_inputs is None:
            self.num_public_inputs = int(public_inputs.size)
            self._set_inputs()
        out = np.concatenate([flat, public_inputs])
        assert out.size == self.n_inputs
        return out

    def record(self, inputs, min_k=17):
        """-> the Recorder of the circuit at the smallest k that holds it.  challenge_cells holds the cells of every challenge (betas, gammas,
        alphas, zeta, fri_alpha, fri_betas, pow_response, indices), vanishing_cells the vanishing polynomial at zeta (one extension element
        per challenge), identity_rows the rows whose cells the quotient identity's assertions compare, round_rows the FRI query rounds"""
        if self.num_public_inputs is None:
            self.num_public_inputs = len(inputs) - self.proof_words
            self._set_inputs()
        assert len(inputs) == self.n_inputs
        rec = hg.Recorder(28, inputs)
        g = hg.GoldilocksChip(rec)
        ge = hg.GoldilocksExtensionChip(rec)
        g.load_table()
        public_inputs = [g.assign_value(hg.Input(w)) for w in self.public_inputs]      # assign_proof_with_pis, verifier_circuit.rs:81-111
        proof = self._assign_proof(g)
        constants_sigmas_cap, circuit_digest = self._assign_verification_key(g)
        plonk = hp.PlonkVerifierChip(rec, self.cd)
        public_inputs_hash = plonk.get_public_inputs_hash(public_inputs)
        ch = self._get_challenges(rec, proof, circuit_digest, public_inputs_hash)
        self.challenge_cells = dict(betas=ch["plonk_betas"], gammas=ch["plonk_gammas"], alphas=ch["plonk_alphas"], zeta=ch["plonk_zeta"],
                                    fri_alpha=ch["fri_alpha"], fri_betas=ch["fri_betas"], pow_response=ch["fri_pow_response"], indices=ch["fri_query_indices"])
        # verify_proof_with_challenges, plonk_verifier_chip.rs:156-242
        self.vanishing_cells = plonk.verify_vanishing_identity(proof["openings"], public_inputs_hash, ch["plonk_zeta"], ch["plonk_betas"],
                                                               ch["plonk_gammas"], ch["plonk_alphas"])
        self.identity_rows = plonk.identity_rows
        self._verify_fri(rec, g, ge, proof, constants_sigmas_cap, ch)
        for row, cell in enumerate(public_inputs):                   # verifier_circuit.rs:190-198
            g.arithmetic_chip.expose_public(cell, row)
        rec.shrink_to_fit(min_k)
        return rec
