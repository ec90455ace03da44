"""Part 3 of the Halo2 verifier circuit: the chips that check the opened values against the plonky2 circuit, recorded over the chips of
halo2_goldilocks.py in the same manner (every method cites its Rust lines and keeps the Rust's order of operations and its wasteful forms:
the row layout is the reference's).  Nothing here assigns a derived witness, so the tape needs no op beyond part 2's.

  GoldilocksExtensionAlgebraChip    chip/goldilocks_extension_algebra_chip.rs:34-171
  the 12 gate constrainers          chip/plonk/gates/{arithmetic,arithmetic_extension,base_sum,constant,multiplication_extension,noop,poseidon,
                                    poseidon_mds,public_input,random_access,reducing,reducing_extension}.rs
  eval_filtered_constraint          chip/plonk/gates/mod.rs:87-132
  PublicInputsHasherChip            chip/public_inputs_hasher_chip.rs:35-365 over Spec::new(8, 22) (poseidon_spec.optimized_spec)
  PlonkVerifierChip                 chip/plonk/vanishing_poly.rs:18-218, chip/plonk/plonk_verifier_chip.rs:42-53, :156-210

A gate is identified as common()["gates"] identifies it: (type, parameter).  An extension element is a list of two cells, an element of the
extension algebra a list of two extension elements."""
from . import halo2_goldilocks as hg
from . import poseidon_spec as ps
from ._lib import (GATE_ARITHMETIC, GATE_ARITHMETIC_EXT, GATE_BASE_SUM, GATE_CONSTANT, GATE_COSET_INTERPOLATION, GATE_MUL_EXT, GATE_NOOP, GATE_POSEIDON, GATE_POSEIDON_MDS,
                   GATE_PUBLIC_INPUT, GATE_RANDOM_ACCESS, GATE_REDUCING, GATE_REDUCING_EXT)

P = hg.P
T, R_F_HALF, R_P = ps.T, ps.HALF_F, ps.R_P
UNUSED_SELECTOR = 0xFFFFFFFF                                         # gates/mod.rs:30


class GoldilocksExtensionAlgebraChip:
    def __init__(self, ctx):
        self.ctx = ctx
        self.goldilocks_extension_chip = hg.GoldilocksExtensionChip(ctx)

    def zero_ext_algebra(self):                                      # goldilocks_extension_algebra_chip.rs:34-44
        zero_extension = self.goldilocks_extension_chip.zero_extension()
        return [zero_extension, zero_extension]

    def convert_to_ext_algebra(self, et):                            # :46-56
        zero_extension = self.goldilocks_extension_chip.zero_extension()
        return [et, zero_extension]

    def inner_product_extension(self, constant, starting_acc, pairs):      # :59-82
        acc = starting_acc
        for a, b in pairs:
            acc = self.goldilocks_extension_chip.arithmetic_extension(constant, 1, a, b, acc)
        return acc

    def scalar_mul_add_ext_algebra(self, a, b, c):                   # :85-98; a in the extension field
        return [self.goldilocks_extension_chip.mul_add_extension(a, b[i], c[i]) for i in range(2)]

    def scalar_mul_ext_algebra(self, a, b):                          # :101-109
        zero = self.zero_ext_algebra()
        return self.scalar_mul_add_ext_algebra(a, b, zero)

    def mul_add_ext_algebra(self, a, b, c):                          # :112-146
        inner, inner_w = [[], []], [[], []]
        for i in range(2):
            for j in range(2 - i):
                inner[(i + j) % 2].append((a[i], b[j]))
            for j in range(2 - i, 2):
                inner_w[(i + j) % 2].append((a[i], b[j]))
        res = []
        for pairs_w, pairs, ci in zip(inner_w, inner, c):
            acc = self.inner_product_extension(hg.W, ci, pairs_w)
            res.append(self.inner_product_extension(1, acc, pairs))
        return res

    def mul_ext_algebra(self, a, b):                                 # :149-157
        zero = self.zero_ext_algebra()
        return self.mul_add_ext_algebra(a, b, zero)

    def sub_ext_algebra(self, a, b):                                 # :159-171
        return [self.goldilocks_extension_chip.sub_extension(a[i], b[i]) for i in range(2)]


# ---- the gate constrainers ------------------------------------------------------------------------------------------------------------------
class GateConstrainer:
    """CustomGateConstrainer (gates/mod.rs:48-133) for the gate (type, parameter)"""

    def __init__(self, ctx, gate):
        self.ctx, (self.type, self.param) = ctx, gate
        if self.type == GATE_COSET_INTERPOLATION:
            raise ValueError("CosetInterpolationGate (gate type %d) has no constrainer: the reference's verifier circuit knows the 12 gates of "
                             "gates/mod.rs:141-196; build the inner circuit without CircuitConfig.use_interpolation_gate" % self.type)
        self.goldilocks_extension_chip = hg.GoldilocksExtensionChip(ctx)
        self.goldilocks_extension_algebra_chip = GoldilocksExtensionAlgebraChip(ctx)
        self.eval_unfiltered_constraint = {
            GATE_NOOP: self._noop, GATE_CONSTANT: self._constant, GATE_PUBLIC_INPUT: self._public_input, GATE_BASE_SUM: self._base_sum,
            GATE_POSEIDON: self._poseidon, GATE_ARITHMETIC: self._arithmetic, GATE_ARITHMETIC_EXT: self._arithmetic_extension,
            GATE_MUL_EXT: self._multiplication_extension, GATE_POSEIDON_MDS: self._poseidon_mds, GATE_RANDOM_ACCESS: self._random_access,
            GATE_REDUCING: self._reducing, GATE_REDUCING_EXT: self._reducing_extension}[self.type]

    @staticmethod
    def get_local_ext_algebra(local_wires, start):                   # mod.rs:51-59
        return [local_wires[start], local_wires[start + 1]]

    def eval_filtered_constraint(self, local_constants, local_wires, public_inputs_hash, row, selector_index, group_range, num_selectors,
                                 combined_gate_constraints):         # mod.rs:87-132; group_range: (first, past the last)
        ge = self.goldilocks_extension_chip
        f_zeta = local_constants[selector_index]
        terms = []
        for i in [i for i in range(*group_range) if i != row] + ([UNUSED_SELECTOR] if num_selectors > 1 else []):
            k = ge.constant_extension((i, 0))
            terms.append(ge.sub_extension(k, f_zeta))
        filter_ = ge.mul_many_extension(terms)
        gate_constraints = self.eval_unfiltered_constraint(local_constants[num_selectors:], local_wires, public_inputs_hash)
        for i, c in enumerate(gate_constraints[:len(combined_gate_constraints)]):
            combined_gate_constraints[i] = ge.mul_add_extension(filter_, c, combined_gate_constraints[i])

    def _noop(self, local_constants, local_wires, public_inputs_hash):      # noop.rs:14-26
        return []

    def _constant(self, local_constants, local_wires, public_inputs_hash):      # constant.rs:18-40
        ge = self.goldilocks_extension_chip
        return [ge.sub_extension(local_constants[i], local_wires[i]) for i in range(self.param)]

    def _public_input(self, local_constants, local_wires, public_inputs_hash):      # public_input.rs:16-43
        ge = self.goldilocks_extension_chip
        out = []
        for wire, hash_part in zip(range(4), public_inputs_hash):
            hash_part_ext = ge.convert_to_extension(hash_part)
            out.append(ge.sub_extension(local_wires[wire], hash_part_ext))
        return out

    def _base_sum(self, local_constants, local_wires, public_inputs_hash):      # base_sum.rs:18-66: WIRE_SUM 0, the limbs from wire 1, base 2
        ge = self.goldilocks_extension_chip
        base = ge.two_extension()
        sum_ = local_wires[0]
        limbs = local_wires[1:1 + self.param]
        computed_sum = ge.reduce_extension(base, limbs)
        constraints = [ge.sub_extension(computed_sum, sum_)]
        for limb in limbs:
            acc = ge.one_extension()
            for i in range(2):                                       # acc' = acc limb + (-i) acc
                acc = ge.arithmetic_extension(1, (P - i) % P, acc, limb, acc)
            constraints.append(acc)
        return constraints

    def _arithmetic(self, local_constants, local_wires, public_inputs_hash):      # arithmetic.rs:19-70: wires 4 i .. 4 i + 3
        ge = self.goldilocks_extension_chip
        const_0, const_1 = local_constants[0], local_constants[1]
        constraints = []
        for i in range(self.param):
            multiplicand_0, multiplicand_1, addend, output = local_wires[4 * i:4 * i + 4]
            term1 = ge.mul_extension(multiplicand_0, multiplicand_1)
            term1 = ge.mul_extension(term1, const_0)
            term2 = ge.mul_extension(addend, const_1)
            computed_output = ge.add_extension(term1, term2)
            constraints.append(ge.sub_extension(output, computed_output))
        return constraints

    def _arithmetic_extension(self, local_constants, local_wires, public_inputs_hash):      # arithmetic_extension.rs:21-83: wires 8 i .. 8 i + 7
        gea = self.goldilocks_extension_algebra_chip
        const_0, const_1 = local_constants[0], local_constants[1]
        constraints = []
        for i in range(self.param):
            multiplicand_0, multiplicand_1, addend, output = (self.get_local_ext_algebra(local_wires, 8 * i + 2 * j) for j in range(4))
            mul = gea.mul_ext_algebra(multiplicand_0, multiplicand_1)
            scaled_mul = gea.scalar_mul_ext_algebra(const_0, mul)
            computed_output = gea.scalar_mul_add_ext_algebra(const_1, addend, scaled_mul)
            constraints += gea.sub_ext_algebra(output, computed_output)
        return constraints

    def _multiplication_extension(self, local_constants, local_wires, public_inputs_hash):      # multiplication_extension.rs:21-72: wires 6 i .. 6 i + 5
        gea = self.goldilocks_extension_algebra_chip
        const_0 = local_constants[0]
        constraints = []
        for i in range(self.param):
            multiplicand_0, multiplicand_1, output = (self.get_local_ext_algebra(local_wires, 6 * i + 2 * j) for j in range(3))
            mul = gea.mul_ext_algebra(multiplicand_0, multiplicand_1)
            computed_output = gea.scalar_mul_ext_algebra(const_0, mul)
            constraints += gea.sub_ext_algebra(output, computed_output)
        return constraints

    def _poseidon_mds(self, local_constants, local_wires, public_inputs_hash):      # poseidon_mds.rs:25-126
        ge, gea = self.goldilocks_extension_chip, self.goldilocks_extension_algebra_chip
        inputs = [self.get_local_ext_algebra(local_wires, 2 * i) for i in range(T)]
        computed_outputs = []
        for row in range(T):                                         # mds_layer, mds_row_shf, :36-96
            res = gea.zero_ext_algebra()
            for i in range(T):
                c = ge.constant_extension((ps.MDS_MATRIX_CIRC[i], 0))
                res = gea.scalar_mul_add_ext_algebra(c, inputs[(i + row) % T], res)
            c = ge.constant_extension((ps.MDS_MATRIX_DIAG[row], 0))
            computed_outputs.append(gea.scalar_mul_add_ext_algebra(c, inputs[row], res))
        constraints = []
        for i, computed_out in enumerate(computed_outputs):
            out = self.get_local_ext_algebra(local_wires, 2 * (T + i))
            constraints += gea.sub_ext_algebra(out, computed_out)
        return constraints

    def _random_access(self, local_constants, local_wires, public_inputs_hash):      # random_access.rs:25-143
        ge = self.goldilocks_extension_chip
        bits_n, num_copies, num_extra_constants = self.param & 0xFF, (self.param >> 8) & 0xFF, (self.param >> 16) & 0xFF
        vec_size = 1 << bits_n
        start_extra_constants = (2 + vec_size) * num_copies          # :50-52
        num_routed_wires = start_extra_constants + num_extra_constants      # :60-62
        two = ge.two_extension()
        constraints = []
        for copy in range(num_copies):
            access_index = local_wires[(2 + vec_size) * copy]
            list_items = [local_wires[(2 + vec_size) * copy + 2 + i] for i in range(vec_size)]
            claimed_element = local_wires[(2 + vec_size) * copy + 1]
            bits = [local_wires[num_routed_wires + copy * bits_n + i] for i in range(bits_n)]
            for b in bits:
                constraints.append(ge.mul_sub_extension(b, b, b))
            reconstructed_index = ge.reduce_extension(two, bits)
            constraints.append(ge.sub_extension(reconstructed_index, access_index))
            for b in bits:
                list_items = [ge.select(b, list_items[2 * k + 1], list_items[2 * k]) for k in range(len(list_items) // 2)]
            assert len(list_items) == 1
            constraints.append(ge.sub_extension(list_items[0], claimed_element))
        for i in range(num_extra_constants):
            constraints.append(ge.sub_extension(local_constants[i], local_wires[start_extra_constants + i]))
        return constraints

    def _reducing_rows(self, local_wires, coeffs, start_accs):      # the loop reducing.rs:72-84 and reducing_extension.rs:77-88 share
        gea = self.goldilocks_extension_algebra_chip
        alpha = self.get_local_ext_algebra(local_wires, 2)
        old_acc = self.get_local_ext_algebra(local_wires, 4)
        n = self.param
        accs = [self.get_local_ext_algebra(local_wires, 0 if i == n - 1 else start_accs + 2 * i) for i in range(n)]      # wires_accs: the last is the output
        constraints = []
        acc = old_acc
        for i in range(n):
            coeff = coeffs(i)
            tmp = gea.mul_add_ext_algebra(acc, alpha, coeff)
            tmp = gea.sub_ext_algebra(tmp, accs[i])
            constraints += tmp
            acc = accs[i]
        return constraints

    def _reducing(self, local_constants, local_wires, public_inputs_hash):      # reducing.rs:19-91: output 0-1, alpha 2-3, old_acc 4-5, coeffs from 6
        gea = self.goldilocks_extension_algebra_chip
        return self._reducing_rows(local_wires, lambda i: gea.convert_to_ext_algebra(local_wires[6 + i]), 6 + self.param)

    def _reducing_extension(self, local_constants, local_wires, public_inputs_hash):      # reducing_extension.rs:19-95: coeff i on 6 + 2 i
        return self._reducing_rows(local_wires, lambda i: self.get_local_ext_algebra(local_wires, 6 + 2 * i), 6 + 2 * self.param)

    # ---- PoseidonGate, poseidon.rs:327-698 ----
    def _constant_layer(self, state, constants):                     # constant_layer :382-404, partial_first_constant_layer :406-427
        ge = self.goldilocks_extension_chip
        for i in range(T):
            c = ge.constant_extension((constants[i], 0))
            state[i] = ge.add_extension(state[i], c)

    def _sbox(self, element):                                        # :429-437
        return self.goldilocks_extension_chip.exp(element, 7)

    def _mds_layer(self, state):                                     # mds_row_shf, mds_layer :450-502
        ge = self.goldilocks_extension_chip
        result = []
        for row in range(T):
            res = ge.zero_extension()
            for i in range(T):
                c = ge.constant_extension((ps.MDS_MATRIX_CIRC[i], 0))
                res = ge.mul_add_extension(c, state[(i + row) % T], res)
            c = ge.constant_extension((ps.MDS_MATRIX_DIAG[row], 0))
            result.append(ge.mul_add_extension(c, state[row], res))
        return result

    def _mds_partial_layer_init(self, state, tb):                    # :504-537
        ge = self.goldilocks_extension_chip
        result = [ge.zero_extension() for _ in range(T)]
        result[0] = state[0]
        for r in range(1, T):
            for c in range(1, T):
                t = ge.constant_extension((tb["init"][r - 1][c - 1], 0))
                result[c] = ge.mul_add_extension(t, state[r], result[c])
        return result

    def _mds_partial_layer_fast(self, state, r, tb):                 # :539-589
        ge = self.goldilocks_extension_chip
        s0 = state[0]
        d = ge.scalar_mul(s0, ps.MDS_MATRIX_CIRC[0] + ps.MDS_MATRIX_DIAG[0])
        for i in range(1, T):
            t = ge.constant_extension((tb["w_hats"][r][i - 1], 0))
            d = ge.mul_add_extension(t, state[i], d)
        result = [ge.zero_extension() for _ in range(T)]
        result[0] = d
        for i in range(1, T):
            t = ge.constant_extension((tb["vs"][r][i - 1], 0))
            result[i] = ge.mul_add_extension(t, state[0], state[i])
        return result

    def _poseidon(self, local_constants, local_wires, public_inputs_hash):      # :592-697
        ge = self.goldilocks_extension_chip
        rc, tb = ps.round_constants(), ps.fast_partial_tables()
        wire_swap, start_delta = 2 * T, 2 * T + 1
        start_full_0 = start_delta + 4
        start_partial = start_full_0 + T * (R_F_HALF - 1)
        start_full_1 = start_partial + R_P
        constraints = []
        swap = local_wires[wire_swap]
        constraints.append(ge.mul_sub_extension(swap, swap, swap))
        for i in range(4):
            input_lhs, input_rhs, delta_i = local_wires[i], local_wires[i + 4], local_wires[start_delta + i]
            diff = ge.sub_extension(input_rhs, input_lhs)
            constraints.append(ge.mul_sub_extension(swap, diff, delta_i))
        state = [ge.zero_extension() for _ in range(T)]
        for i in range(4):
            delta_i, input_lhs, input_rhs = local_wires[start_delta + i], local_wires[i], local_wires[i + 4]
            state[i] = ge.add_extension(input_lhs, delta_i)
            state[i + 4] = ge.sub_extension(input_rhs, delta_i)
        for i in range(8, T):
            state[i] = local_wires[i]
        round_ctr = 0
        for r in range(R_F_HALF):                                    # the first full rounds
            self._constant_layer(state, rc[round_ctr])
            if r != 0:
                for i in range(T):
                    sbox_in = local_wires[start_full_0 + T * (r - 1) + i]
                    constraints.append(ge.sub_extension(state[i], sbox_in))
                    state[i] = sbox_in
            state = [self._sbox(x) for x in state]
            state = self._mds_layer(state)
            round_ctr += 1
        self._constant_layer(state, tb["first"])
        state = self._mds_partial_layer_init(state, tb)
        for r in range(R_P - 1):
            sbox_in = local_wires[start_partial + r]
            constraints.append(ge.sub_extension(state[0], sbox_in))
            state[0] = self._sbox(sbox_in)
            c = ge.constant_extension((tb["post"][r], 0))
            state[0] = ge.add_extension(state[0], c)
            state = self._mds_partial_layer_fast(state, r, tb)
        sbox_in = local_wires[start_partial + R_P - 1]
        constraints.append(ge.sub_extension(state[0], sbox_in))
        state[0] = self._sbox(sbox_in)
        state = self._mds_partial_layer_fast(state, R_P - 1, tb)
        round_ctr += R_P
        for r in range(R_F_HALF):                                    # the second full rounds
            self._constant_layer(state, rc[round_ctr])
            for i in range(T):
                sbox_in = local_wires[start_full_1 + T * r + i]
                constraints.append(ge.sub_extension(state[i], sbox_in))
                state[i] = sbox_in
            state = [self._sbox(x) for x in state]
            state = self._mds_layer(state)
            round_ctr += 1
        for i in range(T):
            constraints.append(ge.sub_extension(state[i], local_wires[T + i]))
        return constraints


# ---- PublicInputsHasherChip -------------------------------------------------------------------------------------------------------------------
RATE = 8


class PublicInputsHasherChip:
    """the public inputs hashed by a Goldilocks Poseidon made of GoldilocksChip rows (the transcript's HasherChip is Bn254PoseidonHash).  The
    reference's incremental interface (update / squeeze with their absorbing and output buffers, :62-100 and :300-313) is not restated: the
    circuit calls hash alone, which in the reference does not go through it either"""

    def __init__(self, ctx):                                         # public_inputs_hasher_chip.rs:37-58
        self.ctx = ctx
        self.spec = ps.optimized_spec()
        self.goldilocks_chip = hg.GoldilocksChip(ctx)
        self.state = [self.goldilocks_chip.assign_constant(0) for _ in range(T)]

    def sbox_full(self, constants):                                  # :144-157: x^7 + constant on every word
        g = self.goldilocks_chip
        for i, constant in enumerate(constants):
            word = self.state[i]
            word2 = g.mul(word, word)
            word4 = g.mul(word2, word2)
            word6 = g.mul(word2, word4)
            self.state[i] = g.mul_add_constant(word6, word, constant)

    def sbox_part(self, constant):                                   # :161-174
        g = self.goldilocks_chip
        word = self.state[0]
        word2 = g.mul(word, word)
        word4 = g.mul(word2, word2)
        word6 = g.mul(word2, word4)
        self.state[0] = g.mul_add_constant(word6, word, constant)

    def absorb_with_pre_constants(self, pre_constants):              # :177-190
        g = self.goldilocks_chip
        self.state = [g.add_constant(word, constant) for word, constant in zip(self.state, pre_constants)]

    def apply_mds(self, mds):                                        # :193-222
        g = self.goldilocks_chip
        self.state = [g.compose(list(zip(self.state, row)), 0) for row in mds]

    def apply_sparse_mds(self, mds):                                 # :225-262; mds: (row, col_hat)
        g = self.goldilocks_chip
        row, col_hat = mds
        new_state = [g.compose(list(zip(self.state, row)), 0)]
        for e, word in zip(col_hat, self.state[1:]):
            new_state.append(g.compose([(self.state[0], e), (word, 1)], 0))
        self.state = new_state

    def permutation(self):                                           # :265-298
        sp = self.spec
        r_f = R_F_HALF
        constants = sp["start"]
        self.absorb_with_pre_constants(constants[0])
        for cs in constants[1:r_f]:
            self.sbox_full(cs)
            self.apply_mds(sp["mds"])
        self.sbox_full(constants[-1])
        self.apply_mds(sp["pre_sparse_mds"])
        for constant, sparse_mds in zip(sp["partial"], sp["sparse"]):
            self.sbox_part(constant)
            self.apply_sparse_mds(sparse_mds)
        for cs in sp["end"]:
            self.sbox_full(cs)
            self.apply_mds(sp["mds"])
        self.sbox_full([0] * T)
        self.apply_mds(sp["mds"])

    def _outputs(self, num_outputs):
        outputs = []
        while True:
            for item in self.state[:RATE]:
                outputs.append(item)
                if len(outputs) == num_outputs:
                    return outputs
            self.permutation()

    def hash(self, inputs, num_outputs):                             # :315-341
        for off in range(0, len(inputs), RATE):
            chunk = inputs[off:off + RATE]
            self.state[:len(chunk)] = chunk
            self.permutation()
        return self._outputs(num_outputs)

    def permute(self, inputs, num_output):                           # :343-364
        self.state[:len(inputs)] = inputs
        self.permutation()
        return self._outputs(num_output)


# ---- PlonkVerifierChip ------------------------------------------------------------------------------------------------------------------------
class PlonkVerifierChip:
    """common_data: what CircuitData.common() gives (gates, groups, selector_indices, num_selectors, k_is, ...)"""

    def __init__(self, ctx, common_data):
        self.ctx, self.cd = ctx, common_data
        self.goldilocks_extension_chip = hg.GoldilocksExtensionChip(ctx)
        self.identity_rows = []

    def get_public_inputs_hash(self, public_inputs):                 # plonk_verifier_chip.rs:42-53
        return PublicInputsHasherChip(self.ctx).hash(list(public_inputs), 4)

    def eval_gate_constraints(self, local_constants, local_wires, public_inputs_hash):      # vanishing_poly.rs:126-153
        cd = self.cd
        zero_extension = self.goldilocks_extension_chip.zero_extension()
        all_gate_constraints = [zero_extension] * cd["num_gate_constraints"]
        for i, gate in enumerate(cd["gates"]):
            selector_index = cd["selector_indices"][i]
            GateConstrainer(self.ctx, (int(gate[0]), int(gate[1]))).eval_filtered_constraint(
                local_constants, local_wires, public_inputs_hash, i, selector_index, tuple(cd["groups"][selector_index]), cd["num_selectors"],
                all_gate_constraints)
        return all_gate_constraints

    def eval_l_0_x(self, n, x, x_pow_n):                             # :155-178: (x^n - 1) / (n (x - 1))
        ge = self.goldilocks_extension_chip
        one_extension = ge.one_extension()
        neg_one_extension = ge.constant_extension((P - 1, 0))
        zero_poly = ge.sub_extension(x_pow_n, one_extension)
        denominator = ge.arithmetic_extension(n % P, n % P, x, one_extension, neg_one_extension)
        return ge.div_extension(zero_poly, denominator)

    def check_partial_products(self, numerators, denominators, partials, z_x, z_gx, max_degree):      # :183-218
        ge = self.goldilocks_extension_chip
        product_accs = [z_x] + list(partials) + [z_gx]
        chunks = range(0, len(numerators), max_degree)
        assert len(chunks) == len(product_accs) - 1                 # zip_eq
        out = []
        for k, off in enumerate(chunks):
            prev_acc, next_acc = product_accs[k], product_accs[k + 1]
            nume_product = ge.mul_many_extension(numerators[off:off + max_degree])
            denom_product = ge.mul_many_extension(denominators[off:off + max_degree])
            next_acc_deno = ge.mul_extension(next_acc, denom_product)
            out.append(ge.mul_sub_extension(prev_acc, nume_product, next_acc_deno))
        return out

    def eval_vanishing_poly(self, x, x_pow_deg, local_constants, local_wires, public_inputs_hash, local_zs, next_zs, partial_products, s_sigmas,
                            betas, gammas, alphas):                  # :18-124
        cd, ge = self.cd, self.goldilocks_extension_chip
        max_degree, num_prods = cd["quotient_degree_factor"], cd["num_partial_products"]
        constraint_terms = self.eval_gate_constraints(local_constants, local_wires, public_inputs_hash)
        vanishing_z_1_terms, vanishing_partial_products_terms = [], []
        l_0_x = self.eval_l_0_x(1 << cd["degree_bits"], x, x_pow_deg)
        s_ids = [ge.scalar_mul(x, int(cd["k_is"][j])) for j in range(cd["num_routed_wires"])]
        for i in range(cd["num_challenges"]):
            z_x, z_gx = local_zs[i], next_zs[i]
            vanishing_z_1_terms.append(ge.mul_sub_extension(l_0_x, z_x, l_0_x))
            numerator_values, denominator_values = [], []
            for j in range(cd["num_routed_wires"]):
                wire_value = local_wires[j]
                beta = ge.convert_to_extension(betas[i])
                gamma = ge.convert_to_extension(gammas[i])
                wire_value_plus_gamma = ge.add_extension(wire_value, gamma)
                numerator_values.append(ge.mul_add_extension(beta, s_ids[j], wire_value_plus_gamma))
                denominator_values.append(ge.mul_add_extension(beta, s_sigmas[j], wire_value_plus_gamma))
            current_partial_products = partial_products[i * num_prods:(i + 1) * num_prods]
            vanishing_partial_products_terms += self.check_partial_products(numerator_values, denominator_values, current_partial_products, z_x,
                                                                            z_gx, max_degree)
        vanishing_terms = vanishing_z_1_terms + vanishing_partial_products_terms + constraint_terms
        out = []
        for alpha in alphas:
            alpha = ge.convert_to_extension(alpha)
            out.append(ge.reduce_extension(alpha, vanishing_terms))
        return out

    def verify_vanishing_identity(self, op, public_inputs_hash, plonk_zeta, betas, gammas, alphas):
        """verify_proof_with_challenges up to the quotient identity (plonk_verifier_chip.rs:165-210) -> the cells of the vanishing polynomial at
        zeta, one extension element per challenge; identity_rows gets the rows the identity's assertions compare (their ASSERT_EQ entries
        write none of their own)"""
        cd, ge = self.cd, self.goldilocks_extension_chip
        one = ge.one_extension()
        zeta_pow_deg = ge.exp_power_of_2_extension(plonk_zeta, cd["degree_bits"])
        vanishing_poly_zeta = self.eval_vanishing_poly(plonk_zeta, zeta_pow_deg, op["constants"], op["wires"], public_inputs_hash, op["plonk_zs"],
                                                       op["plonk_zs_next"], op["partial_products"], op["plonk_sigmas"], betas, gammas, alphas)
        z_h_zeta = ge.sub_extension(zeta_pow_deg, one)
        qdf = cd["quotient_degree_factor"]
        self.identity_rows = []
        for i in range(0, len(op["quotient_polys"]) // qdf):
            chunk = op["quotient_polys"][i * qdf:(i + 1) * qdf]
            recombined_quotient = ge.reduce_extension(zeta_pow_deg, chunk)
            computed_vanishing_poly = ge.mul_extension(z_h_zeta, recombined_quotient)
            ge.assert_equal_extension(vanishing_poly_zeta[i], computed_vanishing_poly)
            self.identity_rows += [c.row for c in vanishing_poly_zeta[i] + computed_vanishing_poly]
        return vanishing_poly_zeta
