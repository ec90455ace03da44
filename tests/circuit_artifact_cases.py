"""Malformed circuit artifacts (include/gl355.h "circuit artifacts", stark-verifier_amd/plonk.py export_blob) for the host check of
csrc/circuit_artifact.h (tests/test_circuit_artifact_host.py) and gl355_circuit_load (tests/test_gpu_circuit_artifact.py): one mutation list,
and this file's own statement of the parser's bounds in Python integers.  An artifact here is a numpy array of u64 words; a case is a
list of edits of a well-formed base -- ("s", i, v) sets word i to v, ("t", n) truncates to n words, ("a", v) appends a word -- which
tests/circuit_artifact_check.cpp reads as `s i v`, `t n` and `a v`."""
import importlib

import numpy as np

import coset_interpolation_model as cim

A = importlib.import_module("stark-verifier_amd.plonk").ARTIFACT_WORDS
HDR = A["ART_HDR_WORDS"]
MAGIC = int.from_bytes(b"GL355CIR", "little")
INVALID_ARG, UNSUPPORTED = -1, -5
U32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
MAX_GATES, MAX_ARITY_BITS = 16, 4
GATE_NAMES = ["NoopGate", "ConstantGate", "PublicInputGate", "BaseSumGate", "PoseidonGate", "ArithmeticGate", "ArithmeticExtensionGate", "MulExtensionGate",
              "PoseidonMdsGate", "RandomAccessGate", "ReducingGate", "ReducingExtensionGate", "CosetInterpolationGate"]
# the words that are only asked to fit 32 bits, by the message that says so
SHAPE_WORDS = range(A["ART_DEGREE_BITS"], A["ART_NUM_GATES"] + 1)
PARAM_WORDS = (A["ART_POW_BITS"], A["ART_NUM_QUERIES"], A["ART_ZERO_KNOWLEDGE"])
# gate_table_check's four messages, by what each contains
GATE_MESSAGES = ("has the unknown type", "has a bad selector group", "has the parameter", "does not fit")


def line(edits):
    return " ".join("s %d %x" % e[1:] if e[0] == "s" else "t %d" % e[1] if e[0] == "t" else "a %x" % e[1] for e in edits)


def apply(base, edits):
    n = min([e[1] for e in edits if e[0] == "t"] + [base.size])
    w = np.concatenate([base[:n], np.array([e[1] for e in edits if e[0] == "a"], dtype=np.uint64)])
    for e in edits:
        if e[0] == "s":
            w[e[1]] = np.uint64(e[2])
    return w


def gate_shape(t, p):
    """csrc/gate_shape.h in integers that cannot wrap: (wires, constants, constraints, routed) or None"""
    from test_gate_shape_host import table
    return table(t, p)


def _gate_refusal(c, gates):
    for g, (t, p, sel, start, end) in enumerate(gates):
        if t > 12:
            return "gate %d has the unknown type %d" % (g, t)
        if sel >= c["num_selectors"] or end > len(gates) or start > end:
            return "gate %d (%s) has a bad selector group" % (g, GATE_NAMES[t])
        s = gate_shape(t, p)
        if s is None:
            return "gate %d: no %s has the parameter 0x%x" % (g, GATE_NAMES[t], p)
        if s[0] > c["num_wires"] or s[1] > c["num_constants"] or s[3] > c["num_routed_wires"]:
            return "gate %d (%s, parameter 0x%x) does not fit: it reads %d wires (%d routed) and %d constants" % (g, GATE_NAMES[t], p, s[0], s[3], s[1])
    return None


def tape_fits(tape, n_inputs, n_words, num_wires):
    """csrc/witness_tape.h tape_entry_fits for every entry of `tape` ([n_ops][5], u64), with no sum of operands"""
    if num_wires < 135:
        return False
    op, a, b, c, d = (tape[:, k] for k in range(5))
    nw, wires = np.uint64(n_words), np.uint64(num_wires)

    def ok(i, span):
        return (i < nw) & (nw - np.minimum(i, nw) >= np.uint64(span))

    def row(i):
        return ok(i, num_wires) & (i % wires == 0)
    good = np.zeros(op.shape, dtype=bool)
    for code, fits in ((0, lambda: ok(a, 1)), (1, lambda: ok(a, 1) & (b < np.uint64(n_inputs))), (2, lambda: ok(a, 1) & ok(b, 1)), (3, lambda: ok(a, 1) & ok(b, 1)),
                       (4, lambda: ok(a, 4)), (5, lambda: ok(a, 8)), (6, lambda: row(a)), (7, lambda: row(a)),
                       (8, lambda: row(a) & (b <= 63) & (b + 1 <= wires)), (9, lambda: row(a) & (b < 4)),
                       (11, lambda: ok(a, 1) & ok(b, 1)), (12, lambda: ok(a, 1) & ok(b, 1)), (13, lambda: ok(a, 1) & ok(b, 1) & ok(c, 1) & ok(d, 1))):
        good |= (op == code) & fits()
    for i in np.nonzero((op == 10) | (op == 14))[0]:
        bi, ci = int(b[i]), int(c[i])
        if int(op[i]) == 10:             # REDUCING: b coefficients, extension coefficients if c
            fit = 1 <= bi <= num_wires and 6 + (2 * bi if ci else bi) + 2 * (bi - 1) <= num_wires
        else:                            # COSET_INTERP: b subgroup bits, c the degree
            fit = 2 <= bi <= 4 and 2 <= ci <= 2 ** bi and cim.layout(bi, ci)["num_wires"] <= num_wires
        good[i] = fit and bool(row(a[i:i + 1])[0])
    return bool(good.all())


def sections(w):
    """of an artifact whose header passed the size checks: {name: (offset, words)} in the artifact's order, and the length they add up to"""
    n = 1 << int(w[A["ART_DEGREE_BITS"]])
    n_sc, routed = int(w[A["ART_NUM_SELECTORS"]]) + int(w[A["ART_NUM_CONSTANTS"]]), int(w[A["ART_NUM_ROUTED_WIRES"]])
    version = int(w[A["ART_VERSION"]])
    lens = [("arity", int(w[A["ART_N_FRI_LAYERS"]]) if version >= 4 else 0), ("constants", n_sc * n), ("sigmas", routed * n), ("k_is", routed),
            ("row_idx", int(w[A["ART_N_ROWS"]])), ("pi_pos", int(w[A["ART_N_PI"]])), ("tape", 5 * int(w[A["ART_N_OPS"]])), ("seg_lens", int(w[A["ART_N_SEGS"]])),
            ("cap", 4 << int(w[A["ART_CAP_HEIGHT"]]) if version in (3, 5) else 0)]
    out, at = {}, HDR
    for name, length in lens:
        out[name] = (at, length)
        at += length
    return out, at


def refusal(w):
    """what artifact_parse says of the artifact `w`: None (accepted) or (code, message), from the format's definition alone"""
    def no(text, code=INVALID_ARG):
        return code, "circuit_load: " + text
    if w.size < HDR:
        return no("null or truncated artifact")
    h = [int(x) for x in w[:HDR]]
    if h[A["ART_MAGIC"]] != MAGIC or not 2 <= h[A["ART_VERSION"]] <= 5:
        return no("not a version-2..5 gl355 circuit artifact")
    c = {name[4:].lower(): h[A[name]] for name in A if A["ART_DEGREE_BITS"] <= A[name] <= A["ART_NUM_GATES"]}
    if any(h[i] > U32 for i in SHAPE_WORDS) or c["num_gates"] > MAX_GATES or not 1 <= c["degree_bits"] <= 24 or not 1 <= c["num_wires"] <= 1024 or \
            c["num_routed_wires"] > c["num_wires"] or c["num_selectors"] + c["num_constants"] > 64:
        return no("implausible circuit shape")
    gates = [h[A["ART_GATES"] + 5 * g:A["ART_GATES"] + 5 * g + 5] for g in range(c["num_gates"])]
    for t, p, sel, start, end in gates:
        if p > U32:
            return no("gate parameter out of range")
        if max(t, sel, start, end) > U32:
            return no("a gate's type, selector or group is no 32-bit value")
    why = _gate_refusal(c, gates)
    if why:
        return no(why)
    n = 1 << c["degree_bits"]
    n_rows, n_ops, n_inputs, n_pi, n_seq, n_segs = (h[A[k]] for k in ("ART_N_ROWS", "ART_N_OPS", "ART_N_INPUTS", "ART_N_PI", "ART_N_SEQ", "ART_N_SEGS"))
    if n_rows > n or n_ops > 1 << 28 or n_pi > 1 << 20:
        return no("implausible sizes")
    if n_seq > n_ops or n_segs > n_ops:
        return no("implausible tape segmentation")
    cap_height, n_layers = h[A["ART_CAP_HEIGHT"]], h[A["ART_N_FRI_LAYERS"]]
    if cap_height > 20:
        return no("implausible cap height")
    if n_layers > 32:
        return no("implausible number of FRI layers")
    sec, need = sections(w)
    if w.size != need:
        return no("artifact length does not match its header")
    if h[A["ART_HASHER"]] not in (0, 1):
        return no("unknown hasher")
    lde_bits = c["degree_bits"] + c["rate_bits"]
    if h[A["ART_VERSION"]] >= 4:
        total = 0
        for a in (int(x) for x in w[HDR:HDR + n_layers]):
            if a == 0 or a > U32:
                return no("a FRI layer's arity bits are zero or no 32-bit value")
            if a > MAX_ARITY_BITS:
                return no("a FRI layer folds by 2, 4, 8 or 16", UNSUPPORTED)
            total += a
            if total > c["degree_bits"]:
                return no("the FRI layers fold below one coefficient")
            if lde_bits - total < cap_height:
                return no("a FRI layer is narrower than the cap")

    def part(name):
        return w[sec[name][0]:sec[name][0] + sec[name][1]]
    if (part("row_idx") >= np.uint64(n)).any():
        return no("witness row index out of range")
    if (part("pi_pos") >= np.uint64(n_rows * c["num_wires"])).any():
        return no("public-input position out of range")
    if n_seq + sum(int(x) for x in part("seg_lens")) != n_ops:
        return no("tape segments do not add up")
    blind_start, n_blind, z_start, n_z_pairs = (h[A[k]] for k in ("ART_BLIND_START", "ART_N_BLIND", "ART_Z_START", "ART_N_Z_PAIRS"))
    if blind_start + n_blind > n or z_start + 2 * n_z_pairs > n:
        return no("blinding rows out of range")
    if n_ops and not tape_fits(part("tape").reshape(-1, 5), n_inputs, n_rows * c["num_wires"], c["num_wires"]):
        return no("malformed witness tape")
    if any(h[i] > U32 for i in PARAM_WORDS):
        return no("pow_bits, num_queries or zero_knowledge is no 32-bit value")
    if c["max_degree"] == 0:
        return no("max_degree is zero")
    if not 1 <= c["num_challenges"] <= 4:
        return no("1 to 4 challenges", UNSUPPORTED)
    if c["num_partial_products"] + 1 != -(-c["num_routed_wires"] // c["max_degree"]):
        return no("inconsistent partial-product count")
    if c["rate_bits"] > 4 or lde_bits > 28:
        return no("unsupported size", UNSUPPORTED)
    if cap_height > lde_bits:
        return no("cap_height too large")
    return None


def view(w):
    """the answer of tests/circuit_artifact_check.cpp to an accepted artifact, from its words"""
    h = [int(x) for x in w[:HDR]]
    version, n_layers = h[A["ART_VERSION"]], h[A["ART_N_FRI_LAYERS"]]
    gates = ["/".join("%d" % x for x in h[A["ART_GATES"] + 5 * g:A["ART_GATES"] + 5 * g + 5]) for g in range(h[A["ART_NUM_GATES"]])]
    arity = [int(x) for x in w[HDR:HDR + n_layers]] if version >= 4 else [1] * n_layers
    s32 = lambda x: x - (1 << 32) if x >> 31 else x
    sec, _ = sections(w)
    parts = [[version, int(version in (3, 5)), int(version >= 4)], h[A["ART_DEGREE_BITS"]:A["ART_NUM_GATES"] + 1], gates,
             h[A["ART_CAP_HEIGHT"]:A["ART_ZERO_KNOWLEDGE"]] + [s32(h[A["ART_ZERO_KNOWLEDGE"]]), h[A["ART_HASHER"]]], arity,
             h[A["ART_BLIND_START"]:A["ART_N_Z_PAIRS"] + 1], h[A["ART_N_ROWS"]:A["ART_N_PI"] + 1] + [h[A["ART_N_SEQ"]], h[A["ART_N_SEGS"]]],
             ["%x" % x for x in h[A["ART_DIGEST"]:A["ART_DIGEST"] + 4]], ["%d:%d" % sec[k] for k in sec]]
    return render(parts)


def render(parts):
    """the answer line of an accepted artifact: its parts, each a list, separated by ` |`"""
    return "ok" + " |".join("".join(" %s" % x for x in p) for p in parts)


def mutations(w):
    """[(what, edits)] around the well-formed artifact `w`: both sides of every bound the parser keeps, and every word at 2^32 and 2^63.
    Most are refused; refusal() says which."""
    assert refusal(w) is None
    h = [int(x) for x in w[:HDR]]
    sec, words = sections(w)
    n = 1 << h[A["ART_DEGREE_BITS"]]
    out = [("magic", [("s", 0, h[0] ^ 1)]), ("version 1", [("s", 1, 1)]), ("version 6", [("s", 1, 6)])]
    out += [("prefix of %d words" % k, [("t", k)]) for k in range(HDR + 1)] + [("one word short", [("t", words - 1)]), ("one word long", [("a", 0)])]
    num_wires, routed, n_sc = h[A["ART_NUM_WIRES"]], h[A["ART_NUM_ROUTED_WIRES"]], h[A["ART_NUM_SELECTORS"]] + h[A["ART_NUM_CONSTANTS"]]
    n_rows, n_ops, lde_bits = h[A["ART_N_ROWS"]], h[A["ART_N_OPS"]], h[A["ART_DEGREE_BITS"]] + h[A["ART_RATE_BITS"]]
    # name -> the values on both sides of its bounds; the words with no bound of their own get the two sides of 2^32
    bounded = dict(
        ART_DEGREE_BITS=(0, 1, 24, 25, 28 - h[A["ART_RATE_BITS"]], 29 - h[A["ART_RATE_BITS"]]), ART_RATE_BITS=(0, 4, 5, 28 - h[A["ART_DEGREE_BITS"]], 29 - h[A["ART_DEGREE_BITS"]]),
        ART_NUM_WIRES=(0, 1, routed - 1, routed, 1024, 1025), ART_NUM_ROUTED_WIRES=(num_wires, num_wires + 1),
        ART_NUM_CONSTANTS=(64 - h[A["ART_NUM_SELECTORS"]], 65 - h[A["ART_NUM_SELECTORS"]]), ART_NUM_SELECTORS=(64 - h[A["ART_NUM_CONSTANTS"]], 65 - h[A["ART_NUM_CONSTANTS"]]),
        ART_NUM_CHALLENGES=(0, 1, 4, 5), ART_MAX_DEGREE=(0, 1, U32), ART_NUM_PARTIAL_PRODUCTS=(h[A["ART_NUM_PARTIAL_PRODUCTS"]] - 1, h[A["ART_NUM_PARTIAL_PRODUCTS"]] + 1, U32),
        ART_NUM_GATES=(MAX_GATES, MAX_GATES + 1), ART_CAP_HEIGHT=(0, lde_bits, lde_bits + 1, 20, 21), ART_POW_BITS=(0, U32), ART_NUM_QUERIES=(0, U32),
        ART_N_FRI_LAYERS=(0, 32, 33), ART_ZERO_KNOWLEDGE=(0, 1, U32), ART_HASHER=(0, 1, 2), ART_BLIND_START=(n - h[A["ART_N_BLIND"]], n - h[A["ART_N_BLIND"]] + 1, U32),
        ART_N_BLIND=(n - h[A["ART_BLIND_START"]], n - h[A["ART_BLIND_START"]] + 1, U32),
        ART_Z_START=(n - 2 * h[A["ART_N_Z_PAIRS"]], n - 2 * h[A["ART_N_Z_PAIRS"]] + 1, U32),
        ART_N_Z_PAIRS=((n - h[A["ART_Z_START"]]) // 2, (n - h[A["ART_Z_START"]]) // 2 + 1, U32),
        ART_N_ROWS=(n, n + 1), ART_N_OPS=(1 << 28, (1 << 28) + 1), ART_N_INPUTS=(0, M64), ART_N_PI=(1 << 20, (1 << 20) + 1),
        ART_N_SEQ=(n_ops, n_ops + 1), ART_N_SEGS=(n_ops, n_ops + 1))
    for name, values in bounded.items():
        out += [("%s = %d" % (name, v), [("s", A[name], v)]) for v in sorted(set(values + (1 << 32, (1 << 32) + h[A[name]], 1 << 63))) if v >= 0]
    out.append(("num_selectors = 2^32 - 1 with num_constants = 2", [("s", A["ART_NUM_SELECTORS"], U32), ("s", A["ART_NUM_CONSTANTS"], 2)]))
    out.append(("blind_start + n_blind = n + 1", [("s", A["ART_BLIND_START"], n - 2), ("s", A["ART_N_BLIND"], 3)]))
    out.append(("z_start + 2 n_z_pairs = n + 1", [("s", A["ART_Z_START"], n - 3), ("s", A["ART_N_Z_PAIRS"], 2)]))
    out.append(("z_start + 2 n_z_pairs wraps in 64 bits", [("s", A["ART_Z_START"], 2), ("s", A["ART_N_Z_PAIRS"], 1 << 63)]))
    # gate fields at their bounds, on the first and the last gate
    for g in sorted({0, h[A["ART_NUM_GATES"]] - 1}):
        at = A["ART_GATES"] + 5 * g
        t, p, sel, start, end = h[at:at + 5]
        for k, name in enumerate(("type", "parameter", "selector_index", "group_start", "group_end")):
            out += [("gate %d: %s = %s" % (g, name, v), [("s", at + k, v)]) for v in (1 << 32, (1 << 32) + h[at + k], 1 << 63)]
        out += [("gate %d: type 13" % g, [("s", at, 13)]), ("gate %d: type 12" % g, [("s", at, 12)]),
                ("gate %d: selector_index = num_selectors" % g, [("s", at + 2, h[A["ART_NUM_SELECTORS"]])]),
                ("gate %d: selector_index = num_selectors - 1" % g, [("s", at + 2, h[A["ART_NUM_SELECTORS"]] - 1)]),
                ("gate %d: group_start > group_end" % g, [("s", at + 3, end + 1)]), ("gate %d: group_start = group_end" % g, [("s", at + 3, end)]),
                ("gate %d: group_end = num_gates + 1" % g, [("s", at + 4, h[A["ART_NUM_GATES"]] + 1)]), ("gate %d: group_end = num_gates" % g, [("s", at + 4, h[A["ART_NUM_GATES"]])]),
                ("gate %d: a ReducingGate without coefficients" % g, [("s", at, 10), ("s", at + 1, 0)]),
                ("gate %d: a ConstantGate of num_constants + 1 constants" % g, [("s", at, 1), ("s", at + 1, h[A["ART_NUM_CONSTANTS"]] + 1)]),
                ("gate %d: a ConstantGate of num_constants constants" % g, [("s", at, 1), ("s", at + 1, h[A["ART_NUM_CONSTANTS"]])])]
    # a used gate slot beyond num_gates holds anything
    if h[A["ART_NUM_GATES"]] < MAX_GATES:
        out.append(("an unused gate slot of type 2^63", [("s", A["ART_GATES"] + 5 * h[A["ART_NUM_GATES"]], 1 << 63)]))
    at, n_layers = sec["arity"]
    if n_layers:
        bits = [int(x) for x in w[at:at + n_layers]]
        out += [("arity word %d = %d" % (l, v), [("s", at + l, v)]) for l in sorted({0, n_layers - 1}) for v in (0, 1, 4, 5, 1 << 32, (1 << 32) + bits[l])]
        spare = h[A["ART_DEGREE_BITS"]] - sum(bits)
        if bits[-1] + spare + 1 <= MAX_ARITY_BITS:
            out += [("the arity bits sum to degree_bits", [("s", at + n_layers - 1, bits[-1] + spare)]), ("the arity bits sum to degree_bits + 1", [("s", at + n_layers - 1, bits[-1] + spare + 1)])]
        # the cap as high as the last layer is wide, and one more
        last = lde_bits - sum(bits)
        if last + 1 <= 20:
            out += [("the last FRI layer as wide as the cap", [("s", A["ART_CAP_HEIGHT"], last)]), ("a FRI layer narrower than the cap", [("s", A["ART_CAP_HEIGHT"], last + 1)])]
    at, length = sec["row_idx"]
    if length:
        out += [("the last row index = n", [("s", at + length - 1, n)]), ("the last row index = n - 1", [("s", at + length - 1, n - 1)]), ("the first row index = 2^32", [("s", at, 1 << 32)])]
    at, length = sec["pi_pos"]
    if length:
        out += [("a public-input position = n_rows * num_wires", [("s", at + length - 1, n_rows * num_wires)]),
                ("a public-input position = n_rows * num_wires - 1", [("s", at + length - 1, n_rows * num_wires - 1)])]
    at, length = sec["seg_lens"]
    if length:
        last = int(w[at + length - 1])
        out += [("the segment lengths sum to n_ops + 1", [("s", at + length - 1, last + 1)]), ("the segment lengths sum to n_ops - 1", [("s", at + length - 1, last - 1)]),
                ("a segment length of 2^64 - 1", [("s", at, M64)]), ("the segment lengths wrap around to n_ops", [("s", at, (int(w[at]) - 1) & M64), ("s", at + length - 1, last + 1)])]
        if length > 1:
            out.append(("two segment lengths that wrap around to their sum", [("s", at, (1 << 63) + int(w[at])), ("s", at + 1, (1 << 63) + int(w[at + 1]))]))
    at, length = sec["tape"]
    if length:
        tape = w[at:at + length].reshape(-1, 5)
        out += [("tape entry 0: opcode 15", [("s", at, 15)]), ("the last tape entry: opcode 2^32", [("s", at + length - 5, 1 << 32)])]
        k = int(np.nonzero(tape[:, 0] == 1)[0][0])                  # an INPUT entry: {1, wire, input}
        out += [("tape entry %d: input n_inputs" % k, [("s", at + 5 * k + 2, h[A["ART_N_INPUTS"]])]),
                ("tape entry %d: input n_inputs - 1" % k, [("s", at + 5 * k + 2, h[A["ART_N_INPUTS"]] - 1)]),
                ("tape entry %d: wire n_rows * num_wires" % k, [("s", at + 5 * k + 1, n_rows * num_wires)]),
                ("tape entry %d: wire n_rows * num_wires - 1" % k, [("s", at + 5 * k + 1, n_rows * num_wires - 1)]),
                ("n_inputs one less than the tape reads", [("s", A["ART_N_INPUTS"], int(tape[tape[:, 0] == 1][:, 2].max()))]),
                ("n_inputs = what the tape reads", [("s", A["ART_N_INPUTS"], int(tape[tape[:, 0] == 1][:, 2].max()) + 1)])]
    return out


def refused(w):
    """[(what, edits, (code, message))]: the cases of mutations(w) that the parser refuses"""
    out = []
    for what, edits in mutations(w):
        why = refusal(apply(w, edits))
        if why is not None:
            out.append((what, edits, why))
    return out
