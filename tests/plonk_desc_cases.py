"""Malformed Halo2 descriptors (include/gl355.h, stark-verifier_amd/halo2.py export_desc) for the host check of csrc/plonk_desc.h
(tests/test_plonk_desc_host.py), gl355_plonk_vk_create (tests/test_plonk_verify_host.py) and gl355_plonk_keygen / gl355_plonk_check_witness
(tests/test_gpu_halo2.py): one mutation list, and this file's own statement of the parser's bounds in Python integers.  A descriptor here is
a list of Python integers, one per u64 word."""
HDR = 24
MAGIC = 0x4B4C503535334C47
MAX_K_DEVICE, MAX_K_VERIFIER = 24, 28
# header word -> (least, greatest) accepted value; word 2 is k, whose greatest value is the entry point's
BOUNDS = {3: (0, 256), 4: (0, 256), 5: (0, 16), 6: (0, 256), 7: (0, 64), 8: (3, 10), 9: (3, 64), 10: (0, 1024), 11: (0, 1024), 12: (0, 64),
          13: (0, 4096), 14: (0, 1 << 20), 15: (0, 1 << 20)}
NOT_QUERIED = "a permutation column is not queried at the current rotation"       # the entry points' own check, after the parser's


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def refusal(w, max_k):
    """what the parser says of the descriptor `w` (None: accepted), from the format's definition alone"""
    if len(w) < HDR:
        return "null or truncated descriptor"
    if w[0] != MAGIC or w[1] != 1:
        return "not a version-1 gl355 PLONK descriptor"
    if not 3 <= w[2] <= max_k or any(not BOUNDS[i][0] <= w[i] <= BOUNDS[i][1] for i in BOUNDS):
        return "implausible circuit shape"
    k, cols, n_perm, n_lookups, bf, nq, n_consts, gate_len = w[2], w[3:6], w[6], w[7], w[9], w[10:13], w[13], w[14]
    if 2 ** k < bf + 3:
        return "fewer rows than the blinding needs"
    pos = HDR
    if len(w) - pos < n_perm:
        return "truncated descriptor"
    for j in range(n_perm):
        kind, idx = w[pos + j] >> 32, w[pos + j] & 0xFFFFFFFF
        if kind > 2 or idx >= cols[kind]:
            return "bad permutation column"
    pos += n_perm
    for kd in range(3):
        if len(w) - pos < nq[kd]:
            return "truncated descriptor"
        for q in range(nq[kd]):
            col, rot = _s32(w[pos + q] >> 32), _s32(w[pos + q])
            if not 0 <= col < cols[kd] or abs(rot) > bf + 1:
                return "bad query"
        pos += nq[kd]
    if len(w) - pos < 4 * n_consts:
        return "truncated descriptor"
    pos += 4 * n_consts

    def program(length):
        nonlocal pos
        if len(w) - pos < 2 * length:
            return False
        u32 = [x for word in w[pos:pos + 2 * length] for x in (word & 0xFFFFFFFF, word >> 32)]
        pos += 2 * length
        for i in range(length):
            op, dst = u32[4 * i], u32[4 * i + 1]
            if op > 5 or dst >= 12:
                return False
            for v in u32[4 * i + 2:4 * i + (4 if op <= 2 else 3)]:
                kind, idx = v >> 24, v & 0xFFFFFF
                limit = 12 if kind == 0 else n_consts if kind == 1 else nq[kind - 2] if kind <= 4 else 0
                if idx >= limit:
                    return False
        return True
    if not program(gate_len):
        return "bad gate program"
    for _ in range(n_lookups):
        if len(w) - pos < 2:
            return "truncated descriptor"
        li, lt = w[pos], w[pos + 1]
        pos += 2
        if li > 1 << 16 or lt > 1 << 16 or not program(li) or not program(lt):
            return "bad lookup program"
    if pos != len(w):
        return "descriptor length does not match its header"
    return None


def perm_queries(w):
    """of an accepted descriptor: per permutation column the index, among its kind's queries, of (column, 0); None if a column has none"""
    starts = [HDR + w[6]]
    for kd in range(3):
        starts.append(starts[-1] + w[10 + kd])
    out = []
    for j in range(w[6]):
        kind, idx = w[HDR + j] >> 32, w[HDR + j] & 0xFFFFFFFF
        qs = [(_s32(x >> 32), _s32(x)) for x in w[starts[kind]:starts[kind + 1]]]
        if (idx, 0) not in qs:
            return None
        out.append(qs.index((idx, 0)))
    return out


def programs(w):
    """of a well-formed descriptor: (offset of the first word, instructions) of the gate program and of every lookup's two programs, and the
    offsets of the lookups' length words"""
    pos = HDR + w[6] + w[10] + w[11] + w[12] + 4 * w[13]
    out, lens = [(pos, w[14])], []
    pos += 2 * w[14]
    for _ in range(w[7]):
        lens.append(pos)
        li, lt = w[pos], w[pos + 1]
        out += [(pos + 2, li), (pos + 2 + 2 * li, lt)]
        pos += 2 + 2 * li + 2 * lt
    assert pos == len(w)
    return out, lens


def _with(w, at, value):
    out = list(w)
    out[at] = value
    return out


def _with_u32(w, word, half, value):
    """the descriptor with one u32 of word `word` replaced (half 0: the low one)"""
    keep = w[word] & (0xFFFFFFFF << 32 if half == 0 else 0xFFFFFFFF)
    return _with(w, word, keep | (value << (32 * half)))


def mutations(w, max_k):
    """[(what, descriptor)] around the well-formed descriptor `w`: both sides of every bound the parser keeps.  Most are refused, the values
    on the inner side of a bound are accepted where nothing else of the descriptor depends on them; refusal() says which."""
    assert refusal(w, max_k) is None and perm_queries(w) is not None
    out = [("magic", _with(w, 0, w[0] ^ 1)), ("version 2", _with(w, 1, 2)), ("version 0", _with(w, 1, 0))]
    out += [("prefix of %d words" % n, w[:n]) for n in range(len(w))] + [("one word more", list(w) + [0])]
    for i, values in [(2, (2, 3, max_k, max_k + 1))] + [(i, (lo - 1, lo, hi, hi + 1)) for i, (lo, hi) in sorted(BOUNDS.items())]:
        out += [("header word %d = %d" % (i, v), _with(w, i, v)) for v in values + (1 << 32, 1 << 63) if v >= 0]
    out.append(("n < bf + 3", _with(_with(w, 2, 3), 9, 6)))
    bf, cols, n_consts, nq = w[9], w[3:6], w[13], w[10:13]
    if w[6]:
        kind = w[HDR] >> 32
        out += [("permutation column of kind 3", _with(w, HDR, 3 << 32 | w[HDR] & 0xFFFFFFFF)),
                ("permutation column %d of kind %d" % (cols[kind], kind), _with(w, HDR, kind << 32 | cols[kind]))]
    at = HDR + w[6]
    for kd in range(3):
        if nq[kd]:
            out += [("query of kind %d: column %d" % (kd, cols[kd]), _with_u32(w, at, 1, cols[kd])), ("query of kind %d: column -1" % kd, _with_u32(w, at, 1, 0xFFFFFFFF))]
            out += [("query of kind %d: rotation %d" % (kd, r), _with_u32(w, at, 0, r & 0xFFFFFFFF)) for r in (bf + 1, -bf - 1, bf + 2, -bf - 2)]
        at += nq[kd]
    progs, lens = programs(w)
    operands = [(0, 12), (0, 11), (1, n_consts), (1, n_consts - 1)] + [(2 + kd, nq[kd] - d) for kd in range(3) for d in (0, 1)] + [(5, 0)]
    for p, (start, length) in enumerate(progs):
        for i in range(length):
            word = start + 2 * i
            fields = [("op", 0, 0, v) for v in (6, 5)] + [("register", 0, 1, v) for v in (12, 11)]
            fields += [("operand %s" % "ab"[o], 1, o, kind << 24 | idx) for o in (0, 1) for kind, idx in operands if idx >= 0]
            out += [("program %d, instruction %d: %s = 0x%x" % (p, i, name, v), _with_u32(w, word + dw, half, v)) for name, dw, half, v in fields]
    for at in lens:
        out += [("lookup input of 2^16 + 1 instructions", _with(w, at, (1 << 16) + 1)), ("lookup table of 2^16 + 1 instructions", _with(w, at + 1, (1 << 16) + 1))]
    if w[6]:                                 # the first permutation column loses its query at rotation 0: the query moves to rotation 1
        kind, idx = w[HDR] >> 32, w[HDR] & 0xFFFFFFFF
        at = HDR + w[6] + sum(nq[:kind]) + perm_queries(w)[0]
        out.append(("the first permutation column is not queried at rotation 0", _with_u32(w, at, 0, 1)))
    return out


def verdict(w, max_k):
    """the message an entry point ends with after its own prefix -- the parser's or NOT_QUERIED -- or None: accepted by both"""
    why = refusal(w, max_k)
    if why is None and perm_queries(w) is None:
        return NOT_QUERIED
    return why
