"""CPU: the one host statement of the circuit artifact (stark-verifier_amd/csrc/circuit_artifact.h) under host sanitizers.

tests/circuit_artifact_check.cpp -- a program with its own main that includes circuit_artifact.h and is linked with witness_tape.cpp and the
two host units that calls into -- is compiled with the host compiler of csrc/Makefile under AddressSanitizer and UBSan, as
tests/test_plonk_desc_host.py does for the Halo2 descriptor.  It reads a base artifact from a file into a heap block of exactly its length,
applies each case's edits (a block of its own whenever the length changes), runs artifact_parse and prints the refusal or the whole view
after reading every word of every section through it: a read outside the artifact is a sanitizer report, which aborts the program.
Nothing is loaded into Python.

Bases, all made on the CPU: the gate-zoo circuit of tests/test_artifact_arity_host.py in the four version layouts, and the outer verifier
circuit of tests/test_recursion_arity_host.py with its tape, three segments and public-input positions.  Accepted artifacts are compared
with the CircuitData and the arguments of export_blob; the mutation list of tests/circuit_artifact_cases.py and a seeded sweep of single-word
header corruptions with that file's statement of the bounds in Python integers."""
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import circuit_artifact_cases as cac
from test_artifact_arity_host import built
from test_host_field import CSRC, FLAGS, ROOT, host_compiler
from test_recursion_arity_host import golden, outer                # noqa: F401 (fixtures)

plonk = importlib.import_module("stark-verifier_amd.plonk")
A = plonk.ARTIFACT_WORDS
SOURCES = [os.path.join(ROOT, "tests", "circuit_artifact_check.cpp")] + [os.path.join(CSRC, f) for f in ("witness_tape.cpp", "host_transcript.cpp", "host_bn254.cpp")]
EXT = np.array([5, 6, 7, 8], dtype=np.uint64)


@pytest.fixture(scope="module")
def zoo():
    """version -> (CircuitData, row map, export_blob's keywords, artifact) of the gate-zoo circuit: arity 2 for versions 2 / 3, [2, 3] for 4 / 5"""
    out = {}
    for version, arities, kw in ((2, 1, {}), (3, 1, dict(external_digest=EXT)), (4, [2, 3], dict(wide_arity=True)), (5, [2, 3], dict(wide_arity=True, external_digest=EXT))):
        data, idx = built(arities)
        out[version] = (data, idx, kw, data.export_blob(idx, **kw))
    return out


@pytest.fixture(scope="module")
def recursive(golden, outer):
    """the outer verifier circuit: (CircuitData, export_blob's arguments, artifact)"""
    b = outer["b"]
    data = b.cb.layout(0)
    data.set_digest(np.arange(8, dtype=np.uint64).reshape(2, 4) + 1)        # cap height 1: any cap, the digest is the loader's to compare
    n_inputs = golden["flat"].size + len(golden["pi"])
    kw = dict(tape=outer["tape"], pi_pos=outer["pi_pos"], n_inputs=n_inputs, tape_layout=b.tape_layout, wide_arity=True)
    return data, outer["idx"], kw, data.export_blob(outer["idx"], **kw)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    path = str(tmp_path_factory.mktemp("circuit_artifact") / "circuit_artifact_check")
    subprocess.run([cxx] + FLAGS + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-pthread"] + SOURCES + ["-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def ask(exe, tmp_path_factory):
    where = tmp_path_factory.mktemp("circuit_artifact_bases")
    files = {}

    def ask(base, cases):
        """the program's answers to `cases` (lists of edits) of the artifact `base`"""
        key = base.tobytes()
        if key not in files:
            files[key] = str(where / ("base%d.bin" % len(files)))
            base.astype("<u8").tofile(files[key])
        res = subprocess.run([exe, files[key]], input="".join(cac.line(e) + "\n" for e in cases), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        got = res.stdout.splitlines()
        assert len(got) == len(cases)
        return got
    return ask


def want(w):
    why = cac.refusal(w)
    return cac.view(w) if why is None else "refused %d %s" % why


def check(ask, base, cases):
    """cases: (what, edits); every answer is the refusal or the view this file expects"""
    got = ask(base, [e for _, e in cases])
    bad = [(what, want(cac.apply(base, e)), g) for (what, e), g in zip(cases, got) if g != want(cac.apply(base, e))]
    assert not bad, "%d of %d artifacts differ, the first (what, expected, answer): %r" % (len(bad), len(cases), bad[0])
    return got


def expected_view(data, idx, version, digest, tape=None, pi_pos=(), n_inputs=0, tape_layout=None):
    """the program's answer to an artifact, from the CircuitData and the arguments of export_blob alone"""
    cfg, cc = data.config, data.c_circuit
    n = 1 << cc.degree_bits
    gates = ["%d/%d/%d/%d/%d" % (g.type, g.param, g.selector_index, g.group_start, g.group_end) for g in list(cc.gates)[:cc.num_gates]]
    start, n_blind, z_pairs, _ = data.blind_rows
    n_ops = 0 if tape is None else tape.shape[0]
    n_seq, seg_lens = tape_layout if tape_layout is not None else (n_ops, [])
    L = len(data.fri_arity_bits)
    lens = [L if version >= 4 else 0, (cc.num_selectors + cc.num_constants) * n, cc.num_routed_wires * n, cc.num_routed_wires, idx.size, len(pi_pos), 5 * n_ops,
            len(seg_lens), 4 << cfg.cap_height if version in (3, 5) else 0]
    offsets = [112 + sum(lens[:k]) for k in range(9)]
    parts = [[version, int(version in (3, 5)), int(version >= 4)],
             [cc.degree_bits, cc.rate_bits, cc.num_wires, cc.num_routed_wires, cc.num_constants, cc.num_selectors, cc.num_challenges, cc.max_degree, cc.num_partial_products,
              cc.num_gates], gates,
             [cfg.cap_height, cfg.proof_of_work_bits, cfg.num_query_rounds, L, int(cfg.zero_knowledge), cfg.hasher], list(data.fri_arity_bits) if version >= 4 else [1] * L,
             [start, n_blind, z_pairs[0][0] if z_pairs else 0, len(z_pairs)], [idx.size, n_ops, n_inputs, len(pi_pos), n_seq, len(seg_lens)],
             ["%x" % int(x) for x in digest], ["%d:%d" % (o, l) for o, l in zip(offsets, lens)]]
    return cac.render(parts)


def test_the_enum_is_the_writers_table_and_every_message_is_stated_once(exe):
    names = subprocess.run([exe, "names"], capture_output=True, text=True, check=True).stdout.split()
    assert dict(zip(names[::2], (int(v) for v in names[1::2]))) == A and len(names) == 2 * len(A)
    messages = subprocess.run([exe, "messages"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(set(messages)) == len(messages) == 26 and all(m.split(" ", 1)[1].startswith("circuit_load: ") for m in messages)
    assert {int(m.split()[0]) for m in messages} == {cac.INVALID_ARG, cac.UNSUPPORTED}


@pytest.mark.parametrize("version", [2, 3, 4, 5])
def test_the_view_of_each_version_equals_the_circuit_data(ask, zoo, version):
    data, idx, kw, blob = zoo[version]
    assert int(blob[A["ART_VERSION"]]) == version
    got, = ask(blob, [[]])
    assert got == expected_view(data, idx, version, kw.get("external_digest", data.circuit_digest))
    assert got == cac.view(blob) and cac.refusal(blob) is None


def test_the_view_of_the_outer_verifier_circuit_equals_its_export_arguments(ask, recursive):
    data, idx, kw, blob = recursive
    n_seq, seg_lens = kw["tape_layout"]
    assert len(seg_lens) == 3 and kw["pi_pos"].size > 0 and kw["tape"].shape[0] > 1000 and kw["n_inputs"] > 100
    got, = ask(blob, [[]])
    assert got == expected_view(data, idx, 4, data.circuit_digest, kw["tape"], kw["pi_pos"], kw["n_inputs"], kw["tape_layout"])
    assert got == cac.view(blob) and cac.refusal(blob) is None


def test_mutation_lists_reach_every_message_and_both_verdicts(exe, ask, zoo, recursive):
    messages = set(subprocess.run([exe, "messages"], capture_output=True, text=True, check=True).stdout.splitlines())
    seen, n_ok = set(), 0
    for blob in [zoo[v][3] for v in (2, 3, 4, 5)] + [recursive[3]]:
        cases = cac.mutations(blob)
        got = check(ask, blob, cases)
        seen |= {g[len("refused "):] for g in got if g.startswith("refused")}
        n_ok += sum(1 for g in got if g.startswith("ok"))
        answers = dict(zip((what for what, _ in cases), got))
        # the defects the parent's loader let through
        assert answers["ART_MAX_DEGREE = 0"] == "refused -1 circuit_load: max_degree is zero"
        assert answers["num_selectors = 2^32 - 1 with num_constants = 2"] == "refused -1 circuit_load: implausible circuit shape"
        assert answers["ART_DEGREE_BITS = %d" % ((1 << 32) + int(blob[A["ART_DEGREE_BITS"]]))] == "refused -1 circuit_load: implausible circuit shape"
        assert answers["ART_NUM_CHALLENGES = 0"] == answers["ART_NUM_CHALLENGES = 5"] == "refused -5 circuit_load: 1 to 4 challenges"
        assert answers["ART_RATE_BITS = 5"] == "refused -5 circuit_load: unsupported size" and answers["ART_RATE_BITS = 4"].startswith("ok")
        assert answers["z_start + 2 n_z_pairs wraps in 64 bits"] == "refused -1 circuit_load: blinding rows out of range"
        assert answers.get("an unused gate slot of type 2^63", cac.view(blob)) == cac.view(blob)       # not part of the circuit
    gate_messages = {m for m in seen if re.search(r": gate \d", m)}
    assert seen - gate_messages == messages, (messages - seen, seen - gate_messages - messages)
    assert all(any(kind in m for m in gate_messages) for kind in cac.GATE_MESSAGES)
    assert n_ok > 100


@pytest.mark.parametrize("base", ["version 2", "version 5", "outer verifier"])
def test_seeded_sweep_of_single_word_header_corruptions(ask, zoo, recursive, base):
    blob = {"version 2": zoo[2][3], "version 5": zoo[5][3], "outer verifier": recursive[3]}[base]
    rng = random.Random(0xA27F + len(base))
    used = [i for i in range(cac.HDR) if not A["ART_GATES"] + 5 * int(blob[A["ART_NUM_GATES"]]) <= i < A["ART_CAP_HEIGHT"]]
    cases = []
    for _ in range(2000):
        at = rng.choice(used) if rng.randrange(4) else rng.randrange(cac.HDR)
        old = int(blob[at])
        new = (old ^ 1 << rng.randrange(64), rng.getrandbits(64), rng.randrange(40), (old + rng.choice((-1, 1))) & cac.M64, old | rng.randrange(1, 4) << 32,
               old ^ 1 << rng.randrange(6))[rng.randrange(6)]
        cases.append(("word %d: %x -> %x" % (at, old, new), [("s", at, new)]))
    got = check(ask, blob, cases)
    n_ok = sum(1 for g in got if g.startswith("ok"))
    assert 100 < n_ok < 1900, n_ok                                                 # the sweep sees both verdicts often
