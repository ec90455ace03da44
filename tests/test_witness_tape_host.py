"""CPU: the witness tape's entry contract (stark-verifier_amd/csrc/witness_tape.h) under host sanitizers.

tests/witness_tape_check.cpp -- a program with its own main, linked with the host replay (witness_tape.cpp) and the two units it
calls into -- is compiled with the host compiler of csrc/Makefile under AddressSanitizer and UBSan, as tests/test_host_field.py does
for the field class.  It gives gl355_witness_replay one-entry tapes over heap rows of exactly 3 x 135 words: the REDUCING counts
whose wire sums wrapped in 64 bits, the accepted and the refused boundary of every opcode, and a seeded sweep of 20 000 entries, in
which tape_entry_fits and the replay's return code must agree and every accepted entry must stay inside the rows (a sanitizer
report aborts the program).  Nothing is loaded into Python."""
import os
import subprocess

import pytest

from test_host_field import CSRC, FLAGS, ROOT, host_compiler

SOURCES = [os.path.join(ROOT, "tests", "witness_tape_check.cpp")] + [os.path.join(CSRC, f) for f in ("witness_tape.cpp", "host_transcript.cpp", "host_bn254.cpp")]


def test_fits_and_replay_agree_and_stay_inside_the_rows(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "witness_tape_check")
    subprocess.run([cxx] + FLAGS + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-pthread"] + SOURCES + ["-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.count("sweep ") == 15
