"""GPU: gl355_circuit_load refuses what the host parser refuses (csrc/circuit_artifact.h), in the parser's words.  The base is the version-4
artifact of the degree-2^6 gate-zoo circuit of tests/test_gpu_artifact_arity.py; the cases are the refused ones of the mutation list of
tests/circuit_artifact_cases.py, which tests/test_circuit_artifact_host.py holds against the parser under host sanitizers.  Only refusals
and the untouched artifact are handed to the loader: a mutation the parser accepts describes a circuit this test has no witness for, and
is neither loaded nor proven with."""
import ctypes as C

import numpy as np
import pytest

import circuit_artifact_cases as cac
from test_gpu_artifact_arity import case

pytestmark = pytest.mark.gpu


def test_the_loader_refuses_the_mutation_list_in_the_parsers_words(gl, ctx):
    c = case(ctx, [2, 3])
    plonk, blob = c["plonk"], c["blob"]
    assert int(blob[1]) == 4 and int(blob[2]) == 6
    refused = cac.refused(blob)
    assert len(refused) > 200 and {code for _, _, (code, _) in refused} == {cac.INVALID_ARG, cac.UNSUPPORTED}
    bad = []
    for what, edits, (code, message) in refused:
        w = np.ascontiguousarray(cac.apply(blob, edits))
        h = C.c_void_p()
        rc = ctx.lib.gl355_circuit_load(ctx.h, w.ctypes.data, w.size, C.byref(h))
        said = (ctx.lib.gl355_last_error(ctx.h) or b"").decode()
        if (rc, said, h.value) != (code, message, None):
            bad.append((what, (code, message), (rc, said, h.value)))
    assert not bad, "%d of %d refusals differ, the first (what, expected, answer): %r" % (len(bad), len(refused), bad[0])
    # afterwards the untouched artifact loads, with a handle of its own, and the context goes on working
    assert plonk.NativeCircuit(ctx, blob).fri_arity_bits == [2, 3]
    x = np.arange(16, dtype=np.uint64).reshape(2, 8)
    got = ctx.hash_no_pad(x)
    assert all(np.array_equal(got[i], plonk.host_hash_no_pad(x[i])) for i in range(2))
