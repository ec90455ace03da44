"""CPU: the circuit artifact's arity table (CircuitData.export_blob(..., wide_arity=True), versions 4 and 5; layout in include/gl355.h).
The circuit is the committed [2, 3] fixture's (tests/golden/fri_arity_proof.json), laid out on the host; the artifact is held, word
for word, against the documented layout assembled here from the circuit data, and the default export of an arity-2 circuit against
itself: versions 2 and 3 do not change."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import fri_arity_cases as fc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_arity_proof.json")
HDR = 112          # header words; the arity table of versions 4 / 5 follows directly


def _u64(a):
    return np.asarray(a, dtype=np.uint64).reshape(-1)


def built(arities):
    """the fixture's circuit at `arities` (layout, tables and digest on the host) and the sparse row map of its witness"""
    g = json.load(open(FIXTURE))
    plonk = importlib.import_module("stark-verifier_amd.plonk")
    b, _ = fc.small_circuit(plonk.CircuitConfig(**dict(g["config"], reduction_arity_bits=arities)), g["circuit_seed"])
    data = b.cb.layout(g["min_degree_bits"])
    data.set_digest(np.array(g["constants_sigmas_cap"], dtype=np.uint64))
    idx, _ = b.sparse_witness()
    return data, np.asarray(idx, dtype=np.uint64)


def documented_layout(data, idx, version, digest):
    """include/gl355.h, "circuit artifacts", restated: version 2 / 3 without a table, 4 / 5 with the arity bits after the header"""
    cfg, cc = data.config, data.c_circuit
    hdr = np.zeros(HDR, dtype=np.uint64)
    hdr[0], hdr[1] = int.from_bytes(b"GL355CIR", "little"), version
    hdr[2:12] = [cc.degree_bits, cc.rate_bits, cc.num_wires, cc.num_routed_wires, cc.num_constants, cc.num_selectors, cc.num_challenges,
                 cc.max_degree, cc.num_partial_products, cc.num_gates]
    for k in range(16):
        gt = cc.gates[k]
        hdr[12 + 5 * k:17 + 5 * k] = [gt.type, gt.param, gt.selector_index, gt.group_start, gt.group_end]
    start, n_blind, z_pairs, _ = data.blind_rows
    hdr[92:106] = [cfg.cap_height, cfg.proof_of_work_bits, cfg.num_query_rounds, len(data.fri_arity_bits), int(cfg.zero_knowledge), cfg.hasher,
                   start, n_blind, z_pairs[0][0] if z_pairs else 0, len(z_pairs), idx.size, 0, 0, 0]
    hdr[106:110] = digest
    table = _u64(data.fri_arity_bits) if version >= 4 else _u64([])
    cap = _u64(data.constants_sigmas_cap) if version in (3, 5) else _u64([])
    return np.concatenate([hdr, table, _u64(data.constants), _u64(data.sigmas), _u64(data.k_is), idx, cap])


@pytest.fixture(scope="module")
def wide():
    return built([2, 3])


@pytest.fixture(scope="module")
def narrow():
    return built(1)


def test_the_default_export_still_refuses_a_wide_circuit_and_names_the_keyword(wide):
    data, idx = wide
    assert data.fri_arity_bits == [2, 3]
    with pytest.raises(ValueError, match="arity-2 FRI only") as ei:
        data.export_blob(idx)
    assert "wide_arity" in str(ei.value)
    with pytest.raises(ValueError, match="arity-2 FRI only"):
        data.export_blob(idx, external_digest=[1, 2, 3, 4])


def test_the_documented_layout_is_what_export_blob_writes_for_versions_2_and_3(narrow):
    """the restatement above is held against the unchanged writer first, so that it can stand for "the version-2 layout" below"""
    data, idx = narrow
    assert data.fri_arity_bits and all(a == 1 for a in data.fri_arity_bits)
    assert np.array_equal(data.export_blob(idx), documented_layout(data, idx, 2, data.circuit_digest))
    ext = np.array([5, 6, 7, 8], dtype=np.uint64)
    assert np.array_equal(data.export_blob(idx, external_digest=ext), documented_layout(data, idx, 3, ext))


@pytest.mark.parametrize("external", [False, True], ids=["version 4", "version 5"])
def test_wide_arity_writes_the_table_after_the_header(wide, external):
    data, idx = wide
    ext = np.array([5, 6, 7, 8], dtype=np.uint64) if external else None
    blob = data.export_blob(idx, external_digest=ext, wide_arity=True)
    assert blob.dtype == np.uint64
    assert int(blob[1]) == (5 if external else 4)
    assert int(blob[95]) == 2 and [int(v) for v in blob[HDR:HDR + 2]] == [2, 3]
    # the version-2 / 3 layout of the same circuit: the length grows by exactly the table, every other word is equal
    base = documented_layout(data, idx, 3 if external else 2, ext if external else data.circuit_digest)
    assert blob.size == base.size + 2
    assert np.array_equal(blob[2:HDR], base[2:HDR]) and blob[0] == base[0]
    assert np.array_equal(blob[HDR + 2:], base[HDR:])
    assert np.array_equal(blob, documented_layout(data, idx, 5 if external else 4, ext if external else data.circuit_digest))
    if external:
        assert np.array_equal(blob[-8:], _u64(data.constants_sigmas_cap))


def test_an_arity_2_circuit_differs_by_the_version_word_and_a_table_of_ones(narrow):
    data, idx = narrow
    L = len(data.fri_arity_bits)
    for ext, v in ((None, 2), (np.array([5, 6, 7, 8], dtype=np.uint64), 3)):
        plain = data.export_blob(idx, external_digest=ext)
        tabled = data.export_blob(idx, external_digest=ext, wide_arity=True)
        assert int(plain[1]) == v and int(tabled[1]) == v + 2
        assert tabled.size == plain.size + L and [int(a) for a in tabled[HDR:HDR + L]] == [1] * L
        assert np.array_equal(np.delete(tabled, np.r_[1, HDR:HDR + L]), np.delete(plain, 1))


def test_the_default_blob_does_not_depend_on_the_new_path(narrow):
    data, idx = narrow
    before = hashlib.sha256(data.export_blob(idx).tobytes()).hexdigest()
    data.export_blob(idx, wide_arity=True)
    assert hashlib.sha256(data.export_blob(idx).tobytes()).hexdigest() == before
    assert hashlib.sha256(data.export_blob(idx, wide_arity=False).tobytes()).hexdigest() == before
