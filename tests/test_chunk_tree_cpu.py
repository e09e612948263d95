"""Not -m gpu: chunk attention under a tree mask (speckv_ext_attend_chunk_masked, SpeckvKVConnector.chunk_tree_masks /
attend_chunk(parents=...)).

The mask rows against tree_masks word for word where both apply (S <= 16) and against a brute-force ancestor walk written here beyond
that, across the word boundaries; the declarations, the export, the entry on the device-less engine; attend_chunk(parents=...)'s
refusals against a library that must not be called."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests.test_chunk_cpu import _Shape, _SilentLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
masks_of = SpeckvKVConnector.chunk_tree_masks


def _as_int(row):
    return sum(int(w) << (32 * i) for i, w in enumerate(row))


def _brute(parents, base, n):
    """a node's row as one int by walking up from it: the low `base` bits, its own bit and its ancestors'; 0 if the node or an
    ancestor is >= n"""
    rows = []
    for j in range(len(parents)):
        bits, a, live = (1 << base) - 1, j, True
        while a >= 0:
            bits |= 1 << (base + a)
            live = live and a < n
            a = parents[a]
        rows.append(bits if live else 0)
    return rows


def _random_trees(rng, batch, S):
    return [[int(rng.integers(-1, j)) for j in range(S)] for _ in range(batch)]


def test_single_word_rows_are_tree_masks_words():
    rng = np.random.default_rng(16)
    for S in range(1, 17):
        for base in (0, 1):
            trees = _random_trees(rng, 5, S)
            n_new = [int(n) for n in rng.integers(0, S + 1, size=5)]
            bases = [base, 1 - base, base, base, 1 - base] if S < 16 else [0] * 5        # (tree_masks: base + S <= 16)
            got = masks_of(trees, bases, n_new)
            want = SpeckvKVConnector.tree_masks(trees, bases, n_new)
            assert [[row for row in req] for req in got] == [[[w] for w in req] for req in want], (S, base)
            one = masks_of(trees[0], bases)                                               # one tree for every request, all live
            assert [[r[0] for r in req] for req in one] == SpeckvKVConnector.tree_masks(trees[0], bases)


@pytest.mark.parametrize("S", [17, 31, 32, 33, 63, 64, 65, 70])
def test_rows_of_large_trees_against_an_ancestor_walk(S):
    rng = np.random.default_rng(S)
    W = (S + 1 + 31) // 32
    trees = _random_trees(rng, 6, S)
    bases = [0, 1, 0, 1, 1, 0]
    n_new = [S, S, int(rng.integers(1, S)), int(rng.integers(1, S)), 0, 1]
    got = masks_of(trees, bases, n_new)
    assert len(got) == 6
    for tree, base, n, rows in zip(trees, bases, n_new, got):
        assert len(rows) == S and all(len(r) == W and all(0 <= w < 1 << 32 for w in r) for r in rows)
        assert [_as_int(r) for r in rows] == _brute(tree, base, n), (S, base, n)
    # every live row carries its own bit and nothing at or beyond base + j + 1
    for base, rows in zip(bases, got):
        for j, r in enumerate(rows):
            v = _as_int(r)
            assert v == 0 or (v >> (base + j)) == 1


@pytest.mark.parametrize("base", [0, 1])
def test_a_chain_is_the_causal_rule_across_the_word_boundaries(base):
    S = 70
    rows = masks_of(list(range(-1, S - 1)), [base])[0]
    assert [_as_int(r) for r in rows] == [(1 << (base + j + 1)) - 1 for j in range(S)]
    j = 31 - base                                                                         # the row whose own bit is bit 31
    assert rows[j] == [0xFFFFFFFF, 0, 0] and rows[j + 1] == [0xFFFFFFFF, 1, 0]
    assert rows[63 - base] == [0xFFFFFFFF, 0xFFFFFFFF, 0] and rows[64 - base] == [0xFFFFFFFF, 0xFFFFFFFF, 1]


def test_dead_nodes_and_the_nodes_below_them_give_zero_rows():
    #        -1 -> 0 -> 1 -> 40 -> 41;  -1 -> 2 -> 3;  39 is a child of the context
    S = 42
    parents = [-1, 0, -1, 2] + [3] * 35 + [-1, 1, 40]
    rows = masks_of(parents, [1], [40])[0]                                                 # nodes 40, 41 are beyond n_new
    assert rows[40] == [0, 0] and rows[41] == [0, 0] and _as_int(rows[39]) == 1 | 1 << 40
    rows = masks_of(parents, [0], [3])[0]                                                  # 3 dead, so is everything below it
    assert [_as_int(r) for r in rows[:3]] == [1, 3, 4] and all(r == [0, 0] for r in rows[3:])
    assert all(r == [0] for r in masks_of([-1, 0, 1], [1], [0])[0])
    assert masks_of([-1], []) == []


def test_malformed_parents_raise():
    for bad in ([], [0], [-2], [-1, 1], [-1, 2, 0], [-1, 0.0], [-1, True], [-1, None], [[-1, 0], [-1]], [[-1, 0]]):
        with pytest.raises(ValueError):
            masks_of(bad, [0, 0])
    for base in ([2], [-1]):
        with pytest.raises(ValueError):
            masks_of([-1, 0], base)
    for n_new in ([3], [-1], [1, 1]):
        with pytest.raises(ValueError):
            masks_of([-1, 0], [0], n_new)
    # the bounded validators keep their bound
    with pytest.raises(ValueError):
        SpeckvKVConnector.tree_masks(list(range(-1, 16)), [0])
    assert len(masks_of(list(range(-1, 16)), [0])[0]) == 17


def test_attend_chunk_masked_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    m = re.search(r"speckv_status_t\s+speckv_ext_attend_chunk_masked\s*\((.*?)\);", header, re.S)
    assert m
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.search(r"tail_stride_elems,\s*const uint32_t\*\s*d_mask,\s*uint32_t\s+mask_words,\s*float\s+sm_scale", params)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    assert header.index("speckv_ext_attend_chunk_masked(") > header.index("speckv_ext_attend_chunk(")          # added at the end
    doc = header[header.index("speckv_ext_attend_chunk_masked:"):]
    assert "IGNORED" in doc and "LIVE iff" in doc and "NOT WRITTEN" in doc and "held position base + a" in doc
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    assert any(fnmatch.fnmatchcase("speckv_ext_attend_chunk_masked", p.strip()) for p in globals_.split(";") if p.strip())
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_masked"]
    plain = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk"]
    assert sig == plain[:16] + [C.c_void_p, C.c_uint32] + plain[16:]
    assert callable(speckv_ctypes.SpeckvLib.attend_chunk_masked)


def test_the_library_exports_attend_chunk_masked_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_chunk_masked")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_attend_chunk_masked_on_the_null_engine_answers_as_attend_chunk_does():
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        one = lambda v: np.asarray([v], np.uint32)
        before = bytes(lib.stats())
        with pytest.raises(SpeckvError) as chunk:
            lib.attend_chunk(u64(a), 0, at, 1, 1, one(0), one(1), at, at, 1024, 1024, None, 0, 0, 0, 1.0, at, 0, 1)
        for d_mask, words in ((at, 1), (0, 1), (at, 0)):                                 # the missing data path is judged first
            with pytest.raises(SpeckvError) as masked:
                lib.attend_chunk_masked(u64(a), 0, at, 1, 1, one(0), one(1), at, at, 1024, 1024, None, 0, 0, 0, d_mask, words, 1.0, at, 0, 1)
            assert masked.value.status == chunk.value.status == -2                        # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


def test_attend_chunk_with_parents_raises_before_any_library_call():
    L, H, D, T, S, R = 2, 8, 128, 64, 40, 8
    conn = SpeckvKVConnector(_SilentLib(), L, H, D, T, "fp8")
    for rid in (1, 2):
        conn.add_request(rid)
    q, kv = _Shape(2, S, H, R, D), _Shape(2, S, L, H, D)
    chain = list(range(-1, S - 1))
    cases = {
        "a parent behind its child": dict(parents=[-1] + [5] * (S - 1)),
        "a parent below -1": dict(parents=[-2] + chain[1:]),
        "a tree of another size": dict(parents=chain[:-1]),
        "trees for another batch": dict(parents=[chain]),
        "trees of two sizes": dict(parents=[chain, chain[:-1]]),
        "a float": dict(parents=[-1.0] + chain[1:]),
        "no nodes": dict(parents=[]),
        "n_new > S with a tree": dict(parents=chain, n_new=[S + 1, 0]),
        "beyond max_tokens": dict(parents=chain, n_new=[S, S], req_ids=[1, 2], k_new=kv),
    }
    conn.requests[2].length = T - 2
    for what, change in cases.items():
        args = dict(layer=0, req_ids=[1, 2], q=q, k_new=kv, v_new=kv, sm_scale=1.0, n_new=[S, 2], parents=chain)
        args.update(change)
        with pytest.raises(ValueError):
            conn.attend_chunk(**args)
            pytest.fail(what)
    # the bounded tree route keeps its refusal of 17 nodes
    with pytest.raises(ValueError):
        SpeckvKVConnector._tree_parents(list(range(-1, 16)), 1)
    with pytest.raises(ValueError):
        SpeckvKVConnector.spec_groups(17, 1)
