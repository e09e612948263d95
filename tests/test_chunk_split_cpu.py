"""Not -m gpu: the split chunk attention (speckv_ext_attend_chunk_split, speckv_ext_chunk_split_plan, SpeckvKVConnector.chunk_pieces /
attend_chunk(splits=...)).

The declarations, the entry on the device-less engine, the piece rule of the library against the connector's restatement and against a
brute-force restatement written here, the index search the kernel runs on the item prefixes, and the connector's refusals against a
library that must not be called."""
import ctypes as C
import fnmatch
import itertools
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests.test_chunk_cpu import _Shape, _SilentLib, _kernel_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_END = [0, 2, 32, 34, 1024, 1026, 4000, 32768]
N_Q = [0, 1, 8, 9, 70, 512]
RPPS = [1, 2, 4, 8, 16]
SPLITS = [0, 1, 2, 3, 5, 64]
FLOOR = 32                                        # kChunkPieceFloorTiles


def test_the_split_entry_and_the_plan_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_attend_chunk_split\s*\(", header)
    assert re.search(r"speckv_status_t\s+speckv_ext_chunk_split_plan\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # additive entries: the version stays
    assert "#define SPECKV_CHUNK_SPLITS_MAX 64u" in header
    doc = header[header.index("speckv_ext_attend_chunk_split:"):]
    assert "DEPEND ON THE PIECE COUNT" in doc and "WHOLE CALL" in doc and "sequence alone" in doc
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    for name in ("speckv_ext_attend_chunk_split", "speckv_ext_chunk_split_plan"):
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), patterns
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_split"]
    assert len(sig) == 23
    masked = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_masked"]
    assert sig[:18] == masked[:18] and sig[18] is C.c_uint32 and sig[19:] == masked[18:]         # n_splits in front of sm_scale
    plan = speckv_ctypes._EXT_SIGNATURES["speckv_ext_chunk_split_plan"]
    assert len(plan) == 8 and [plan[k] for k in (0, 3, 4, 5)] == [C.c_uint32] * 4 and all(plan[k] is C.c_void_p for k in (1, 2, 6, 7))
    assert callable(speckv_ctypes.SpeckvLib.attend_chunk_split) and callable(speckv_ctypes.SpeckvLib.chunk_split_plan)
    assert speckv_ctypes.CHUNK_SPLITS_MAX == 64


def test_the_library_exports_both_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_chunk_split") and hasattr(lib, "speckv_ext_chunk_split_plan")
    assert hasattr(lib, "speckv_ext_attend_chunk") and hasattr(lib, "speckv_ext_attend_chunk_masked")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_split_entry_on_the_null_engine_answers_as_write_pairs_does():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call; nothing is counted"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        before = bytes(lib.stats())
        with pytest.raises(SpeckvError) as write:
            lib.write_pairs(u64(a), u64(0), u64([at, at + 2048, at + 4096, at + 6144]), 4, 1, 2048, 1)
        for n_splits, mask in ((0, 0), (1, 0), (5, 0), (5, at)):
            with pytest.raises(SpeckvError) as chunk:
                lib.attend_chunk_split(u64(a), 0, at, 1, 1, np.asarray([0], np.uint32), np.asarray([1], np.uint32), at, at, 1024, 1024, None, 0,
                                       0, 0, mask, 1, n_splits, 1.0, at, 0, 1)
            assert chunk.value.status == write.value.status == -2              # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- the piece rule
def _ceil(a, b):
    return -(-a // b)


def _brute(pos_end, n_q, rpp, n_splits, n_cus):
    """the rule restated from the interface's text, sequence by sequence"""
    n_pool = [_ceil(p, 32) for p in pos_end]
    if n_splits == 0:
        g0 = 8 * sum(len({(j * rpp) // 64 for j in range(n)}) for n in n_q)
        target = 3 * n_cus
        if g0 == 0 or g0 >= target:
            first = [1] * len(pos_end)
        else:
            want = target // g0                                  # the pieces of a call fit one round of resident workgroups
            first = [min(max(t // FLOOR, 1), min(want, 64)) for t in n_pool]
    elif n_splits == 1:
        first = [1] * len(pos_end)
    else:
        first = [min(n_splits, max(1, t)) for t in n_pool]
    pieces, tpps = [], []
    for t, p in zip(n_pool, first):
        tpp = _ceil(t, p)
        pieces.append(_ceil(t, tpp) if tpp else 1)
        tpps.append(tpp)
    return pieces, tpps


def _plan(lib, pos_end, n_q, rpp, n_splits, n_cus):
    n = len(pos_end)
    pe, nq = (C.c_uint32 * n)(*pos_end), (C.c_uint32 * n)(*n_q)
    pieces, tpp = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    rc = lib.speckv_ext_chunk_split_plan(n, pe, nq, rpp, n_splits, n_cus, pieces, tpp)
    return rc, list(pieces), list(tpp)


def _invariants(pos_end, pieces, tpps, what):
    for p_end, p, tpp in zip(pos_end, pieces, tpps):
        n_pool = _ceil(p_end, 32)
        assert 1 <= p <= max(1, n_pool), what
        ranges = [(k * tpp, min((k + 1) * tpp, n_pool)) for k in range(p)]
        if n_pool == 0:
            assert (p, tpp) == (1, 0), what
            continue
        assert all(b > a for a, b in ranges), (what, "an empty piece")
        assert ranges[0][0] == 0 and ranges[-1][1] == n_pool and all(ranges[k][1] == ranges[k + 1][0] for k in range(p - 1)), what


@pytest.fixture(scope="module")
def clib():
    lib = C.CDLL(pkg.build_library())
    lib.speckv_ext_chunk_split_plan.restype = C.c_int
    lib.speckv_ext_chunk_split_plan.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("n_cus", [1, 256])
@pytest.mark.parametrize("n_splits", SPLITS)
def test_the_plan_against_the_connector_and_a_brute_force_restatement(clib, n_splits, n_cus):
    """works without speckv_init.  Single sequences over the whole sweep, and batches: the sweep's pos_end with every n_q rotated
    against them, so that every (pos_end, n_q) pair appears inside a batch too"""
    for rpp in RPPS:
        batches = [([p], [n]) for p, n in itertools.product(POS_END, N_Q)]
        for r in range(len(N_Q)):
            batches.append((POS_END, [N_Q[(i + r) % len(N_Q)] for i in range(len(POS_END))]))
        batches += [([32768], [1]), ([32768, 32768], [1, 1]), ([4000] * 3, [40, 5, 0]), ([], [])]
        for pos_end, n_q in batches:
            what = (pos_end, n_q, rpp, n_splits, n_cus)
            rc, pieces, tpps = _plan(clib, pos_end, n_q, rpp, n_splits, n_cus)
            assert rc == 0, what
            assert (pieces, tpps) == _brute(pos_end, n_q, rpp, n_splits, n_cus), what
            py = SpeckvKVConnector.chunk_pieces(n_q, pos_end, rpp, n_splits, n_cus)
            assert (py[0], py[1]) == (pieces, tpps), what
            counts, _ = SpeckvKVConnector.chunk_blocks(n_q, rpp)
            assert py[2] == [sum(c * p for c, p in zip(counts[:i], pieces[:i])) for i in range(len(counts))], what
            _invariants(pos_end, pieces, tpps, what)
            if n_splits == 1:
                assert pieces == [1] * len(pos_end), what
            if n_splits == 0 and 8 * sum(counts) >= 3 * n_cus:
                assert pieces == [1] * len(pos_end), what


def test_the_rule_splits_a_short_step_over_a_long_context(clib):
    """the issue's example: a 40-node tree at rows_per_pos 8 over 32k stored positions = 5 blocks x 8 heads = 40 workgroups on 256 CUs"""
    rc, pieces, tpps = _plan(clib, [32768], [40], 8, 0, 256)
    assert rc == 0 and pieces == [19] and tpps == [54]                   # want = 768 // 40 = 19 <= 1024 // 32; ceil(1024 / 19) = 54
    rc, pieces, tpps = _plan(clib, [32768], [40], 8, 0, 0)               # n_cus 0 without an engine: 256
    assert rc == 0 and pieces == [19]
    assert SpeckvKVConnector.chunk_pieces([40], [32769], 8)[0] == [19]   # a length of 32769: the odd last position is held
    assert _plan(clib, [32768], [512], 8, 0, 256)[1] == [1]              # 64 blocks x 8 = 512 > 768 / 2: two pieces would not fit a round


@pytest.mark.parametrize("n_splits", [2, 3, 5, 64])
def test_a_forced_count_depends_on_the_sequence_alone(clib, n_splits):
    """the batch permuted, and with members dropped: every remaining member keeps its pieces"""
    rng = np.random.default_rng(n_splits)
    n_q = [N_Q[i % len(N_Q)] for i in range(len(POS_END))]
    for rpp in (1, 8):
        _, pieces, tpps = _plan(clib, POS_END, n_q, rpp, n_splits, 256)
        alone = {p: _plan(clib, [p], [1], rpp, n_splits, 1)[1:] for p in POS_END}
        for p_end, p, tpp in zip(POS_END, pieces, tpps):
            assert alone[p_end] == ([p], [tpp])
        for _ in range(4):
            order = rng.permutation(len(POS_END))
            keep = order[:int(rng.integers(1, len(POS_END) + 1))]
            _, p2, t2 = _plan(clib, [POS_END[i] for i in keep], [n_q[i] for i in keep], rpp, n_splits, 256)
            assert p2 == [pieces[i] for i in keep] and t2 == [tpps[i] for i in keep]


def test_the_plan_refuses_65_pieces_and_bad_rows_per_pos(clib):
    out = (C.c_uint32 * 1)(7)
    one = (C.c_uint32 * 1)(64)
    for rpp, n_splits in ((4, 65), (4, 0xFFFFFFFF), (0, 1), (3, 1), (32, 0)):
        assert clib.speckv_ext_chunk_split_plan(1, one, one, rpp, n_splits, 256, out, out) == -4       # SPECKV_ERR_INVAL
        assert out[0] == 7
    assert clib.speckv_ext_chunk_split_plan(1, None, one, 4, 1, 256, out, out) == -4
    assert clib.speckv_ext_chunk_split_plan(1, one, one, 4, 1, 256, None, out) == -4
    for bad in (65, -1, True, 2.5, None):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_pieces([1], [64], 4, bad)


@pytest.mark.parametrize("n_splits", [0, 2, 3, 5, 64])
@pytest.mark.parametrize("rpp", [1, 8, 16])
def test_the_kernels_search_over_the_item_prefixes(n_splits, rpp):
    """every flat work item finds, by k_attend_chunk's binary search over first_item, the (sequence, block, piece) the enumeration gives
    it -- batches with sequences of zero live positions first, last and twice in a row"""
    batches = [([4000, 32768, 34, 0, 1026, 2], [0, 70, 0, 0, 9, 1]), ([32768, 0, 4000, 1024], [1, 8, 70, 0]),
               ([0, 0, 32768], [0, 0, 9]), ([4000], [0]), ([32768, 32768, 32768], [0, 0, 0]), ([1024, 4000, 34, 32768], [0, 0, 512, 0])]
    for pos_end, n_q in batches:
        pieces, _, firsts = SpeckvKVConnector.chunk_pieces(n_q, pos_end, rpp, n_splits, 256)
        counts, _ = SpeckvKVConnector.chunk_blocks(n_q, rpp)
        flat = [(b, blk, p) for b, c in enumerate(counts) for blk in range(c) for p in range(pieces[b])]
        if n_splits == 64 and sum(counts):
            assert len(flat) > sum(counts)
        for item, (b, blk, p) in enumerate(flat):
            found = _kernel_search(firsts, item)
            rest = item - firsts[found]
            assert (found, rest // pieces[found], rest % pieces[found]) == (b, blk, p), (pos_end, n_q, rpp, n_splits, item)
            assert blk * (64 // rpp) < n_q[b]


# ----------------------------------------------------------------------------- the connector's refusals
@pytest.mark.parametrize("bad", [-1, True, 2.5, 65, None, "0"])
def test_attend_chunk_refuses_a_bad_splits_before_any_library_call(bad):
    L, H, D, T, S, R = 2, 8, 128, 64, 5, 4
    conn = SpeckvKVConnector(_SilentLib(), L, H, D, T, "fp8")
    conn.add_request(1)
    q, kv = _Shape(1, S, H, R, D), _Shape(1, S, L, H, D)
    with pytest.raises(ValueError, match="splits"):
        conn.attend_chunk(0, [1], q, kv, kv, 1.0, splits=bad)
    with pytest.raises(ValueError, match="splits"):
        conn.attend_chunk(0, [1], q, kv, kv, 1.0, parents=[-1, 0, 0, 1, 1], splits=bad)
