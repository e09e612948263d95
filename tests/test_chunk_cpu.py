"""Not -m gpu: chunk attention (speckv_ext_attend_chunk, SpeckvKVConnector.chunk_blocks / attend_chunk).

The declarations, the entry on the device-less engine, the static block rule against a brute-force count and against the index search
the kernel runs on it, and attend_chunk()'s refusals against a library that must not be called."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attend_chunk_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_attend_chunk\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    doc = header[header.index("speckv_ext_attend_chunk:"):]
    assert "QUERY STAYS fp16" in doc and "NOT capturable" in doc
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_attend_chunk", p) for p in patterns), patterns
    assert "speckv_ext_attend_chunk" in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk"]
    assert len(sig) == 20
    assert [sig[k] for k in (0, 2, 4, 5)] == [C.c_uint32] * 4 and [sig[k] for k in (10, 11, 15)] == [C.c_uint64] * 3 and sig[16] is C.c_float
    assert all(sig[k] is C.c_void_p for k in (1, 3, 6, 7, 8, 9, 12, 13, 14, 17, 18, 19))
    assert callable(speckv_ctypes.SpeckvLib.attend_chunk)
    makefile = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "Makefile")).read()
    assert "attend_chunk.hip" in makefile                                  # a translation unit of its own


def test_the_library_exports_attend_chunk_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_chunk")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_attend_chunk_on_the_null_engine_answers_as_write_pairs_does():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call"""
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
        with pytest.raises(SpeckvError) as chunk:
            lib.attend_chunk(u64(a), 0, at, 1, 1, np.asarray([0], np.uint32), np.asarray([1], np.uint32), at, at, 1024, 1024, None, 0, 0, 0,
                             1.0, at, 0, 1)
        assert chunk.value.status == write.value.status == -2              # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


def _kernel_search(firsts, fb):
    """k_attend_chunk's binary search: the last request whose exclusive block prefix is <= fb"""
    lo, hi = 0, len(firsts)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if firsts[mid] <= fb:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("rows_per_pos", [1, 2, 4, 8, 16])
def test_chunk_blocks_against_a_brute_force_count(rows_per_pos):
    """per request the number of distinct blocks its live positions fall into, counted position by position; the exclusive prefix;
    and every flat block index finds, by the kernel's search, the request and the local block that the enumeration gives it"""
    per = 64 // rows_per_pos
    rng = np.random.default_rng(rows_per_pos)
    batches = [[70, 33, 17, 16, 1, 0], [0, 0, 5, 0], [0], [1], [per], [per + 1], [0, per - 1, 0, 0, 3 * per, 0], []]
    batches += [list(rng.integers(0, 300, size=9) * rng.integers(0, 2, size=9)) for _ in range(6)]
    for n_new in batches:
        n_new = [int(n) for n in n_new]
        counts, firsts = SpeckvKVConnector.chunk_blocks(n_new, rows_per_pos)
        brute = [len({(j * rows_per_pos) // 64 for j in range(n)}) for n in n_new]
        assert counts == brute, (n_new, rows_per_pos)
        assert firsts == [sum(brute[:i]) for i in range(len(brute))]
        flat = [(b, blk) for b, c in enumerate(brute) for blk in range(c)]
        for fb, (b, blk) in enumerate(flat):
            found = _kernel_search(firsts, fb)
            assert (found, fb - firsts[found]) == (b, blk), (n_new, rows_per_pos, fb)
            assert blk * per < n_new[b]                                    # a block the kernel starts has a live position


def test_chunk_blocks_refuses_bad_input():
    for bad in (0, 3, 5, 32, -1, True, 4.0, None):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_blocks([1], bad)
    for bad in ([-1], [1, -3], [1.5], [True], [None]):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_blocks(bad, 4)
    assert SpeckvKVConnector.chunk_blocks([], 4) == ([], [])


class _Shape:
    """stands in for a tensor in front of the shape checks: anything beyond .shape is a use the checks should have prevented"""

    def __init__(self, *shape):
        self.shape = shape


class _SilentLib:
    """a library that may create requests and must not be asked for anything else"""

    def __init__(self):
        self.handles = 0

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} in front of a ValueError")


def test_attend_chunk_raises_before_any_library_call():
    L, H, D, T, S, R = 2, 8, 128, 64, 5, 4
    conn = SpeckvKVConnector(_SilentLib(), L, H, D, T, "fp8")
    for rid in (1, 2):
        conn.add_request(rid)
    conn.requests[2].length = T - 2
    q, kv = _Shape(2, S, H, R, D), _Shape(2, S, L, H, D)
    cases = {
        "q without rows_per_pos": dict(q=_Shape(2, S, H, D)),
        "k_new without layers": dict(k_new=_Shape(2, S, H, D)),
        "v_new of another S": dict(v_new=_Shape(2, S + 1, L, H, D)),
        "heads": dict(q=_Shape(2, S, 4, R, D)),
        "dim": dict(q=_Shape(2, S, H, R, 64)),
        "batch": dict(req_ids=[1]),
        "no positions": dict(q=_Shape(2, 0, H, R, D), k_new=_Shape(2, 0, L, H, D), v_new=_Shape(2, 0, L, H, D)),
        "rows_per_pos": dict(q=_Shape(2, S, H, 3, D)),
        "layer": dict(layer=L),
        "n_new > S": dict(n_new=[S + 1, 0]),
        "n_new < 0": dict(n_new=[-1, 0]),
        "n_new of another batch": dict(n_new=[1]),
        "beyond max_tokens": dict(n_new=[0, 3]),
    }
    for what, change in cases.items():
        args = dict(layer=0, req_ids=[1, 2], q=q, k_new=kv, v_new=kv, sm_scale=1.0, n_new=[S, 2])
        args.update(change)
        with pytest.raises(ValueError):
            conn.attend_chunk(**args)
            pytest.fail(what)
    other = SpeckvKVConnector(_SilentLib(), L, H, D, T, "int8")
    other.add_request(1)
    with pytest.raises(ValueError, match="FP8, INT4 or MXFP4"):
        other.attend_chunk(0, [1], _Shape(1, S, H, R, D), _Shape(1, S, L, H, D), _Shape(1, S, L, H, D), 1.0)
