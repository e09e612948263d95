"""Not -m gpu: paged-cache transfers (speckv_ext_read_slots / speckv_ext_write_slots, SpeckvKVConnector.paged_spans / load_paged /
store_paged).

The declarations, both entries on the device-less engine, the span rule against a brute-force enumeration, a numpy restatement of
the kernels' index rule against "every position of every span", and the connector's choice between the one-launch route and the
row route against a recording library."""
import contextlib
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
ENTRIES = ("speckv_ext_read_slots", "speckv_ext_write_slots")


def test_the_slot_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # additive entries: the version stays
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    c_api = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    for name in ENTRIES:
        assert re.search(r"speckv_status_t\s+%s\s*\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in c_api
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_slots"]
    assert sig == speckv_ctypes._EXT_SIGNATURES["speckv_ext_write_slots"]                # the same arguments
    assert len(sig) == 13
    assert sig[4] is C.c_uint32 and sig[6] is C.c_uint64 and sig[8] is C.c_uint32 and sig[9] is C.c_uint32 and sig[10] is C.c_uint64 \
        and sig[11] is C.c_uint64
    assert callable(speckv_ctypes.SpeckvLib.read_slots) and callable(speckv_ctypes.SpeckvLib.write_slots)
    assert speckv_ctypes.EXT_ABI_VERSION == 6


def test_the_library_exports_the_slot_entries_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_slot_entries_on_the_null_engine_have_no_data_path():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(2 * 4 * 2048 + 16, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        slots = np.asarray([0, 1, 2, 3], dtype=np.int64)
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        for call in (lib.read_slots, lib.write_slots):
            with pytest.raises(SpeckvError) as e:
                call(u64(h), u64(0), u64(4), u64(0), slots.ctypes.data, 4, u64(at), 0, 4 * 2048, 16, 1)
            assert e.value.status == -2                                    # SPECKV_ERR_DRIVER
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ the span rule
def _brute_pairs(first, count):
    """the position pairs that hold a position of [first, first + count)"""
    return sorted({p // 2 for p in range(first, first + count)})


def test_paged_spans_against_brute_force():
    cases = [(f, c) for f in range(0, 9) for c in range(0, 8)]
    for f, c in cases:
        pairs = _brute_pairs(f, c)
        (first_pair, n, prefix), = SpeckvKVConnector.paged_spans([f], [c])
        assert prefix == 0 and n == len(pairs), (f, c)
        if pairs:
            assert first_pair == pairs[0] and pairs == list(range(first_pair, first_pair + n)), (f, c)
    spans = SpeckvKVConnector.paged_spans([f for f, _ in cases], [c for _, c in cases])
    at = 0
    for (f, c), (first_pair, n, prefix) in zip(cases, spans):
        assert prefix == at and n == len(_brute_pairs(f, c)), (f, c)
        at += n
    assert SpeckvKVConnector.paged_spans([], []) == []
    assert SpeckvKVConnector.paged_spans([5, 7, 2], [0, 1, 2]) == [(2, 0, 0), (3, 1, 0), (1, 1, 1)]
    for bad in (([1], [1, 2]), ([-1], [2]), ([0], [-2])):
        with pytest.raises(ValueError):
            SpeckvKVConnector.paged_spans(*bad)


def _kernel_index_rule(firsts, counts, n_layers, kind_fast):
    """numpy restatement of slot_work (row_transfer.hip): for every flat wave index, (span, pair, l, kind, t_even wanted, t_odd wanted) --
    the span by searching the exclusive prefix as the kernel does"""
    spans = SpeckvKVConnector.paged_spans(firsts, counts)
    prefix = np.asarray([s[2] for s in spans], dtype=np.int64)
    n_pairs = int(sum(s[1] for s in spans))
    per = 2 * n_layers
    out = []
    for i in range(n_pairs * per):
        if kind_fast:
            pp, j = divmod(i, per)
        else:
            j, pp = divmod(i, n_pairs)
        lo, hi = 0, len(spans)                                            # the last span whose prefix is <= pp
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if prefix[mid] <= pp:
                lo = mid
            else:
                hi = mid
        pair = firsts[lo] // 2 + (pp - int(prefix[lo]))
        t0 = 2 * pair - firsts[lo]
        wanted = [0 <= t0 + h < counts[lo] for h in (0, 1)]
        out.append((lo, pair, j >> 1, j & 1, t0, wanted))
    return out


@pytest.mark.parametrize("kind_fast", [False, True])
def test_the_kernel_index_rule_covers_every_position_exactly_once(kind_fast):
    firsts = [0, 5, 33, 64, 7, 2, 9, 0]
    counts = [34, 27, 1, 0, 0, 2, 1, 1]
    n_layers = 3
    seen = {}
    for span, pair, layer, kind, t0, wanted in _kernel_index_rule(firsts, counts, n_layers, kind_fast):
        assert counts[span] > 0, "a wave landed in an empty span"
        assert any(wanted), "a wave with no row to move"
        for h in (0, 1):
            if wanted[h]:
                pos = firsts[span] + t0 + h
                assert pos == 2 * pair + h
                key = (span, pos, layer, kind)
                assert key not in seen, key
                seen[key] = t0 + h                                       # the row of the span's slot mapping
    want = {(s, p, layer, kind): p - firsts[s] for s in range(len(firsts)) for p in range(firsts[s], firsts[s] + counts[s])
            for layer in range(n_layers) for kind in (0, 1)}
    assert seen == want


# ------------------------------------------------------------------------------------------------ the connector's choice of route
class _RecordingLib:
    def __init__(self):
        self.handles, self.calls = 0, []

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def read_slots(self, *a): self.calls.append(("read_slots",) + a)
    def write_slots(self, *a): self.calls.append(("write_slots",) + a)
    def fetch_range(self, *a): self.calls.append(("fetch_range",) + a)
    def write_runs(self, *a): self.calls.append(("write_runs",) + a)


class _Stream:
    cuda_stream = 7

    def wait_stream(self, other): pass


def _cpu_torch(monkeypatch):
    import torch
    from cxl_speckv_amd import kv_connector
    st = _Stream()
    empty = torch.empty
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: empty(*a, **k))
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    return torch, st


def test_load_and_store_take_one_call_or_fall_back(monkeypatch):
    """a [2, blocks, 16, 8, 128] fp16 cache per layer: ONE read_slots / write_slots call with the spans, the region step, the cache
    bases and the plane stride; each fall-back condition -- a K pre-scale, a cache that is not fp16, not contiguous in its last three
    dimensions, without 2048-byte rows -- issues none and goes the row route (fetch_range / write_runs per request)"""
    torch, st = _cpu_torch(monkeypatch)
    L, H, D, T, BS, NB = 2, 8, 128, 64, 16, 6

    def fresh():
        conn = SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8")
        for rid, n in ((1, 34), (2, 32)):
            conn.add_request(rid)
            conn.requests[rid].length = n
        return conn

    good = [torch.zeros((2, NB, BS, H, D), dtype=torch.float16) for _ in range(L)]
    guarded = [torch.zeros((2, NB + 2, BS, H, D), dtype=torch.float16)[:, 1:-1] for _ in range(L)]      # a view with guard blocks
    slots = torch.arange(0, 34 + 31, dtype=torch.int64)
    for caches in (good, guarded):
        conn = fresh()
        conn.load_paged([1, 2], [0, 1], [34, 31], slots, caches, stream=st)
        (name, handles, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream), = conn.lib.calls
        assert name == "read_slots" and list(handles) == [1, 2] and list(firsts) == [0, 1] and list(counts) == [34, 31] and list(begins) == [0, 34]
        assert d_slots == slots.data_ptr() and n_slots == NB * BS and list(bases) == [c.data_ptr() for c in caches]
        assert layer_begin == 0 and kind_stride == caches[0].stride(0) * 2 and step == T // 2 and stream == st.cuda_stream
    # a span that reaches the odd last position: the stored part by the launch, the last row from the tail
    conn = fresh()
    conn.requests[1].length = 35
    tail = (torch.full((L, H, D), 3.0, dtype=torch.float16), torch.full((L, H, D), -3.0, dtype=torch.float16))
    conn.requests[1].set_tail(*tail)
    conn.load_paged([1], [30], [5], torch.tensor([9, 8, 7, 6, 50], dtype=torch.int64), good, stream=st)
    (call,) = conn.lib.calls
    assert call[0] == "read_slots" and list(call[3]) == [4]
    for layer in range(L):
        assert torch.equal(good[layer][0].reshape(-1, H, D)[50], tail[0][layer]) and torch.equal(good[layer][1].reshape(-1, H, D)[50], tail[1][layer])
        good[layer].zero_()
    # store: whole pairs by the launch at the request's length, the odd last position kept as the tail
    conn = fresh()
    epoch = conn._epoch
    held = conn.store_paged([1, 2], [5, 0], torch.tensor([0, 1, 2, 3, 4], dtype=torch.int64), good, stream=st)
    (call,) = conn.lib.calls
    assert held == [] and call[0] == "write_slots" and list(call[2]) == [34, 32] and list(call[3]) == [4, 0] and list(call[4]) == [0, 5]
    assert conn.length(1) == 39 and conn.length(2) == 32 and conn._epoch != epoch and tuple(conn.requests[1].tail_k.shape) == (L, H, D)
    conn.requests[2].length = 33
    with pytest.raises(ValueError):
        conn.store_paged([2], [2], torch.tensor([0, 1], dtype=torch.int64), good, stream=st)
    # the fall-back conditions
    bad = {
        "not fp16": [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16) for _ in range(L)],
        "not contiguous in the last three": [torch.zeros((2, NB, BS, H, 2 * D), dtype=torch.float16)[..., :D] for _ in range(L)],
        "no 2048-byte rows": [torch.zeros((2, NB, BS, 4, D), dtype=torch.float16) for _ in range(L)],
    }
    for what, caches in bad.items():
        assert fresh()._paged_geometry(caches) is None, what
    assert fresh()._paged_geometry(good) == (NB * BS, good[0].stride(0) * 2)
    for what, caches in (("not fp16", bad["not fp16"]), ("not contiguous in the last three", bad["not contiguous in the last three"]),
                         ("a K pre-scale", good)):
        conn = fresh()
        if what == "a K pre-scale":
            conn._kscale = torch.ones((L, H, D), dtype=torch.float16)
            conn._kscale_inv = torch.ones((L, H, D), dtype=torch.float16)
        conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), caches, stream=st)
        names = [c[0] for c in conn.lib.calls]
        assert names == ["fetch_range"] * (2 * L), (what, names)
        conn = fresh()
        if what == "a K pre-scale":
            conn._kscale = torch.ones((L, H, D), dtype=torch.float16)
            conn._kscale_inv = torch.ones((L, H, D), dtype=torch.float16)
        conn.requests[2].length = 0
        conn.store_paged([2], [32], torch.arange(32, dtype=torch.int64), caches, stream=st)
        names = [c[0] for c in conn.lib.calls]
        assert names == ["write_runs"], (what, names)
        assert conn.length(2) == 32
