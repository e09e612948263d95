"""Not -m gpu: the rollback of committed positions (speckv_ext_read_pairs, SpeckvKVConnector.truncate_plan / truncate).

The declarations, the entry on the device-less engine, the static planner over every small case against the rule written out here,
and truncate()'s bookkeeping against a recording library."""
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


def test_read_pairs_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_read_pairs\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_read_pairs", p) for p in patterns), patterns
    assert "speckv_ext_read_pairs" in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    # the mirror image of write_pairs, argument for argument
    assert speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_pairs"] == speckv_ctypes._EXT_SIGNATURES["speckv_ext_write_pairs"]
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_pairs"]
    assert len(sig) == 8 and sig[3] is C.c_uint32 and sig[4] is C.c_uint64 and sig[5] is C.c_uint32 and sig[6] is C.c_uint64
    assert callable(speckv_ctypes.SpeckvLib.read_pairs)


def test_the_library_exports_read_pairs_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_read_pairs")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_read_pairs_on_the_null_engine_has_no_data_path():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8192, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        with pytest.raises(SpeckvError) as pairs:
            lib.read_pairs(np.asarray([h], dtype=np.uint64), np.asarray([0], dtype=np.uint64), np.asarray([[at, 0, at + 2048, 0]], dtype=np.uint64),
                           4, 1, 2048, 1)
        assert pairs.value.status == -2                                    # SPECKV_ERR_DRIVER
        assert not buf.any()
    finally:
        lib.finalize()


def test_truncate_plan_over_every_small_case():
    """every (length, new_len) with 0 <= new_len <= length <= 6, one request at a time and all of them as one batch, against the rule:
    a cut to an odd length reads position new_len - 1 back from page (new_len - 1) // 2; a cut of an odd length to an even one drops
    the held position; everything else touches neither pool nor tail"""
    cases = [(ln, new) for ln in range(7) for new in range(ln + 1)]
    for ln, new in cases:
        want_read = [(0, (new - 1) // 2)] if new < ln and new & 1 else []
        want_drop = [0] if new < ln and ln & 1 and not new & 1 else []
        assert SpeckvKVConnector.truncate_plan([ln], [new]) == (want_drop, want_read), (ln, new)
    drops, reads = SpeckvKVConnector.truncate_plan([c[0] for c in cases], [c[1] for c in cases])
    assert drops == [b for b, (ln, new) in enumerate(cases) if new < ln and ln & 1 and not new & 1]
    assert reads == [(b, (new - 1) // 2) for b, (ln, new) in enumerate(cases) if new < ln and new & 1]
    for ln in range(7):
        with pytest.raises(ValueError):
            SpeckvKVConnector.truncate_plan([4, ln], [4, ln + 1])
        with pytest.raises(ValueError):
            SpeckvKVConnector.truncate_plan([ln], [-1])
    assert SpeckvKVConnector.truncate_plan([], []) == ([], [])


class _RecordingLib:
    """what truncate() asks of the library: every read_pairs call with its arguments; the rows asked for are filled with a pattern
    that names (handle, page, layer, kind), host tensors standing in for device buffers"""

    def __init__(self):
        self.handles, self.calls = 0, []

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    @staticmethod
    def pattern(handle, page, layer, kind):
        return np.full(1024, 1000 * handle + 100 * page + 10 * layer + kind, dtype=np.int16)

    def read_pairs(self, handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        rows = np.asarray(rows, dtype=np.uint64).reshape(len(handles), 4)
        self.calls.append(([int(h) for h in handles], [int(f) for f in first_pages], rows.copy(), int(page_step), int(n_layers), int(layer_stride), stream))
        for h, f, r in zip(handles, first_pages, rows):
            for layer in range(int(n_layers)):
                for k in range(4):
                    if r[k]:
                        row = self.pattern(int(h), int(f), layer, k // 2)
                        C.memmove(int(r[k]) + layer * int(layer_stride), row.ctypes.data, 2048)


class _Stream:
    cuda_stream = 7

    def wait_stream(self, other): pass


def test_truncate_asks_for_one_read_and_keeps_the_books(monkeypatch):
    """truncate() against a recording library: one read_pairs call for the batch with the handles and pages of truncate_plan's reads,
    the odd slots NULL, page_step = the pages of a region, all layers, a stride of one row; the rows become the tails, and lengths,
    tails, _tail_ids, _epoch and the dropped plan are those of a connector that stopped there.  No read, no call."""
    import contextlib
    import torch
    from cxl_speckv_amd import kv_connector
    st = _Stream()
    empty = torch.empty
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: empty(*a, **k))
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    L, H, D, T = 3, 8, 128, 64
    conn = SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8")
    ids, lengths = [21, 22, 23, 24, 25, 26], [33, 33, 34, 8, 9, 6]
    held = {}
    for rid, n in zip(ids, lengths):
        conn.add_request(rid)
        r = conn.requests[rid]
        r.length = n
        if n & 1:
            held[rid] = (torch.full((L, H, D), float(rid), dtype=torch.float16), torch.full((L, H, D), -float(rid), dtype=torch.float16))
            r.set_tail(*held[rid])
    conn._tail_ids, conn._tail_k, conn._tail_v = (25,), held[25][0][None], held[25][1][None]
    conn._arg_key, conn._fold_key, conn._plan_stream, epoch = ("a plan",), ("fold rows",), st, conn._epoch
    new = [32, 31, 33, 8, 9, 3]                                        # drop, read, read, nothing, nothing, read
    conn.truncate(ids, new, stream=st)
    assert len(conn.lib.calls) == 1
    handles, firsts, rows, step, layers, stride, stream = conn.lib.calls[0]
    assert handles == [conn.requests[r].handle for r in (22, 23, 26)] and firsts == [15, 16, 1]
    assert step == T // 2 and layers == L and stride == H * D * 2 and stream == st.cuda_stream
    assert (rows[:, 1] == 0).all() and (rows[:, 3] == 0).all() and rows[:, 0].all() and rows[:, 2].all()
    assert (np.diff(rows[:, 0].astype(np.int64)) == L * H * D * 2).all() and (np.diff(rows[:, 2].astype(np.int64)) == L * H * D * 2).all()
    assert [conn.length(r) for r in ids] == new
    assert conn._epoch != epoch and conn._arg_key is None and conn._fold_key is None and conn._plan_stream is None
    assert conn._tail_ids == (22, 23, 26)
    for i, (rid, page) in enumerate(((22, 15), (23, 16), (26, 1))):
        r = conn.requests[rid]
        for kind, tail, whole in ((0, r.tail_k, conn._tail_k), (1, r.tail_v, conn._tail_v)):
            assert torch.equal(tail.view(torch.int16), whole[i].view(torch.int16))                         # installed as rows of one tensor pair, as _committed installs tails
            for layer in range(L):
                want = _RecordingLib.pattern(r.handle, page, layer, kind)
                assert np.array_equal(tail[layer].numpy().view(np.int16).reshape(-1), want), (rid, layer, kind)
    assert conn.requests[21].tail_k is None and conn.requests[24].tail_k is None
    assert torch.equal(conn.requests[25].tail_k, held[25][0]) and torch.equal(conn.requests[25].tail_v, held[25][1])     # untouched
    # cuts that need no row back: no call; a dropped tail that the lockstep tensors named takes them along
    conn._tail_ids, conn._tail_k, conn._tail_v = (25,), held[25][0][None], held[25][1][None]
    conn.truncate(ids, [30, 31, 32, 8, 8, 2], stream=st)
    assert len(conn.lib.calls) == 1
    assert [conn.length(r) for r in ids] == [30, 31, 32, 8, 8, 2]
    assert [conn.requests[r].tail_k is not None for r in ids] == [False, True, False, False, False, False]
    assert conn._tail_ids == () and conn._tail_k is None
    e = conn._epoch
    conn.truncate(ids, [30, 31, 32, 8, 8, 2], stream=st)             # nothing to do: nothing moves
    assert conn._epoch == e and len(conn.lib.calls) == 1
    with pytest.raises(ValueError):
        conn.truncate(ids, [30, 32, 32, 8, 8, 2], stream=st)
    assert [conn.length(r) for r in ids] == [30, 31, 32, 8, 8, 2]
