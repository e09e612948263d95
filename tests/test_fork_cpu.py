"""Not -m gpu: forking requests (speckv_ext_copy_runs, SpeckvKVConnector.fork_plan / fork).

The declarations, the entry on the device-less engine, the static planner over every small case against the rule written out here,
and fork()'s calls and bookkeeping against a recording library."""
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


def test_copy_runs_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_copy_runs\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_copy_runs", p) for p in patterns), patterns
    assert "speckv_ext_copy_runs" in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_copy_runs"]           # src, dst, n_pages, n_pairs, run_firsts, n_runs, stream
    assert len(sig) == 7 and sig[3] is C.c_uint32 and sig[5] is C.c_uint32
    assert all(sig[k] is C.c_void_p for k in (0, 1, 2, 4, 6))
    assert callable(speckv_ctypes.SpeckvLib.copy_runs)
    # the statistics struct grew at its END, and the binding grew with it
    fields = re.search(r"typedef struct \{([^}]*)\} speckv_ext_stats_t;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names[-1] == "copied_pages" and speckv_ctypes.Stats._fields_[-1] == ("copied_pages", C.c_uint64)
    assert [n for n, _ in speckv_ctypes.Stats._fields_] == names


def test_the_library_exports_copy_runs_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_copy_runs")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_copy_runs_on_the_null_engine_answers_as_write_pairs_does():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call; the statistics struct of the
    library and of the binding have one size, and nothing was counted"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a, b = lib.alloc(64 * 4096), lib.alloc(64 * 4096)
        buf = np.zeros(8192, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        with pytest.raises(SpeckvError) as write:
            lib.write_pairs(u64(a), u64(0), u64([at, at + 2048, at + 4096, at + 6144]), 4, 1, 2048, 1)
        with pytest.raises(SpeckvError) as copy:
            lib.copy_runs(u64(a), u64(b), u64(4), u64(0, 32), 1)
        assert copy.value.status == write.value.status == -2              # SPECKV_ERR_DRIVER
        assert lib.stats().copied_pages == 0
    finally:
        lib.finalize()


def test_fork_plan_over_every_small_case():
    """every (source length, length) with 0 <= length <= source length <= 6, one at a time and all as one batch, against the rule:
    length // 2 stored pairs are copied; an odd length needs a tail -- the source's own held row when the lengths are equal,
    otherwise the even half of stored page (length - 1) // 2"""
    cases = [(ln, new) for ln in range(7) for new in range(ln + 1)]
    rule = lambda ln, new: None if new % 2 == 0 else ("held" if new == ln else "read")
    for ln, new in cases:
        assert SpeckvKVConnector.fork_plan([ln], [new]) == ([new // 2], [rule(ln, new)]), (ln, new)
    n_pages, tails = SpeckvKVConnector.fork_plan([c[0] for c in cases], [c[1] for c in cases])
    assert n_pages == [new // 2 for _, new in cases] and tails == [rule(ln, new) for ln, new in cases]
    # the named ones: even and odd, full and shorter, 0 and 1
    assert SpeckvKVConnector.fork_plan([32, 33, 33, 33, 32, 5, 1, 1], [32, 33, 32, 17, 17, 0, 1, 0]) == \
        ([16, 16, 16, 8, 8, 0, 0, 0], [None, "held", None, "read", "read", None, "held", None])
    for ln in range(7):
        with pytest.raises(ValueError):
            SpeckvKVConnector.fork_plan([4, ln], [4, ln + 1])
        with pytest.raises(ValueError):
            SpeckvKVConnector.fork_plan([ln], [-1])
    assert SpeckvKVConnector.fork_plan([], []) == ([], [])


class _RecordingLib:
    """what fork() asks of the library: every copy_runs and read_pairs call with its arguments; the rows read_pairs is asked for are
    filled with a pattern that names (handle, page, layer, kind), host tensors standing in for device buffers"""

    def __init__(self, fail=None):
        self.handles, self.copies, self.reads, self.freed, self.fail = 0, [], [], [], fail

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def free(self, handle):
        self.freed.append(handle)

    @staticmethod
    def pattern(handle, page, layer, kind):
        return np.full(1024, 1000 * handle + 100 * page + 10 * layer + kind, dtype=np.int16)

    def copy_runs(self, src, dst, n_pages, run_firsts, stream):
        if self.fail == "copy_runs":
            raise speckv_ctypes.SpeckvError("speckv_ext_copy_runs", -1)
        self.copies.append(([int(h) for h in src], [int(h) for h in dst], [int(n) for n in n_pages], [int(f) for f in run_firsts], stream))

    def read_pairs(self, handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        if self.fail == "read_pairs":
            raise speckv_ctypes.SpeckvError("speckv_ext_read_pairs", -1)
        rows = np.asarray(rows, dtype=np.uint64).reshape(len(handles), 4)
        self.reads.append(([int(h) for h in handles], [int(f) for f in first_pages], rows.copy(), int(page_step), int(n_layers), int(layer_stride), stream))
        for h, f, r in zip(handles, first_pages, rows):
            for layer in range(int(n_layers)):
                for k in range(4):
                    if r[k]:
                        row = self.pattern(int(h), int(f), layer, k // 2)
                        C.memmove(int(r[k]) + layer * int(layer_stride), row.ctypes.data, 2048)


class _Stream:
    cuda_stream = 7

    def wait_stream(self, other): pass


L, H, D, T = 3, 8, 128, 64


def _connector(monkeypatch, fail=None):
    """a connector over the recording library with sources of lengths 33, 33, 32, 6, 0, 1 (ids 21..26), the odd ones holding a tail"""
    import torch
    from cxl_speckv_amd import kv_connector
    st = _Stream()
    empty = torch.empty
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: empty(*a, **k))
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    conn = SpeckvKVConnector(_RecordingLib(fail), L, H, D, T, "fp8")
    held = {}
    for rid, n in zip([21, 22, 23, 24, 25, 26], [33, 33, 32, 6, 0, 1]):
        conn.add_request(rid)
        r = conn.requests[rid]
        r.length = n
        if n & 1:
            held[rid] = (torch.full((L, H, D), float(rid), dtype=torch.float16), torch.full((L, H, D), -float(rid), dtype=torch.float16))
            r.set_tail(*held[rid])
    return conn, st, held


def _state(conn):
    return ({rid: (r.handle, r.length, r._tail) for rid, r in conn.requests.items()}, conn._epoch, conn._arg_key, conn._fold_key, conn._tail_ids)


def test_fork_asks_for_one_copy_and_one_read_and_keeps_the_books(monkeypatch):
    """fork() against a recording library: ONE copy_runs call with the source and new handles, fork_plan's page counts and the first
    page of every (layer, kind) region; ONE read_pairs call on the SOURCE handles for the "read" tails, odd slots NULL, rows of one
    tensor pair; "held" tails are clones of the source's rows that share no storage with them; lengths, tails and _epoch as for
    requests written independently."""
    import torch
    conn, st, held = _connector(monkeypatch)
    src = [21, 21, 22, 23, 24, 24, 26, 25]                                # a source may appear several times
    new = [31, 32, 33, 34, 35, 36, 37, 38]
    lengths = [33, 17, 32, 31, 6, 5, 1, 0]                                # held, read, -, read, -, read, held, -
    epoch = conn._epoch
    keep = conn.fork(src, new, lengths, stream=st)
    h = lambda rid: conn.requests[rid].handle
    assert len(conn.lib.copies) == 1 and len(conn.lib.reads) == 1
    s, d, n_pages, firsts, stream = conn.lib.copies[0]
    assert s == [h(r) for r in src] and d == [h(r) for r in new] and n_pages == [16, 8, 16, 15, 3, 2, 0, 0]
    assert firsts == [j * (T // 2) for j in range(2 * L)] and stream == st.cuda_stream
    handles, pages, rows, step, layers, stride, stream = conn.lib.reads[0]
    assert handles == [h(21), h(23), h(24)] and pages == [8, 15, 2]       # the SOURCES, page (length - 1) // 2
    assert step == T // 2 and layers == L and stride == H * D * 2 and stream == st.cuda_stream
    assert (rows[:, 1] == 0).all() and (rows[:, 3] == 0).all() and rows[:, 0].all() and rows[:, 2].all()
    assert (np.diff(rows[:, 0].astype(np.int64)) == L * H * D * 2).all() and (np.diff(rows[:, 2].astype(np.int64)) == L * H * D * 2).all()
    assert [conn.length(r) for r in new] == lengths and conn._epoch != epoch
    assert [conn.length(r) for r in (21, 22, 23, 24, 25, 26)] == [33, 33, 32, 6, 0, 1]
    assert len(keep) == 2
    for i, (rid, source, page) in enumerate(((32, 21, 8), (34, 23, 15), (36, 24, 2))):
        r = conn.requests[rid]
        for kind, tail, whole in ((0, r.tail_k, keep[0]), (1, r.tail_v, keep[1])):
            assert torch.equal(tail.view(torch.int16), whole[i].view(torch.int16))
            for layer in range(L):
                assert np.array_equal(tail[layer].numpy().view(np.int16).reshape(-1), _RecordingLib.pattern(h(source), page, layer, kind)), (rid, layer, kind)
    for rid, source in ((31, 21), (37, 26)):                              # "held": equal values, storage of their own
        r, s_ = conn.requests[rid], conn.requests[source]
        assert torch.equal(r.tail_k, held[source][0]) and torch.equal(r.tail_v, held[source][1])
        assert r.tail_k.data_ptr() != s_.tail_k.data_ptr() and r.tail_v.data_ptr() != s_.tail_v.data_ptr()
        s_.tail_k.fill_(7.0)                                              # the source moves on: the fork does not
        assert bool((r.tail_k == float(source)).all())
    for rid in (33, 35, 38):
        assert conn.requests[rid].tail_k is None
    assert torch.equal(conn.requests[22].tail_k, held[22][0])             # a source is untouched


def test_fork_without_stored_pairs_makes_no_call(monkeypatch):
    conn, st, held = _connector(monkeypatch)
    conn.fork([26, 25, 21], [41, 42, 43], [1, 0, 0], stream=st)          # a held row, nothing, nothing
    assert conn.lib.copies == [] and conn.lib.reads == []
    assert [conn.length(r) for r in (41, 42, 43)] == [1, 0, 0] and conn.requests[41].tail_k is not None
    conn.fork([21], [44], stream=st)                                      # lengths default to the sources'
    assert len(conn.lib.copies) == 1 and conn.lib.reads == [] and conn.length(44) == 33
    assert conn.fork([], [], stream=st) == []


def test_fork_refusals_change_no_state(monkeypatch):
    conn, st, held = _connector(monkeypatch)
    before, handles = _state(conn), conn.lib.handles
    with pytest.raises(KeyError):
        conn.fork([21, 22], [51, 23], stream=st)                          # an existing id
    with pytest.raises(KeyError):
        conn.fork([21, 22], [51, 51], stream=st)                          # the same new id twice
    with pytest.raises(KeyError):
        conn.fork([99], [51], stream=st)                                  # an unknown source
    with pytest.raises(ValueError):
        conn.fork([21, 24], [51, 52], [33, 7], stream=st)                 # longer than the source
    with pytest.raises(ValueError):
        conn.fork([21], [51], [-1], stream=st)
    assert _state(conn) == before and conn.lib.handles == handles and conn.lib.copies == [] and conn.lib.reads == []


@pytest.mark.parametrize("fail", ["copy_runs", "read_pairs"])
def test_a_failed_launch_frees_what_fork_allocated(monkeypatch, fail):
    conn, st, held = _connector(monkeypatch, fail)
    before = _state(conn)
    with pytest.raises(speckv_ctypes.SpeckvError):
        conn.fork([21, 21], [61, 62], [33, 17], stream=st)
    assert 61 not in conn.requests and 62 not in conn.requests
    assert sorted(conn.lib.freed) == [7, 8]                               # the two allocations fork made, and no other
    assert _state(conn)[0] == before[0]                                   # the sources are untouched
