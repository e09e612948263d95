"""Not -m gpu: the one-launch commit of a multi-position step (speckv_ext_write_pairs, SpeckvKVConnector.commit).

The declarations, and the connector against recording libraries with host tensors standing in for device buffers: commit() must ask
the library for the pages, page images, lengths and tails that append_tokens() / append_path() come to -- with ONE library call."""
import contextlib
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_connector, speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_pairs_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_write_pairs\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_write_pairs", p) for p in patterns), patterns
    assert "speckv_ext_write_pairs" in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_write_pairs"]
    assert len(sig) == 8 and sig[3] is C.c_uint32 and sig[4] is C.c_uint64 and sig[5] is C.c_uint32 and sig[6] is C.c_uint64
    assert callable(speckv_ctypes.SpeckvLib.write_pairs)


def test_write_pairs_on_the_null_engine_has_no_data_path():
    """the fake device has a page table and no data path: write_pairs answers what write_strided_batch answers there"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(4096, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        with pytest.raises(SpeckvError) as batch:
            lib.write_strided_batch([h], np.asarray([0], dtype=np.uint64), np.asarray([at], dtype=np.uint64), 4, 2, 1)
        with pytest.raises(SpeckvError) as pairs:
            lib.write_pairs(np.asarray([h], dtype=np.uint64), np.asarray([0], dtype=np.uint64), np.full((1, 4), at, dtype=np.uint64), 4, 1, 2048, 1)
        assert pairs.value.status == batch.value.status != 0
    finally:
        lib.finalize()


class _RecordingLib:
    """what the connector asks of the library, recorded: every page image a write would store, by (handle, page), and every call"""

    def __init__(self):
        self.handles, self.writes, self.calls = 0, [], []

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def write_strided(self, handle, first, step, n_pages, src, stream, call="write_strided"):
        if call:
            self.calls.append(call)
        for j in range(int(n_pages)):
            self.writes.append((int(handle), int(first) + j * int(step), C.string_at(int(src) + 4096 * j, 4096)))

    def write_strided_batch(self, handles, firsts, srcs, step, n_each, stream):
        self.calls.append("write_strided_batch")
        for h, f, s in zip(handles, firsts, srcs):
            self.write_strided(h, f, step, n_each, int(s), stream, call=None)

    def write_pairs(self, handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        self.calls.append("write_pairs")
        rows = np.asarray(rows, dtype=np.uint64).reshape(len(handles), 4)
        assert layer_stride % 16 == 0 and (rows % 16 == 0).all()
        for h, f, r in zip(handles, first_pages, rows):
            for j in range(2 * int(n_layers)):
                layer, kind = j >> 1, j & 1
                image = b"".join(C.string_at(int(r[2 * kind + half]) + layer * int(layer_stride), 2048) for half in (0, 1))
                self.writes.append((int(h), int(f) + j * int(page_step), image))


class _Stream:
    cuda_stream = 1

    def wait_stream(self, other): pass


L, H, D, T, B, S = 2, 8, 128, 64, 5, 4
IDS = [11, 12, 13, 14, 15]


@pytest.fixture
def host(monkeypatch):
    import torch
    st = _Stream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    return st


def _connectors():
    a, b = SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8"), SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8")
    for conn in (a, b):
        for rid in IDS:
            conn.add_request(rid)
    return a, b


def _same_state(a, b):
    import torch
    for rid in IDS:
        assert a.length(rid) == b.length(rid)
        ra, rb = a.requests[rid], b.requests[rid]
        assert (ra.tail_k is None) == (rb.tail_k is None) == (a.length(rid) % 2 == 0)
        if ra.tail_k is not None:
            assert torch.equal(ra.tail_k, rb.tail_k) and torch.equal(ra.tail_v, rb.tail_v)
    assert a._tail_ids == b._tail_ids and a._epoch == b._epoch
    if a._tail_ids:
        assert torch.equal(a._tail_k, b._tail_k) and torch.equal(a._tail_v, b._tail_v)
    assert sorted(a.lib.writes) == sorted(b.lib.writes)                     # (handle, page, image)


def _step(gen):
    import torch
    return (torch.randn((B, S, L, H, D), generator=gen).to(torch.float16), torch.randn((B, S, L, H, D), generator=gen).to(torch.float16))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("kscale", [False, True])
def test_commit_writes_what_append_tokens_writes(host, seed, kscale):
    """six steps of accept counts that include 0 and S, requests at odd and even lengths: the same (handle, page, image), lengths and
    tails as append_tokens -- from exactly one library call per commit that writes, none when nothing is accepted; with the K
    pre-scale on (host tensors as the scale) the images are still append_tokens'"""
    import torch
    a, b = _connectors()
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    if kscale:
        for conn in (a, b):
            conn._kscale_inv = (torch.rand((L, H, D), generator=torch.Generator().manual_seed(7)) + 0.5).to(torch.float16)
    keep = []
    for step in range(6):
        k, v = _step(gen)
        n_accept = [0, 1, 2, 3, S] if step == 0 else [int(x) for x in rng.integers(0, S + 1, B)]
        n_accept = n_accept[step % B:] + n_accept[:step % B]
        if step == 3:
            n_accept = [0] * B
        if step == 4:
            n_accept = [1 if a.length(rid) % 2 == 0 else 0 for rid in IDS]  # tails only: nothing goes to the pool
        calls, writes = len(a.lib.calls), len(a.lib.writes)
        keep.append(a.commit(IDS, k, v, [list(range(n)) for n in n_accept], stream=host))
        keep.append(b.append_tokens(IDS, k, v, n_accept, stream=host))
        pool = len(a.lib.writes) > writes
        assert a.lib.calls[calls:] == (["write_pairs"] if pool else [])
        if step in (3, 4):
            assert not pool
        _same_state(a, b)
    assert len(a.lib.writes) > 10 * 2 * L and set(a.lib.calls) == {"write_pairs"}


def test_commit_of_a_strided_step_reads_a_contiguous_copy(host):
    """k_new / v_new that are views (a step tensor with the layers in front): commit makes them contiguous and returns the copies"""
    import torch
    a, b = _connectors()
    gen = torch.Generator().manual_seed(3)
    k, v = (x.permute(2, 0, 1, 3, 4).contiguous().permute(1, 2, 0, 3, 4) for x in _step(gen))
    assert not k.is_contiguous()
    keep = a.commit(IDS, k, v, [[0, 1, 2], [0, 1], [0], [], [0, 1, 2, 3]], stream=host)
    b.append_tokens(IDS, k, v, [3, 2, 1, 0, 4], stream=host)
    assert keep[0].is_contiguous() and torch.equal(keep[0], k) and torch.equal(keep[1], v)
    _same_state(a, b)


@pytest.mark.parametrize("per_request", [False, True])
def test_commit_of_tree_paths_writes_what_append_path_writes(host, per_request):
    """a two-leaf tree of 4 nodes (0 <- 1 <- 2, 1 <- 3), and one tree per request: accepted paths through commit(parents=...) against
    append_path, over three steps so that pairs consume tails of earlier steps"""
    import torch
    a, b = _connectors()
    gen = torch.Generator().manual_seed(9)
    tree = [-1, 0, 1, 1]
    trees = [[-1, 0, 1, 1], [-1, -1, 0, 1], [-1, 0, 0, 2], [-1, 0, 1, 2], [-1, -1, -1, 2]]
    steps = [[[0, 1, 3], [0, 1, 2], [0], [], [0, 1]], [[0], [0, 1, 3], [0, 1, 2], [0, 1], []], [[0, 1, 2], [], [0, 1, 3], [0], [0, 1]]]
    own = [[[0, 1, 3], [1, 3], [0, 1], [0, 1, 2, 3], [2, 3]], [[0], [0, 2], [0, 2, 3], [], [1]], [[0, 1, 2], [1, 3], [], [0], [2, 3]]]
    for paths in (own if per_request else steps):
        k, v = _step(gen)
        parents = trees if per_request else tree
        calls = len(a.lib.calls)
        a.commit(IDS, k, v, paths, parents=parents, stream=host)
        b.append_path(IDS, k, v, paths, parents=parents, stream=host)
        assert a.lib.calls[calls:] == ["write_pairs"]
        _same_state(a, b)


def test_commit_refuses_what_append_path_refuses_and_changes_nothing(host):
    import torch
    a, _ = _connectors()
    gen = torch.Generator().manual_seed(4)
    k, v = _step(gen)
    a.commit(IDS, k, v, [[0], [0, 1], [0, 1, 2], [], [0]], stream=host)
    tree = [-1, 0, 1, 1]

    def state():
        return ([a.length(rid) for rid in IDS], [None if a.requests[rid].tail_k is None else a.requests[rid].tail_k.clone() for rid in IDS],
                list(a.lib.writes), list(a.lib.calls), a._epoch, a._tail_ids)

    before = state()
    none = [[] for _ in IDS]
    bad = [
        dict(nodes=[[0, 2, 3]] + none[1:], parents=tree),                  # 2 and 3 are siblings
        dict(nodes=[[1, 2]] + none[1:], parents=tree),                     # does not start at a child of the committed context
        dict(nodes=[[2, 1]] + none[1:], parents=None),                     # descends
        dict(nodes=[[0, 0]] + none[1:], parents=None),                     # does not ascend
        dict(nodes=[[0, S]] + none[1:], parents=None),                     # out of range
        dict(nodes=[[-1]] + none[1:], parents=None),
        dict(nodes=none[1:], parents=None),                                # one list per request
    ]
    for case in bad:
        with pytest.raises(ValueError):
            a.commit(IDS, k, v, case["nodes"], parents=case["parents"], stream=host)
    full = a.requests[IDS[1]]
    length = full.length
    full.length = T - 1                                                     # a request one position short of full
    with pytest.raises(ValueError, match="full"):
        a.commit(IDS, k, v, [[0]] + [[0, 1]] + none[2:], stream=host)
    full.length = length
    after = state()
    assert before[0] == after[0] and before[2:] == after[2:]
    for x, y in zip(before[1], after[1]):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y))


def test_pair_gather_encoder_uses_no_flat_memory_instructions():
    """k_compress_pairs<...> keeps the property tests/test_build_guards.py asks of k_compress<...>: rows and records are reached
    through global-address-space accesses (the RLE form keeps k_compress' one tail store of the all-zero record).  It lives in
    row_transfer.o with the other row-transfer kernels: kernels.o, whose headline kernel is pinned by its instructions, holds none
    of them, and row_transfer.o holds nothing else -- no out-of-line device function that a kernel would reach by a pc-relative call."""
    from tests.test_build_guards import OBJ, OBJDUMP, _disassemble
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    if not os.path.exists(os.path.join(OBJ, "row_transfer.o")) or not os.path.exists(os.path.join(OBJ, "kernels.o")):
        import __graft_entry__ as entry
        entry.build()
    family = r"k_(read|compress)_(pairs|slots)"
    stray = sorted(name for name in _disassemble("kernels.o") if re.search(family, name))
    assert not stray, f"row-transfer kernels in kernels.o: {stray}"
    funcs = _disassemble("row_transfer.o")
    # a kernel's symbol is <namespaces>k_<family>[_ex]<template arguments>Ev<argument struct>: the name directly behind the namespaces
    other = sorted(name for name in funcs if not re.match(r"_ZN6speckv\d+_GLOBAL__N_1\d+" + family + r"(_ex)?I[^I]*EEv", name))
    assert funcs and not other, f"row_transfer.o holds functions that are no row-transfer kernel: {other}"
    for pattern, allowed, instances in ((r"k_compress_pairsILi[0134]ELi\dE", 0, 6), (r"k_compress_pairsILi2ELi\dE", 1, 2), (r"k_compress_pairsILi5ELi0E", 0, 1)):
        hits = {name: n for name, n in funcs.items() if re.search(pattern, name)}
        assert len(hits) == instances, (pattern, sorted(hits))
        for name, n in hits.items():
            assert n <= allowed, f"{name}: {n} flat memory instructions (allowed {allowed})"
