"""Not -m gpu: the split pool's life cycle -- speckv_ext_read_pairs_kv / speckv_ext_copy_runs_kv as declared, exported and bound, what they
answer on the null engine, and what SpeckvSplitKVConnector.truncate / fork / commit(nodes=...) hand the library, against a recording
library and brute-force restatements of the header's page rules."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _RecordingLib, _ctypes_of, _declared, _pages_named
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, H, D, T = 4, 8, 128, 64
LAYER = H * D * 2                                       # the real layer stride
ROW = L * LAYER                                         # bytes of a position's rows of all layers
REGION = T // 2


# ------------------------------------------------------------------------------------------------------------- the declarations
def test_both_entries_are_declared_defined_and_bound_behind_the_second_handle_array():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header and speckv_ctypes.EXT_ABI_VERSION == 6
    c_api = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    read, read_kv = _declared(header, "speckv_ext_read_pairs"), _declared(header, "speckv_ext_read_pairs_kv")
    copy, copy_kv = _declared(header, "speckv_ext_copy_runs"), _declared(header, "speckv_ext_copy_runs_kv")
    assert read_kv.startswith("const speckv_handle_t* k_handles, const speckv_handle_t* v_handles, const uint64_t* first_pages,")
    assert read_kv[read_kv.index("const uint64_t* first_pages"):] == read[read.index("const uint64_t* first_pages"):]
    assert copy_kv.startswith("const speckv_handle_t* k_src, const speckv_handle_t* v_src, const speckv_handle_t* k_dst, const speckv_handle_t* v_dst, "
                              "const uint64_t* n_pages,")
    assert copy_kv[copy_kv.index("const uint64_t* n_pages"):] == copy[copy.index("const uint64_t* n_pages"):]
    for name, decl in (("speckv_ext_read_pairs_kv", read_kv), ("speckv_ext_copy_runs_kv", copy_kv)):
        assert _ctypes_of(decl) == speckv_ctypes._EXT_SIGNATURES[name], name       # the binding is the declaration
        assert "speckv_status_t %s(" % name in c_api, name
    # the python bindings: the parents' arguments behind the handle arrays
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(pkg.SpeckvLib.read_pairs_kv) == ["self", "k_handles", "v_handles"] + params(pkg.SpeckvLib.read_pairs)[2:]
    assert params(pkg.SpeckvLib.copy_runs_kv) == ["self", "k_src", "v_src", "k_dst", "v_dst"] + params(pkg.SpeckvLib.copy_runs)[3:]
    text = header[header.index("/* speckv_ext_read_pairs and speckv_ext_copy_runs for the split pool"):header.index("speckv_status_t speckv_ext_read_pairs_kv(")]
    for said in ("SPECKV_EXT_ABI_VERSION stays", "ONE launch", "ACROSS both", "K even, K odd", "num_tokens"):
        assert said in text, said


def test_the_library_exports_both_at_version_6():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_read_pairs_kv") and hasattr(lib, "speckv_ext_copy_runs_kv")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_null_engine_answers_as_for_the_parents_and_touches_nothing():
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        hs = [lib.alloc(64 * 4096) for _ in range(4)]
        buf = np.zeros(4 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        rows = u64(at, 0, at + 2048, 0).reshape(1, 4)
        status = []
        for call, args in ((lib.read_pairs, (u64(hs[0]), u64(0), rows, 8, 1, 2048, 1)),
                           (lib.read_pairs_kv, (u64(hs[0]), u64(hs[1]), u64(0), rows, 8, 1, 2048, 1)),
                           (lib.copy_runs, (u64(hs[0]), u64(hs[2]), u64(2), u64(0, 8), 1)),
                           (lib.copy_runs_kv, (u64(hs[0]), u64(hs[1]), u64(hs[2]), u64(hs[3]), u64(2), u64(0, 8), 1))):
            with pytest.raises(SpeckvError) as e:
                call(*args)
            status.append(e.value.status)
        assert status[0] == status[1] and status[2] == status[3] and status[0] == -2      # SPECKV_ERR_DRIVER: no data path
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _Lib(_RecordingLib):
    def read_pairs_kv(self, k_handles, v_handles, first_pages, rows, page_step, n_layers, layer_stride, stream):
        n = len(k_handles)
        self.calls.append(("read_pairs_kv", [int(h) for h in k_handles], [int(h) for h in v_handles], [int(f) for f in first_pages],
                           np.asarray(rows, dtype=np.uint64).reshape(n, 4).copy(), int(page_step), int(n_layers), int(layer_stride), stream))

    def copy_runs_kv(self, k_src, v_src, k_dst, v_dst, n_pages, run_firsts, stream):
        as_list = lambda x: [int(v) for v in x]
        self.calls.append(("copy_runs_kv", as_list(k_src), as_list(v_src), as_list(k_dst), as_list(v_dst), as_list(n_pages), as_list(run_firsts), stream))

    def read_pairs(self, *a): raise AssertionError("the single-allocation entry on a split pool")
    def copy_runs(self, *a): raise AssertionError("the single-allocation entry on a split pool")


def _rows_named(call):
    """The header's rule of speckv_ext_read_pairs_kv, restated: pair i names page first_pages[i] + l * page_step of k_handles[i] and of
    v_handles[i] for l < n_layers; the halves of the K page go to d_rows[4 i] / d_rows[4 i + 1] + l * layer_stride_bytes, those of the V
    page to d_rows[4 i + 2] / d_rows[4 i + 3] + l * layer_stride_bytes; 0 = not wanted.  -> {(handle, page): (even address, odd address)}"""
    _, ks, vs, firsts, rows, step, n_layers, stride, _ = call
    named = {}
    for i, f in enumerate(firsts):
        for l in range(n_layers):
            for kind, h in enumerate((ks[i], vs[i])):
                key = (h, f + l * step)
                assert key not in named, "two pairs share a page"
                even, odd = int(rows[i, 2 * kind]), int(rows[i, 2 * kind + 1])
                named[key] = (even + l * stride if even else 0, odd + l * stride if odd else 0)
    return named


def _records_named(call):
    """The header's rule of speckv_ext_copy_runs_kv, restated: pair i copies pages [run_firsts[r], run_firsts[r] + n_pages[i]) for every run r
    from k_src[i] to k_dst[i] and from v_src[i] to v_dst[i].  -> {(destination handle, page): source handle}"""
    _, k_src, v_src, k_dst, v_dst, n_pages, firsts, _ = call
    named = {}
    for i, n in enumerate(n_pages):
        for src, dst in ((k_src[i], k_dst[i]), (v_src[i], v_dst[i])):
            for f in firsts:
                for p in range(f, f + n):
                    assert (dst, p) not in named, "a destination page named twice"
                    named[(dst, p)] = src
    return named


def _connector(torch, lengths):
    """requests 0.. with the given lengths and, where odd, random tails; nothing of it went through the library"""
    lib = _Lib()
    conn = SpeckvSplitKVConnector(lib, L, H, D, T)
    tails = {}
    for b, n in enumerate(lengths):
        conn.add_request(b)
        r = conn.requests[b]
        r.length = n
        if n & 1:
            r.tail_k, r.tail_v = torch.randn((L, H, D)).to(torch.float16), torch.randn((L, H, D)).to(torch.float16)
            tails[b] = (r.tail_k, r.tail_v)
    del lib.calls[:]
    return lib, conn, tails


# every case of truncate_plan: unchanged (even, odd), even -> even, odd -> even (drop), odd -> odd, even -> odd, odd -> its own even part,
# to 1 and to 0
TRUNCATE = [(34, 34), (33, 33), (34, 30), (33, 32), (33, 31), (34, 31), (35, 34), (64, 1), (7, 0), (2, 1), (33, 2), (63, 33)]


def test_truncate_names_exactly_the_rows_that_come_back(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lengths, new = [a for a, _ in TRUNCATE], [b for _, b in TRUNCATE]
    lib, conn, tails = _connector(torch, lengths)
    epoch = conn._epoch
    conn._tails = conn._fold = conn._spec = conn._tree = ("stale",)
    conn.truncate(list(range(len(lengths))), new, stream=st)
    (call,) = lib.calls                                                         # ONE call for the whole batch
    assert call[0] == "read_pairs_kv" and call[5] == REGION and call[6] == L and call[7] == LAYER and call[8] == st.cuda_stream
    want = {}
    for b, (n0, n) in enumerate(zip(lengths, new)):
        r = conn.requests[b]
        assert conn.length(b) == n
        if n == n0:
            if n & 1:
                assert r.tail_k is tails[b][0] and r.tail_v is tails[b][1]      # untouched
            continue
        if not n & 1:
            assert r.tail_k is None and r.tail_v is None, b
            continue
        # the new last position n - 1 is the even half of a stored page, in every layer's region of both allocations
        assert r.tail_k.shape == (L, H, D) and r.tail_k.dtype == torch.float16 and r.tail_k.is_contiguous() and r.tail_k.data_ptr() % 16 == 0
        for l in range(L):
            for h, t in ((r.k_handle, r.tail_k), (r.v_handle, r.tail_v)):
                want[(h, l * REGION + (n - 1) // 2)] = (t.data_ptr() + l * LAYER, 0)
    assert _rows_named(call) == want
    assert conn._epoch > epoch and conn._tails[0] is None and conn._fold[0] is None and conn._spec[0] is None and conn._tree[0] is None


def test_truncate_that_needs_no_row_makes_no_call_and_refusals_change_nothing(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn, tails = _connector(torch, [34, 33, 10, 9])
    conn.truncate([0, 1, 2, 3], [30, 32, 10, 9], stream=st)                     # even -> even, a dropped tail, unchanged
    assert lib.calls == [] and [conn.length(b) for b in range(4)] == [30, 32, 10, 9]
    assert conn.requests[1].tail_k is None and conn.requests[3].tail_k is tails[3][0]
    epoch = conn._epoch
    for bad in ([31, 32, 10, 9], [30, 32, 10, -1], [30, 32, 10]):
        with pytest.raises(ValueError):
            conn.truncate([0, 1, 2, 3], bad, stream=st)
    with pytest.raises(KeyError):
        conn.truncate([0, 99], [1, 1], stream=st)
    assert lib.calls == [] and [conn.length(b) for b in range(4)] == [30, 32, 10, 9] and conn._epoch == epoch


# (source length, forked length or None = all): every case of fork_plan, one source three times
FORK = [(34, None), (33, None), (33, 31), (33, 32), (34, 33), (34, 0), (1, None), (2, 1), (33, 33), (0, None)]


def test_fork_names_exactly_the_records_and_rows(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    src_lengths = [34, 33, 1, 2, 0]
    src_of = [0, 1, 1, 1, 0, 0, 2, 3, 1, 4]
    assert [src_lengths[s] for s in src_of] == [a for a, _ in FORK]
    lengths = [a if n is None else n for a, n in FORK]
    lib, conn, tails = _connector(torch, src_lengths)
    new_ids = list(range(100, 100 + len(FORK)))
    held = conn.fork(src_of, new_ids, None if all(n is None for _, n in FORK) else lengths, stream=st)
    calls = [c for c in lib.calls if c[0] not in ("alloc", "set_layout")]
    assert [c[0] for c in calls] == ["copy_runs_kv", "read_pairs_kv"]          # one of each for the whole batch
    assert [c[2] for c in lib.calls if c[0] == "alloc"] == [4, 5] * len(FORK)  # an FP8 and an MXFP4 allocation per fork
    copy, read = calls
    assert copy[6] == [l * REGION for l in range(L)] and copy[7] == st.cuda_stream
    assert read[5] == REGION and read[6] == L and read[7] == LAYER and read[8] == st.cuda_stream
    want_rec, want_rows = {}, {}
    for s, rid, n in zip(src_of, new_ids, lengths):
        src, new = conn.requests[s], conn.requests[rid]
        assert conn.length(rid) == n and conn.length(s) == src_lengths[s]
        for p in range(0, n & ~1, 2):                                           # every stored pair, every layer, both allocations
            for l in range(L):
                want_rec[(new.k_handle, l * REGION + p // 2)] = src.k_handle
                want_rec[(new.v_handle, l * REGION + p // 2)] = src.v_handle
        if not n & 1:
            assert new.tail_k is None and new.tail_v is None
        elif n == src_lengths[s]:                                               # a clone of the source's tail, never a view
            assert torch.equal(new.tail_k, tails[s][0]) and torch.equal(new.tail_v, tails[s][1])
            assert new.tail_k.data_ptr() != tails[s][0].data_ptr() and src.tail_k is tails[s][0]
        else:                                                                   # read from the SOURCE's stored page
            assert any(new.tail_k.data_ptr() - t.data_ptr() in range(0, t.numel() * 2) for t in held)
            for l in range(L):
                want_rows[(src.k_handle, l * REGION + (n - 1) // 2, rid)] = (new.tail_k.data_ptr() + l * LAYER, 0)
                want_rows[(src.v_handle, l * REGION + (n - 1) // 2, rid)] = (new.tail_v.data_ptr() + l * LAYER, 0)
    assert _records_named(copy) == want_rec
    # (two forks may read one source page: the rule's dictionary is keyed by the page alone, so restate it per pair here)
    got_rows = {}
    _, ks, vs, firsts, rows, step, n_layers, stride, _ = read
    readers = [rid for s, rid, n in zip(src_of, new_ids, lengths) if n & 1 and n != src_lengths[s]]
    assert len(readers) == len(firsts)
    for i, rid in enumerate(readers):
        one = ("read_pairs_kv", ks[i:i + 1], vs[i:i + 1], firsts[i:i + 1], rows[i:i + 1], step, n_layers, stride, None)
        for (h, page), at in _rows_named(one).items():
            got_rows[(h, page, rid)] = at
    assert got_rows == want_rows


def test_fork_refusals_come_before_any_allocation_and_a_failed_launch_frees(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn, tails = _connector(torch, [34, 33])
    epoch = conn._epoch
    for src, new, lengths, error in (([0], [1], None, KeyError), ([0, 0], [5, 5], None, KeyError), ([9], [5], None, KeyError),
                                     ([0], [5], [35], ValueError), ([0], [5], [-1], ValueError), ([0, 1], [5], None, ValueError),
                                     ([0], [5], [1, 2], ValueError)):
        with pytest.raises(error):
            conn.fork(src, new, lengths, stream=st)
    assert lib.calls == [] and sorted(conn.requests) == [0, 1] and conn._epoch == epoch
    assert conn.fork([], [], stream=st) == [] and lib.calls == []

    def refuse(*a):
        raise SpeckvError("speckv_ext_copy_runs_kv", -4)
    monkeypatch.setattr(lib, "copy_runs_kv", refuse)
    with pytest.raises(SpeckvError):
        conn.fork([0, 1], [5, 6], stream=st)
    made = [c[1] for c in lib.calls if c[0] == "alloc"]
    assert len(made) == 4 and sorted(c[1] for c in lib.calls if c[0] == "free") == sorted(made)
    assert sorted(conn.requests) == [0, 1] and conn.length(0) == 34 and conn.length(1) == 33 and conn.requests[1].tail_k is tails[1][0]


def test_fork_of_nothing_stored_is_allocations_only(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn, tails = _connector(torch, [34, 1])
    conn.fork([0, 1], [5, 6], [0, 1], stream=st)                                # length 0, and a held tail alone
    assert {c[0] for c in lib.calls} == {"alloc", "set_layout"}
    assert conn.length(5) == 0 and conn.length(6) == 1 and torch.equal(conn.requests[6].tail_k, tails[1][0])


# ------------------------------------------------------------------------------------------------------------ commit(nodes=...)
PARENTS = [-1, 0, 0, 1, 1, 2, 5]                                                # a tree of 7 nodes
PATHS = [[0, 2, 5, 6], [0, 1, 4], [], [0], [0, 1, 3]]
BEFORE = [33, 34, 7, 1, 0]


def test_commit_of_a_path_is_commit_of_the_gathered_rows(monkeypatch):
    """two write_pairs calls, and through the header's page rule every page of both allocations names the rows that commit(n_accept)
    names for the path's rows gathered to the front"""
    torch, st = _cpu_torch(monkeypatch)
    B, S = len(PATHS), len(PARENTS)
    k_new, v_new = torch.randn((B, S, L, H, D)).to(torch.float16), torch.randn((B, S, L, H, D)).to(torch.float16)
    longest = max(len(p) for p in PATHS)
    k_path, v_path = torch.zeros((B, longest, L, H, D), dtype=torch.float16), torch.zeros((B, longest, L, H, D), dtype=torch.float16)
    for b, path in enumerate(PATHS):
        for t, j in enumerate(path):
            k_path[b, t], v_path[b, t] = k_new[b, j], v_new[b, j]
    torch.manual_seed(5)
    lib_a, a, tails_a = _connector(torch, BEFORE)
    torch.manual_seed(5)
    lib_b, b_, tails_b = _connector(torch, BEFORE)
    ids = list(range(B))
    a.commit(ids, k_new, v_new, nodes=PATHS, parents=PARENTS, stream=st)
    b_.commit(ids, k_path, v_path, [len(p) for p in PATHS], stream=st)
    assert [c[0] for c in lib_a.calls] == ["write_pairs", "write_pairs"] == [c[0] for c in lib_b.calls]

    def meaning(addr, new, width, tails, kind, node_of):
        """an address as (request, step node, byte inside the position's rows), or the tail it points into"""
        off = addr - new.data_ptr()
        if 0 <= off < new.numel() * 2:
            b, t = divmod(off // ROW, width)
            return ("new", b, node_of(b, t), off % ROW)
        for b, pair in tails.items():
            if 0 <= addr - pair[kind].data_ptr() < ROW:
                return ("tail", b, addr - pair[kind].data_ptr())
        raise AssertionError("an address outside every tensor of the step")

    for kind in (0, 1):
        ca, cb = lib_a.calls[kind], lib_b.calls[kind]
        assert ca[1] == cb[1] and ca[2] == cb[2] and ca[4:] == cb[4:]           # handles, pages, step, layers, stride, stream
        na, nb = _pages_named(ca), _pages_named(cb)
        assert set(na) == set(nb)
        for page in na:
            got = [meaning(x, (k_new, v_new)[kind], S, tails_a, kind, lambda b, t: t) for x in na[page]]
            want = [meaning(x, (k_path, v_path)[kind], longest, tails_b, kind, lambda b, t: PATHS[b][t]) for x in nb[page]]
            assert got == want, page
    for rid in ids:
        ra, rb = a.requests[rid], b_.requests[rid]
        assert ra.length == rb.length == BEFORE[rid] + len(PATHS[rid])
        assert (ra.tail_k is None) == (rb.tail_k is None)
        if ra.tail_k is not None:
            assert torch.equal(ra.tail_k, rb.tail_k) and torch.equal(ra.tail_v, rb.tail_v)
    # a prefix path is the prefix commit, call for call
    torch.manual_seed(5)
    lib_c, c, _ = _connector(torch, BEFORE)
    torch.manual_seed(5)
    lib_d, d, _ = _connector(torch, BEFORE)
    for rid in ids:                                                             # the same tail tensors: the addresses must agree
        d.requests[rid].tail_k, d.requests[rid].tail_v = c.requests[rid].tail_k, c.requests[rid].tail_v
    c.commit(ids, k_new, v_new, nodes=[list(range(n)) for n in (4, 3, 0, 1, 7)], stream=st)
    d.commit(ids, k_new, v_new, [4, 3, 0, 1, 7], stream=st)
    assert len(lib_c.calls) == len(lib_d.calls) == 2
    for x, y in zip(lib_c.calls, lib_d.calls):
        assert x[:3] == y[:3] and np.array_equal(x[3], y[3]) and x[4:] == y[4:]


def test_commit_judges_a_path_before_anything_changes(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn, tails = _connector(torch, [33, T - 2])
    k = torch.zeros((2, len(PARENTS), L, H, D), dtype=torch.float16)
    epoch = conn._epoch
    for kwargs in (dict(nodes=[[0, 3], []], parents=PARENTS),                   # 3 is no child of 0
                   dict(nodes=[[1], []], parents=PARENTS),                      # does not start at the committed context
                   dict(nodes=[[0, 7], []]),                                    # outside the step
                   dict(nodes=[[2, 1], []]),                                    # without parents: must ascend
                   dict(nodes=[[0], [0, 1, 3]], parents=PARENTS),               # request 1 is full
                   dict(nodes=[[0]], parents=PARENTS),                          # one path per request
                   dict(nodes=[[0], []], parents=[-1, 0]),                      # one parent per node
                   dict(),                                                      # neither
                   dict(n_accept=[1, 0], nodes=[[0], []]),                      # both
                   dict(n_accept=[1, 0], parents=PARENTS)):                     # parents without a path
        with pytest.raises(ValueError):
            conn.commit([0, 1], k, k, stream=st, **kwargs)
    assert lib.calls == [] and conn.length(0) == 33 and conn.length(1) == T - 2 and conn._epoch == epoch
    assert conn.requests[0].tail_k is tails[0][0]
