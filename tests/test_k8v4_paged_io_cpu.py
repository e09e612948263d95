"""Not -m gpu: the paged-cache transfers of the split pool (speckv_ext_read_slots_kv / speckv_ext_write_slots_kv,
SpeckvSplitKVConnector.load_paged / store_paged): the declarations, the no-data-path engine, the bindings, paged_plan against a
brute-force restatement, the shared cache-geometry judgement against SpeckvKVConnector._paged_geometry(bf16=True), and what the
connector hands the library, against a recording library."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_shared import paged_cache_geometry
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from tests.test_paged_io_cpu import _RecordingLib, _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("speckv_ext_read_slots_kv", "speckv_ext_write_slots_kv")


# ------------------------------------------------------------------------------------------------------------- the declarations
def test_the_kv_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                     # additive entries: the version stays
    assert "SPECKV_EXT_ABI_VERSION stays" in header                          # ... and the entries' comment says so
    c_api = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    for name in ENTRIES:
        m = re.search(r"speckv_status_t\s+%s\s*\(([^;]*)\);" % name, header)
        assert m and name in c_api, name
        args = m.group(1)
        assert re.search(r"k_handles,\s*const speckv_handle_t\*\s*v_handles", args) and "const speckv_ext_slot_rows_t* rows" in args, name
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"^\s*([A-Za-z_*]+);", exports.split("local:")[0], flags=re.M)
    for name in ENTRIES:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
    ex, kv = speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_slots_ex"], speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_slots_kv"]
    assert kv == speckv_ctypes._EXT_SIGNATURES["speckv_ext_write_slots_kv"]
    assert kv == [C.c_void_p] + ex                                           # the _ex arguments behind a second handle array
    lib = C.CDLL(pkg.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_kv_entries_on_the_null_engine_have_no_data_path():
    """on the no-data-path engine both entries return what the _ex entries return there, and touch nothing"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        k, v = lib.alloc(64 * 4096), lib.alloc(64 * 4096)                   # (the boundary comes before any judgement of the handles)
        buf = np.zeros(2 * 4 * 2048 + 16, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        slots = np.asarray([0, 1, 2, 3], dtype=np.int64)
        u64 = lambda *x: np.asarray(x, dtype=np.uint64)
        status = []
        for call in (lib.read_slots_ex, lib.write_slots_ex):
            with pytest.raises(SpeckvError) as e:
                call(u64(k), u64(0), u64(4), u64(0), slots.ctypes.data, 4, u64(at), 0, 4 * 2048, 16, 1, elem=1)
            status.append(e.value.status)
        for call in (lib.read_slots_kv, lib.write_slots_kv):
            with pytest.raises(SpeckvError) as e:
                call(u64(k), u64(v), u64(0), u64(4), u64(0), slots.ctypes.data, 4, u64(at), 0, 4 * 2048, 16, 1, elem=1)
            status.append(e.value.status)
        assert status == [-2] * 4                                            # SPECKV_ERR_DRIVER
        assert not buf.any()
    finally:
        lib.finalize()


def test_the_bindings_have_the_documented_defaults():
    for name in ("read_slots_kv", "write_slots_kv"):
        sig = inspect.signature(getattr(speckv_ctypes.SpeckvLib, name))
        names = list(sig.parameters)
        assert names[:13] == ["self", "k_handles", "v_handles", "first_tokens", "n_tokens", "slot_begins", "d_slots", "n_slots", "caches",
                              "layer_begin", "kind_stride", "page_step", "stream"], name
        assert all(sig.parameters[n].default is inspect.Parameter.empty for n in names[:13]), name
        defaults = {n: sig.parameters[n].default for n in names[13:]}
        assert defaults["elem"] == speckv_ctypes.SLOT_ELEM_FP16 == 0 and defaults["held_in"] is None and defaults["held_stride"] == 0 \
            and defaults["held_out"] is None, (name, defaults)
        assert names[13:17] == ["elem", "held_in", "held_stride", "held_out"], name


# ------------------------------------------------------------------------------------------------------------------ paged_plan
def test_paged_plan_against_brute_force():
    """all (length, first, count) with length <= 9, as a read and -- first = length -- as a write, one and three spans at a time:
    first_token, n_tokens, slot_begin, the pair range the engine derives (SpeckvKVConnector.paged_spans, less the pair of a held
    position), held-in exactly when a write starts on an odd stored boundary or a read ends on the odd last position, held-out
    exactly when the new length is odd"""
    plan = SpeckvSplitKVConnector.paged_plan
    reads = [(n, f, c) for n in range(10) for f in range(n + 1) for c in range(n - f + 1)]
    for n, f, c in reads:
        (first, count, begin, h_in, h_out), = plan([n], [f], [c])
        positions = set(range(f, f + c))
        tail = {n - 1} if n & 1 else set()                                   # the position that lives in the tail, in no page
        assert (first, count, begin) == (f, c, 0) and h_out is False
        assert h_in == bool(positions & tail), (n, f, c)
        # the pages the one call decodes: those of the span's stored positions
        pair0, n_pairs, _ = SpeckvKVConnector.paged_spans([f], [c])[0]
        decoded = range(pair0, pair0 + n_pairs - (1 if h_in else 0)) if c else range(0)
        assert set(decoded) == {p // 2 for p in positions - tail}, (n, f, c)
        if h_in:
            assert (first + count - 1) % 2 == 0                              # what speckv_ext_read_slots_ex asks of a held-in span
    writes = [(n, c) for n in range(10) for c in range(10)]
    for n, c in writes:
        (first, count, begin, h_in, h_out), = plan([n], None, [c])
        assert count == c and begin == 0
        assert h_in == bool(c and n & 1) and h_out == bool(c and (n + c) & 1), (n, c)
        assert first == (n if c else n & ~1)
        assert (first & 1) == h_in and ((first + count) & 1) == h_out        # whole pairs only: what speckv_ext_write_slots_ex asks
        # the pages encoded: every whole pair of the positions the request then holds that was not whole before
        pairs = range(first // 2, (first + count) // 2)
        assert set(pairs) == {p for p in range((n + c) // 2) if p >= n // 2}, (n, c)
    rng = np.random.default_rng(3)
    for _ in range(200):                                                     # several spans: the slot begins are the counts in front
        pick = [reads[i] for i in rng.integers(0, len(reads), 3)]
        got = plan([n for n, _, _ in pick], [f for _, f, _ in pick], [c for _, _, c in pick])
        at = 0
        for (n, f, c), g in zip(pick, got):
            assert g == plan([n], [f], [c])[0][:2] + (at,) + plan([n], [f], [c])[0][3:]
            at += c
        pick = [writes[i] for i in rng.integers(0, len(writes), 3)]
        got = plan([n for n, _ in pick], None, [c for _, c in pick])
        at = 0
        for (n, c), g in zip(pick, got):
            assert g == plan([n], None, [c])[0][:2] + (at,) + plan([n], None, [c])[0][3:]
            at += c
    assert plan([0, 6, 7], None, [5, 0, 3]) == [(0, 5, 0, False, True), (6, 0, 5, False, False), (7, 3, 5, True, False)]
    for bad in (([4], [3], [2]), ([4], [0], [-1]), ([4, 4], [0], [1, 1]), ([4], [-1], [1])):
        with pytest.raises(ValueError):
            plan(*bad)
    with pytest.raises(ValueError):
        plan([4], None, [-1])


# ------------------------------------------------------------------------------------------------------------ the cache geometry
def test_the_geometry_helper_judges_as_the_fp8_connector_does():
    """a table of shapes, strides, dtypes and alignments: paged_cache_geometry accepts and refuses what
    SpeckvKVConnector._paged_geometry(bf16=True) does, with the same geometry, and names what was wrong"""
    import torch
    L, H, D, BS, NB = 2, 8, 128, 16, 6
    z = lambda *shape, dtype=torch.float16: torch.zeros(shape, dtype=dtype)
    off = z(2 * NB * BS * H * D + 8)
    table = {
        "fp16": ([z(2, NB, BS, H, D) for _ in range(L)], True),
        "bf16": ([z(2, NB, BS, H, D, dtype=torch.bfloat16) for _ in range(L)], True),
        "a view between guard blocks": ([z(2, NB + 2, BS, H, D)[:, 1:-1] for _ in range(L)], True),
        "heads and dim that give 2048 bytes otherwise": ([z(2, NB, BS, 4, 256) for _ in range(L)], True),
        "one cache too few": ([z(2, NB, BS, H, D)], False),
        "fp32": ([z(2, NB, BS, H, D, dtype=torch.float32) for _ in range(L)], False),
        "mixed dtypes": ([z(2, NB, BS, H, D), z(2, NB, BS, H, D, dtype=torch.bfloat16)], False),
        "bf16 behind fp16": ([z(2, NB, BS, H, D, dtype=torch.bfloat16), z(2, NB, BS, H, D)], False),
        "four dimensions": ([z(2, NB * BS, H, D) for _ in range(L)], False),
        "three planes": ([z(3, NB, BS, H, D) for _ in range(L)], False),
        "rows of 1024 bytes": ([z(2, NB, BS, 4, D) for _ in range(L)], False),
        "strided channels": ([z(2, NB, BS, H, 2 * D)[..., :D] for _ in range(L)], False),
        "blocks apart": ([z(2, NB, 2 * BS, H, D)[:, :, :BS] for _ in range(L)], False),
        "different block counts": ([z(2, NB, BS, H, D), z(2, NB + 1, BS, H, D)], False),
        "not 16-byte aligned": ([off[4:4 + 2 * NB * BS * H * D].view(2, NB, BS, H, D) for _ in range(L)], False),
    }
    for what, (caches, ok) in table.items():
        conn = SpeckvKVConnector(_RecordingLib(), L, H, D, 64, "fp8")
        want = conn._paged_geometry(caches, bf16=True)
        geo, wrong = paged_cache_geometry(caches, L, bf16=True)
        assert geo == want and (geo is not None) == ok and (wrong is None) == ok, (what, geo, want, wrong)
        if not ok:
            assert isinstance(wrong, str) and wrong
        plain = paged_cache_geometry(caches, L)[0]
        assert plain == conn._paged_geometry(caches), what
    geo, _ = paged_cache_geometry(table["bf16"][0], L, bf16=True)
    assert geo == (NB * BS, NB * BS * 2048, 1) and paged_cache_geometry(table["bf16"][0], L)[0] is None
    assert paged_cache_geometry(table["a view between guard blocks"][0], L, bf16=True)[0] == (NB * BS, (NB + 2) * BS * 2048, 0)


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _RecordingKVLib(_RecordingLib):
    def read_slots_kv(self, *a, **k): self.calls.append(("read_slots_kv",) + a + (k,))
    def write_slots_kv(self, *a, **k): self.calls.append(("write_slots_kv",) + a + (k,))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_the_split_connector_hands_over_one_call_each_way(monkeypatch, dtype):
    torch, st = _cpu_torch(monkeypatch)
    L, H, D, T, BS, NB = 2, 8, 128, 64, 16, 6
    elem = 1 if dtype == "bfloat16" else 0
    caches = [torch.zeros((2, NB + 2, BS, H, D), dtype=getattr(torch, dtype))[:, 1:-1] for _ in range(L)]
    conn = SpeckvSplitKVConnector(_RecordingKVLib(), L, H, D, T)
    handles = {rid: conn.add_request(rid) for rid in (1, 2, 3)}
    for rid, n in ((1, 35), (2, 32), (3, 0)):
        conn.requests[rid].length = n
    tk, tv = torch.ones((L, H, D), dtype=torch.float16), torch.ones((L, H, D), dtype=torch.float16)
    conn.requests[1].tail_k, conn.requests[1].tail_v = tk, tv
    slots = torch.arange(5 + 31 + 4, dtype=torch.int64)
    conn.load_paged([1, 2, 1], [30, 1, 30], [5, 31, 4], slots, caches, stream=st)
    (name, ks, vs, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "read_slots_kv" and list(ks) == [handles[r][0] for r in (1, 2, 1)] and list(vs) == [handles[r][1] for r in (1, 2, 1)]
    assert list(firsts) == [30, 1, 30] and list(counts) == [5, 31, 4] and list(begins) == [0, 5, 36] and d_slots == slots.data_ptr()
    assert n_slots == NB * BS and list(bases) == [c.data_ptr() for c in caches] and layer_begin == 0
    assert kind_stride == caches[0].stride(0) * 2 and step == T // 2 and stream == st.cuda_stream
    assert kw["elem"] == elem and kw["held_stride"] == H * D * 2 and kw.get("held_out") is None
    assert list(kw["held_in"]) == [tk.data_ptr(), tv.data_ptr(), 0, 0, 0, 0]  # only the span that ends on the tail
    conn.lib.calls.clear()
    conn.load_paged([1, 2], [0, 0], [0, 0], slots[:0], caches, stream=st)
    assert conn.lib.calls == []                                              # nothing is launched when every count is 0
    # ---- store: 35 + 2 -> 37 (held-in and held-out), 32 + 0, 0 + 5 -> 5 (held-out)
    epoch = conn._epoch
    held = conn.store_paged([1, 2, 3], [2, 0, 5], torch.arange(7, dtype=torch.int64), caches, stream=st)
    (name, ks, vs, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "write_slots_kv" and list(ks) == [handles[r][0] for r in (1, 2, 3)] and list(vs) == [handles[r][1] for r in (1, 2, 3)]
    assert list(firsts) == [35, 32, 0] and list(counts) == [2, 0, 5] and list(begins) == [0, 2, 2] and kw["elem"] == elem
    assert list(kw["held_in"]) == [tk.data_ptr(), tv.data_ptr(), 0, 0, 0, 0] and kw["held_stride"] == H * D * 2
    r1, r3 = conn.requests[1], conn.requests[3]
    row = L * H * D * 2
    assert list(kw["held_out"]) == [r1.tail_k.data_ptr(), r1.tail_v.data_ptr(), 0, 0, r3.tail_k.data_ptr(), r3.tail_v.data_ptr()]
    assert r3.tail_k.data_ptr() - r1.tail_k.data_ptr() == row and tuple(r1.tail_k.shape) == (L, H, D) and r1.tail_k.dtype == torch.float16
    assert [conn.length(r) for r in (1, 2, 3)] == [37, 32, 5] and conn._epoch != epoch and conn.requests[2].tail_k is None
    assert any(t is tk for t in held) and any(t is tv for t in held)         # the rows the launch read stay alive with the caller
    # ---- refusals before any state changes
    conn.lib.calls.clear()
    epoch = conn._epoch
    one = torch.arange(1, dtype=torch.int64)
    for bad in (lambda: conn.store_paged([1, 1], [1, 0], one, caches, stream=st),
                lambda: conn.store_paged([2], [T], torch.arange(T, dtype=torch.int64), caches, stream=st),
                lambda: conn.store_paged([2], [2], one, caches, stream=st),
                lambda: conn.store_paged([2], [1], one.to(torch.int32), caches, stream=st),
                lambda: conn.store_paged([2], [1], one, [c.to(torch.float32) for c in caches], stream=st),
                lambda: conn.store_paged([2], [1], one, caches[:1], stream=st),
                lambda: conn.load_paged([2], [32], [1], one, caches, stream=st),
                lambda: conn.load_paged([2], [0], [1], one, [c.to(torch.float32) for c in caches], stream=st)):
        with pytest.raises(ValueError):
            bad()
    assert conn.lib.calls == [] and conn._epoch == epoch and [conn.length(r) for r in (1, 2, 3)] == [37, 32, 5]
    with pytest.raises(ValueError, match="float32"):                         # the refusal names what was wrong
        conn.load_paged([2], [0], [1], one, [c.to(torch.float32) for c in caches], stream=st)
