"""Not -m gpu: the fused paged-cache route (speckv_ext_read_slots_ex / speckv_ext_write_slots_ex, load_paged / store_paged with
fused=True).

The two conversion rules of include/speckv_ext.h as numpy restatements -- the pin every GPU test compares against -- checked
against torch's CPU casts over all 65 536 patterns; the declarations; and what the connector hands the library for bf16 caches and
odd lengths, against a recording library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests.test_paged_io_cpu import _RecordingLib, _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("speckv_ext_read_slots_ex", "speckv_ext_write_slots_ex")


# --------------------------------------------------------------------------------------------------------- the conversion rules
def bf16_to_fp16_bits(bits):
    """bf16 row -> pool: the exact value rounded once to fp16, nearest even (uint16 bf16 bits -> uint16 fp16 bits)"""
    f32 = (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return f32.astype(np.float16).view(np.uint16)


def fp16_to_bf16_bits(bits):
    """pool -> bf16 row: the decoded fp16 value rounded once to bf16, nearest even (uint16 fp16 bits -> uint16 bf16 bits).  Says
    nothing about a NaN: compare those by position (equal_off_nan)."""
    f = np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (((f + 0x7FFF + ((f >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def fp16_is_nan(bits):
    return (np.asarray(bits) & 0x7FFF) > 0x7C00


def bf16_is_nan(bits):
    return (np.asarray(bits) & 0x7FFF) > 0x7F80


def equal_off_nan(got, want, nan_in, is_nan):
    """bits equal wherever the input was no NaN, a NaN (any payload) wherever it was one"""
    got, want, nan_in = np.asarray(got), np.asarray(want), np.asarray(nan_in)
    return bool(np.array_equal(got[~nan_in], want[~nan_in]) and is_nan(got[nan_in]).all())


def test_both_conversions_against_torch_over_all_patterns():
    import torch
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    t = torch.from_numpy(bits.view(np.int16).copy())
    down = t.view(torch.bfloat16).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    mine = bf16_to_fp16_bits(bits)
    nan = bf16_is_nan(bits)
    assert np.array_equal(mine[~nan], down[~nan]) and fp16_is_nan(down[nan]).all() and fp16_is_nan(mine[nan]).all()
    finite = ~nan & ((bits & 0x7FFF) != 0x7F80)
    assert int((finite & ((mine & 0x7FFF) == 0x7C00)).sum()) == 28672         # finite bf16 values that overflow to +-inf
    assert int((((bits & 0x7FFF) != 0) & ((mine & 0x7FFF) == 0)).sum()) == 26112     # non-zero ones that round to +-0
    assert ((mine & 0x8000) == (bits & 0x8000))[~nan].all()                  # the sign stays, of a zero too
    sub = (mine & 0x7FFF) - 1 < 0x3FF                                        # fp16 subnormals are produced, not flushed
    assert sub.any() and ((bits[sub] & 0x7FFF) != 0).all()
    up = t.view(torch.float16).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    mine = fp16_to_bf16_bits(bits)
    nan = fp16_is_nan(bits)
    assert np.array_equal(mine[~nan], up[~nan]) and bf16_is_nan(up[nan]).all()            # (the restatement is silent on NaN)
    # bf16 -> fp16 -> bf16 is the identity wherever fp16 can hold the value
    exact = ~bf16_is_nan(bits) & (bf16_to_fp16_bits(bits).view(np.float16).astype(np.float32) == (bits.astype(np.uint32) << 16).view(np.float32))
    assert np.array_equal(fp16_to_bf16_bits(bf16_to_fp16_bits(bits))[exact], bits[exact])


# ------------------------------------------------------------------------------------------------------------- the declarations
def test_the_ex_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                     # additive entries: the version stays
    c_api = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    for name in ENTRIES:
        assert re.search(r"speckv_status_t\s+%s\s*\(" % name, header) and name in c_api, name
    assert "speckv_ext_slot_rows_t" in header and "SPECKV_SLOT_ELEM_BF16 1u" in header and "SPECKV_SLOT_ELEM_FP16 0u" in header
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_slots_ex"]
    assert sig == speckv_ctypes._EXT_SIGNATURES["speckv_ext_write_slots_ex"]
    plain = speckv_ctypes._EXT_SIGNATURES["speckv_ext_read_slots"]
    assert sig[:12] == plain[:12] and sig[12:] == [C.c_void_p, C.c_void_p]    # today's arguments, the options, the stream
    rows = speckv_ctypes.SlotRows
    assert C.sizeof(rows) == 32 and rows.d_held_in.offset == 8 and rows.d_held_out.offset == 16 and rows.held_layer_stride_bytes.offset == 24
    assert (speckv_ctypes.SLOT_ELEM_FP16, speckv_ctypes.SLOT_ELEM_BF16) == (0, 1)
    lib = C.CDLL(pkg.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_ex_entries_on_the_null_engine_have_no_data_path():
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(2 * 4 * 2048 + 16, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        slots = np.asarray([0, 1, 2, 3], dtype=np.int64)
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        for call in (lib.read_slots_ex, lib.write_slots_ex):
            with pytest.raises(SpeckvError) as e:
                call(u64(h), u64(0), u64(4), u64(0), slots.ctypes.data, 4, u64(at), 0, 4 * 2048, 16, 1, elem=1)
            assert e.value.status == -2                                      # SPECKV_ERR_DRIVER
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _RecordingExLib(_RecordingLib):
    def read_slots_ex(self, *a, **k): self.calls.append(("read_slots_ex",) + a + (k,))
    def write_slots_ex(self, *a, **k): self.calls.append(("write_slots_ex",) + a + (k,))


L, H, D, T, BS, NB = 2, 8, 128, 64, 16, 6


def _fresh(lengths=((1, 34), (2, 32))):
    conn = SpeckvKVConnector(_RecordingExLib(), L, H, D, T, "fp8")
    for rid, n in lengths:
        conn.add_request(rid)
        conn.requests[rid].length = n
    return conn


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_fused_calls_for_even_and_odd_lengths(monkeypatch, dtype):
    """the one call each way: spans, slot begins, element type, which spans carry held-in / held-out rows, their addresses and the
    stride; lengths, _epoch and the batched tails afterwards"""
    torch, st = _cpu_torch(monkeypatch)
    dt = getattr(torch, dtype)
    elem = 1 if dtype == "bfloat16" else 0
    caches = [torch.zeros((2, NB + 2, BS, H, D), dtype=dt)[:, 1:-1] for _ in range(L)]
    assert _fresh()._paged_geometry(caches, bf16=True) == (NB * BS, caches[0].stride(0) * 2, elem)
    assert (_fresh()._paged_geometry(caches) is None) == (elem == 1)          # the plain rule is as it was
    # ---- load: request 1 has 35 positions (a tail), request 2 has 32
    conn = _fresh(((1, 35), (2, 32)))
    tk, tv = torch.ones((1, L, H, D), dtype=torch.float16), torch.ones((1, L, H, D), dtype=torch.float16)
    conn.requests[1].set_tail(tk, tv, 0)
    slots = torch.arange(5 + 31 + 4, dtype=torch.int64)
    conn.load_paged([1, 2, 1], [30, 1, 30], [5, 31, 4], slots, caches, stream=st, fused=True)
    (name, handles, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "read_slots_ex" and list(handles) == [1, 2, 1] and list(firsts) == [30, 1, 30] and list(counts) == [5, 31, 4]
    assert list(begins) == [0, 5, 36] and d_slots == slots.data_ptr() and n_slots == NB * BS and list(bases) == [c.data_ptr() for c in caches]
    assert layer_begin == 0 and kind_stride == caches[0].stride(0) * 2 and step == T // 2 and stream == st.cuda_stream
    assert kw["elem"] == elem and kw["held_stride"] == H * D * 2 and kw.get("held_out") is None
    assert list(kw["held_in"]) == [tk.data_ptr(), tv.data_ptr(), 0, 0, 0, 0]  # only the span that ends on the tail
    conn = _fresh()
    conn.load_paged([1, 2], [0, 1], [34, 31], torch.arange(65, dtype=torch.int64), caches, stream=st, fused=True)
    (call,) = conn.lib.calls
    assert call[0] == "read_slots_ex" and call[-1]["held_in"] is None and call[-1]["elem"] == elem
    # ---- store: 34 + 5 -> 39 (held-out), 33 + 3 -> 36 (held-in), 35 + 2 -> 37 (both), 32 + 0, 20 + 1 -> 21 (only a move)
    conn = _fresh(((1, 34), (2, 33), (3, 35), (4, 32), (5, 20)))
    tails = torch.arange(2 * L * H * D, dtype=torch.float16).reshape(2, L, H, D)
    own_k, own_v = torch.zeros((L, H, D), dtype=torch.float16), torch.zeros((L, H, D), dtype=torch.float16)
    tails_v = tails + 1
    conn.requests[2].set_tail(tails, tails_v, 1)
    conn.requests[3].set_tail(own_k, own_v)
    conn._tail_ids, conn._tail_k, conn._tail_v = (9, 2), tails, tails_v
    epoch = conn._epoch
    slots = torch.arange(11, dtype=torch.int64)
    held = conn.store_paged([1, 2, 3, 4, 5], [5, 3, 2, 0, 1], slots, caches, stream=st, fused=True)
    (name, handles, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "write_slots_ex" and list(handles) == [1, 2, 3, 4, 5] and list(firsts) == [34, 33, 35, 32, 20]
    assert list(counts) == [5, 3, 2, 0, 1] and list(begins) == [0, 5, 8, 10, 10] and kw["elem"] == elem and kw["held_stride"] == H * D * 2
    row = L * H * D * 2
    k2 = conn.requests[2]
    assert list(kw["held_in"]) == [0, 0, tails.data_ptr() + row, tails_v.data_ptr() + row, own_k.data_ptr(), own_v.data_ptr(), 0, 0, 0, 0]
    nk, nv = conn._tail_k, conn._tail_v
    assert conn._tail_ids == (1, 3, 5) and tuple(nk.shape) == (3, L, H, D) and nk.dtype == torch.float16 and nv.dtype == torch.float16
    assert list(kw["held_out"]) == [nk.data_ptr(), nv.data_ptr(), 0, 0, nk.data_ptr() + row, nv.data_ptr() + row, 0, 0,
                                    nk.data_ptr() + 2 * row, nv.data_ptr() + 2 * row]
    assert [conn.length(r) for r in (1, 2, 3, 4, 5)] == [39, 36, 37, 32, 21] and conn._epoch != epoch
    assert k2._tail is None and conn.requests[4]._tail is None
    for j, rid in enumerate((1, 3, 5)):
        assert conn.requests[rid]._tail[0] is nk and conn.requests[rid]._tail[1] is nv and conn.requests[rid]._tail[2] == j
    assert any(t is own_k for t in held) and any(t is tails for t in held)     # the rows the launch read stay alive with the caller
    # a store that leaves no tail drops the batched tails its requests were part of
    conn.store_paged([1], [1], torch.arange(1, dtype=torch.int64), caches, stream=st, fused=True)
    assert conn._tail_ids == () and conn._tail_k is None and conn.length(1) == 40 and conn.requests[1]._tail is None


def test_fused_false_is_today_and_the_row_route_stays(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    good = [torch.zeros((2, NB, BS, H, D), dtype=torch.float16) for _ in range(L)]
    bf16 = [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16) for _ in range(L)]
    # fused=False: exactly the calls of today, for fp16 and for bf16 caches
    conn = _fresh()
    conn.load_paged([1, 2], [0, 1], [34, 31], torch.arange(65, dtype=torch.int64), good, stream=st, fused=False)
    conn.store_paged([1, 2], [4, 0], torch.arange(4, dtype=torch.int64), good, stream=st, fused=False)
    assert [c[0] for c in conn.lib.calls] == ["read_slots", "write_slots"] and len(conn.lib.calls[0]) == 12
    conn = _fresh()
    conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), bf16, stream=st)
    assert [c[0] for c in conn.lib.calls] == ["fetch_range"] * (2 * L)
    conn = _fresh(((2, 33),))
    for caches in (good, bf16):
        with pytest.raises(ValueError):
            conn.store_paged([2], [2], torch.arange(2, dtype=torch.int64), caches, stream=st)
    # fused=True and the row route: a K pre-scale, a dtype that is neither, strides that do not fit, mixed dtypes
    others = {
        "float32": [torch.zeros((2, NB, BS, H, D), dtype=torch.float32) for _ in range(L)],
        "strides": [torch.zeros((2, NB, BS, H, 2 * D), dtype=torch.bfloat16)[..., :D] for _ in range(L)],
        "mixed": [good[0], bf16[1]],
        "prescale": bf16,
    }
    for what, caches in others.items():
        conn = _fresh()
        if what == "prescale":
            conn._kscale = torch.ones((L, H, D), dtype=torch.float16)
            conn._kscale_inv = torch.ones((L, H, D), dtype=torch.float16)
        assert conn._paged_geometry(caches, bf16=True) is None, what
        conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), caches, stream=st, fused=True)
        assert [c[0] for c in conn.lib.calls] == ["fetch_range"] * (2 * L), what
        conn = _fresh(((2, 0),))
        if what == "prescale":
            conn._kscale = torch.ones((L, H, D), dtype=torch.float16)
            conn._kscale_inv = torch.ones((L, H, D), dtype=torch.float16)
        conn.store_paged([2], [32], torch.arange(32, dtype=torch.int64), caches, stream=st, fused=True)
        assert [c[0] for c in conn.lib.calls] == ["write_runs"] and conn.length(2) == 32, what
        conn.requests[2].length = 33
        with pytest.raises(ValueError):                                      # on the row route an odd length still raises
            conn.store_paged([2], [2], torch.arange(2, dtype=torch.int64), caches, stream=st, fused=True)


def test_the_adapter_passes_fused_only_when_asked():
    from cxl_speckv_amd.vllm_connector import SpeckvVllmConnector
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True)._fused == {}
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True, paged_fused=True)._fused == {"fused": True}
