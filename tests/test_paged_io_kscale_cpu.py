"""Not -m gpu: the K pre-scale inside the one-launch paged-cache route (speckv_ext_read_slots_kmul / speckv_ext_write_slots_kmul,
load_paged / store_paged with fused=True, kscale=True).

The one rule of include/speckv_ext.h as numpy restatements -- the pin every GPU test compares against: the exact fp32 product of a
cache or pool element and its channel's fp16 factor, rounded once to the destination's element type -- checked against torch's CPU
half multiply over all 65 536 patterns; the declarations; and what the connector hands the library, against a recording library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests.test_paged_io_cpu import _cpu_torch
from tests.test_paged_io_fused_cpu import _RecordingExLib, bf16_is_nan, bf16_to_fp16_bits, fp16_is_nan, fp16_to_bf16_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("speckv_ext_read_slots_kmul", "speckv_ext_write_slots_kmul")


# ------------------------------------------------------------------------------------------------------------------ the one rule
def _f32_to_bf16_bits(f32):
    """fp32 -> bf16 by one round-to-nearest-even; says nothing about a NaN"""
    f = np.asarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((f + 0x7FFF + ((f >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _product(bits, mul_bits, src_bf16):
    """the exact product in fp32: 11 x 11 or 8 x 11 significand bits fit its 24 (the factor is fp16 either way)"""
    bits = np.asarray(bits, dtype=np.uint16)
    x = (bits.astype(np.uint32) << 16).view(np.float32) if src_bf16 else bits.view(np.float16).astype(np.float32)
    m = np.asarray(mul_bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return x * m


def scaled_to_fp16_bits(bits, mul_bits, src_bf16=False):
    """cache element (fp16 or bf16 bits) x factor (fp16 bits) -> the fp16 bits the pool side gets: one rounding, nearest even.  Also
    pool -> fp16 cache row (src_bf16=False)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return _product(bits, mul_bits, src_bf16).astype(np.float16).view(np.uint16)


def scaled_to_bf16_bits(bits, mul_bits):
    """decoded fp16 bits x factor -> the bf16 bits of a cache row: one rounding, nearest even (a NaN: by position)"""
    return _f32_to_bf16_bits(_product(bits, mul_bits, False))


def factor_bits(layers, heads=8, dim=128, first_layer=0):
    """[layers][heads * dim] fp16 bits of powers of two that differ by layer, head and channel: exponent ((7 l + 3 h + c) % 9) - 4"""
    l, h, c = np.meshgrid(np.arange(first_layer, first_layer + layers), np.arange(heads), np.arange(dim), indexing="ij")
    return np.exp2(((7 * l + 3 * h + c) % 9) - 4).astype(np.float16).reshape(layers, heads * dim).view(np.uint16)


def wide_factor_bits(layers, heads=8, dim=128):
    """the same table with 2^-14 and 2^14 entries: products that leave fp16's range on either side"""
    f = factor_bits(layers, heads, dim).copy()
    f[:, 5::17] = np.float16(2.0 ** -14).view(np.uint16)
    f[:, 11::19] = np.float16(2.0 ** 14).view(np.uint16)
    return f


def test_the_rule_is_torchs_half_multiply_over_all_patterns_and_factors():
    import torch
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16)
    nan = fp16_is_nan(bits)
    over = under = 0
    for e in range(-14, 15):
        m = np.float16(2.0 ** e)
        mine = scaled_to_fp16_bits(bits, np.full(bits.shape, m.view(np.uint16)))
        theirs = (t * torch.tensor(float(m), dtype=torch.float16)).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(mine[~nan], theirs[~nan]) and fp16_is_nan(mine[nan]).all() and fp16_is_nan(theirs[nan]).all(), e
        finite = ~nan & ((bits & 0x7FFF) < 0x7C00)
        over += int((finite & ((mine & 0x7FFF) == 0x7C00)).sum())
        under += int((finite & ((bits & 0x7FFF) != 0) & ((mine & 0x7FFF) == 0)).sum())
        assert ((mine & 0x8000) == (bits & 0x8000))[~nan].all()              # the sign stays, of a zero too
    assert over and under                                                     # both ends of fp16's range are met
    # a factor that is no power of two: still the exact product rounded once
    m = np.float16(1.37)
    mine = scaled_to_fp16_bits(bits, np.full(bits.shape, m.view(np.uint16)))
    theirs = (t * torch.tensor(float(m), dtype=torch.float16)).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(mine[~nan], theirs[~nan])


def test_one_rounding_from_bf16_differs_from_two_only_where_the_issue_says():
    """bf16 x factor -> fp16 in one rounding against bf16 -> fp16 -> x factor: equal except where bf16 -> fp16 is itself inexact or the
    product leaves fp16's normal range -- 1064 patterns at 2^-4 and 2752 at 2^4; rows of magnitude about 1 with factors 2^-4 .. 2^4
    are therefore served bit for bit by the row route, which the connector-level GPU twins rely on."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    ok = ~bf16_is_nan(bits)
    counts = {}
    for e in (-4, 4):
        m = np.full(bits.shape, np.float16(2.0 ** e).view(np.uint16))
        one = scaled_to_fp16_bits(bits, m, src_bf16=True)
        two = scaled_to_fp16_bits(bf16_to_fp16_bits(bits), m)
        counts[e] = int((one != two)[ok].sum())
        mag = ok & (np.abs((bits.astype(np.uint32) << 16).view(np.float32)) >= 2.0 ** -6) & (np.abs((bits.astype(np.uint32) << 16).view(np.float32)) <= 64.0)
        assert np.array_equal(one[mag], two[mag])
    assert counts == {-4: 1064, 4: 2752}, counts
    # pool -> bf16: fp16 x factor -> bf16 in one rounding is no bf16(fp16(product)) everywhere either; the restatement is the former
    m = np.full(bits.shape, np.float16(2.0 ** -3).view(np.uint16))
    okh = ~fp16_is_nan(bits)
    one, two = scaled_to_bf16_bits(bits, m), fp16_to_bf16_bits(scaled_to_fp16_bits(bits, m))
    assert (one != two)[okh].any()


def test_factor_tables_differ_by_layer_head_and_channel():
    f = factor_bits(2).view(np.float16).astype(np.float32).reshape(2, 8, 128)
    assert f.min() == 2.0 ** -4 and f.max() == 2.0 ** 4
    assert (f[0] != f[1]).any() and (f[:, 0] != f[:, 1]).any() and (f[:, :, 0] != f[:, :, 1]).any()
    assert np.array_equal(factor_bits(1, first_layer=1)[0], factor_bits(2)[1])
    w = wide_factor_bits(2).view(np.float16).astype(np.float32)
    assert w.min() == 2.0 ** -14 and w.max() == 2.0 ** 14


# ------------------------------------------------------------------------------------------------------------- the declarations
def _ctypes_of(decl):
    out = []
    for arg in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","):
        arg = arg.strip()
        out.append(C.c_void_p if "*" in arg else {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}[arg.split()[0]])
    return out


def test_the_kmul_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                     # additive entries: the version stays
    c_api = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:[^}]*\bspeckv_\*;", exports)                    # the list names every speckv_* symbol
    for name in ENTRIES:
        m = re.search(r"speckv_status_t\s+%s\s*\(((?:[^()]|/\*.*?\*/)*)\);" % name, header, re.S)
        assert m and name in c_api, name
        sig = _ctypes_of(m.group(1))
        assert sig == speckv_ctypes._EXT_SIGNATURES[name], name             # the binding is the declaration
        ex = speckv_ctypes._EXT_SIGNATURES[name.replace("_kmul", "_ex")]
        assert sig == ex[:-1] + [C.c_void_p, C.c_uint64] + ex[-1:], name    # the _ex list, the factor rows and their stride, the stream
        plain = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert re.search(r"const void\* d_k_mul\s*,\s*uint64_t k_mul_layer_stride_bytes,\s*void\* stream$", plain), name
    not_built = re.search(r"Not built: capture into a HIP graph,([^*]|\*(?!/))*?2048 bytes", header)
    assert not_built and "pre-scale" not in not_built.group(0)               # the gap is no longer listed
    lib = C.CDLL(pkg.build_library())
    for name in ENTRIES:
        assert hasattr(lib, name)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    for name in ("read_slots_kmul", "write_slots_kmul"):
        assert callable(getattr(pkg.SpeckvLib, name))


def test_the_kmul_entries_on_the_null_engine_have_no_data_path():
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(2 * 4 * 2048 + 16, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        mul = np.ones(1024 + 8, dtype=np.float16)
        mat = mul.ctypes.data + (-mul.ctypes.data) % 16
        slots = np.asarray([0, 1, 2, 3], dtype=np.int64)
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        for call in (lib.read_slots_kmul, lib.write_slots_kmul):
            for k_mul in (mat, 0):
                with pytest.raises(SpeckvError) as e:
                    call(u64(h), u64(0), u64(4), u64(0), slots.ctypes.data, 4, u64(at), 0, 4 * 2048, 16, 1, elem=1, k_mul=k_mul, k_mul_stride=2048)
                assert e.value.status == -2                                  # SPECKV_ERR_DRIVER
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _RecordingKmulLib(_RecordingExLib):
    def read_slots_kmul(self, *a, **k): self.calls.append(("read_slots_kmul",) + a + (k,))
    def write_slots_kmul(self, *a, **k): self.calls.append(("write_slots_kmul",) + a + (k,))


L, H, D, T, BS, NB = 2, 8, 128, 64, 16, 6


def _fresh(lengths=((1, 34), (2, 32)), prescale=True):
    import torch
    conn = SpeckvKVConnector(_RecordingKmulLib(), L, H, D, T, "int4")
    for rid, n in lengths:
        conn.add_request(rid)
        conn.requests[rid].length = n
    if prescale:
        conn._kscale = torch.full((L, H, D), 2.0, dtype=torch.float16)
        conn._kscale_inv = torch.full((L, H, D), 0.5, dtype=torch.float16)
    return conn


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_kscale_calls_for_even_and_odd_lengths(monkeypatch, dtype):
    """with the keyword and a pre-scale: exactly one _kmul call each way -- the _ex call's arguments, the factor pointer (_kscale on a
    load, _kscale_inv on a store) and its layer stride, held rows for odd lengths"""
    torch, st = _cpu_torch(monkeypatch)
    dt = getattr(torch, dtype)
    elem = 1 if dtype == "bfloat16" else 0
    caches = [torch.zeros((2, NB + 2, BS, H, D), dtype=dt)[:, 1:-1] for _ in range(L)]
    conn = _fresh(((1, 35), (2, 32)))
    assert conn._paged_geometry(caches, bf16=True) is None and conn._paged_geometry(caches) is None      # the answers of before
    assert conn._paged_geometry(caches, bf16=True, kscale=True) == (NB * BS, caches[0].stride(0) * 2, elem)
    tk, tv = torch.ones((1, L, H, D), dtype=torch.float16), torch.ones((1, L, H, D), dtype=torch.float16)
    conn.requests[1].set_tail(tk, tv, 0)
    slots = torch.arange(5 + 31 + 4, dtype=torch.int64)
    conn.load_paged([1, 2, 1], [30, 1, 30], [5, 31, 4], slots, caches, stream=st, fused=True, kscale=True)
    (name, handles, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "read_slots_kmul" and list(handles) == [1, 2, 1] and list(firsts) == [30, 1, 30] and list(counts) == [5, 31, 4]
    assert list(begins) == [0, 5, 36] and d_slots == slots.data_ptr() and n_slots == NB * BS and list(bases) == [c.data_ptr() for c in caches]
    assert layer_begin == 0 and kind_stride == caches[0].stride(0) * 2 and step == T // 2 and stream == st.cuda_stream
    assert kw["elem"] == elem and kw["held_stride"] == H * D * 2 and kw.get("held_out") is None
    assert list(kw["held_in"]) == [tk.data_ptr(), tv.data_ptr(), 0, 0, 0, 0]
    assert kw["k_mul"] == conn._kscale.data_ptr() and kw["k_mul_stride"] == H * D * 2
    # ---- store: 34 + 5 -> 39 (held-out), 33 + 3 -> 36 (held-in), 35 + 2 -> 37 (both), 32 + 0, 20 + 1 -> 21 (only a move)
    conn = _fresh(((1, 34), (2, 33), (3, 35), (4, 32), (5, 20)))
    tails = torch.arange(2 * L * H * D, dtype=torch.float16).reshape(2, L, H, D)
    tails_v = tails + 1
    own_k, own_v = torch.zeros((L, H, D), dtype=torch.float16), torch.zeros((L, H, D), dtype=torch.float16)
    conn.requests[2].set_tail(tails, tails_v, 1)
    conn.requests[3].set_tail(own_k, own_v)
    held = conn.store_paged([1, 2, 3, 4, 5], [5, 3, 2, 0, 1], torch.arange(11, dtype=torch.int64), caches, stream=st, fused=True, kscale=True)
    (name, handles, firsts, counts, begins, d_slots, n_slots, bases, layer_begin, kind_stride, step, stream, kw), = conn.lib.calls
    assert name == "write_slots_kmul" and list(handles) == [1, 2, 3, 4, 5] and list(firsts) == [34, 33, 35, 32, 20]
    assert list(counts) == [5, 3, 2, 0, 1] and list(begins) == [0, 5, 8, 10, 10] and kw["elem"] == elem and kw["held_stride"] == H * D * 2
    assert kw["k_mul"] == conn._kscale_inv.data_ptr() and kw["k_mul_stride"] == H * D * 2
    row = L * H * D * 2
    assert list(kw["held_in"]) == [0, 0, tails.data_ptr() + row, tails_v.data_ptr() + row, own_k.data_ptr(), own_v.data_ptr(), 0, 0, 0, 0]
    nk, nv = conn._tail_k, conn._tail_v
    assert conn._tail_ids == (1, 3, 5) and tuple(nk.shape) == (3, L, H, D) and nk.dtype == torch.float16
    assert list(kw["held_out"]) == [nk.data_ptr(), nv.data_ptr(), 0, 0, nk.data_ptr() + row, nv.data_ptr() + row, 0, 0,
                                    nk.data_ptr() + 2 * row, nv.data_ptr() + 2 * row]
    assert [conn.length(r) for r in (1, 2, 3, 4, 5)] == [39, 36, 37, 32, 21]
    assert any(t is own_k for t in held) and any(t is tails for t in held)


def test_without_the_keyword_or_without_a_prescale_the_calls_are_those_of_before(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    bf16 = [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16) for _ in range(L)]
    # a pre-scale without the keyword: the row route, fused or not
    for fused in (False, True):
        conn = _fresh()
        conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), bf16, stream=st, fused=fused)
        assert [c[0] for c in conn.lib.calls] == ["fetch_range"] * (2 * L), fused
        conn = _fresh(((2, 0),))
        conn.store_paged([2], [32], torch.arange(32, dtype=torch.int64), bf16, stream=st, fused=fused)
        assert [c[0] for c in conn.lib.calls] == ["write_runs"] and conn.length(2) == 32, fused
        conn.requests[2].length = 33
        with pytest.raises(ValueError):
            conn.store_paged([2], [2], torch.arange(2, dtype=torch.int64), bf16, stream=st, fused=fused)
    # the keyword without fused=True means nothing
    conn = _fresh()
    conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), bf16, stream=st, kscale=True)
    assert [c[0] for c in conn.lib.calls] == ["fetch_range"] * (2 * L)
    # no pre-scale: the keyword gives the fused=True call, argument for argument
    both = []
    for kw in (dict(fused=True), dict(fused=True, kscale=True)):
        conn = _fresh(((1, 35), (2, 32)), prescale=False)
        tk, tv = torch.ones((1, L, H, D), dtype=torch.float16), torch.ones((1, L, H, D), dtype=torch.float16)
        conn.requests[1].set_tail(tk, tv, 0)
        slots = torch.arange(40, dtype=torch.int64)
        conn.load_paged([1, 2], [30, 1], [5, 31], slots[:36], bf16, stream=st, **kw)
        conn.store_paged([2], [3], slots[:3], bf16, stream=st, **kw)
        assert [c[0] for c in conn.lib.calls] == ["read_slots_ex", "write_slots_ex"]
        assert all("k_mul" not in c[-1] for c in conn.lib.calls)
        both.append([(c[0], [list(x) if hasattr(x, "__len__") else x for x in c[1:5]], c[-1]["elem"]) for c in conn.lib.calls])
    assert both[0] == both[1]


def test_caches_that_do_not_fit_still_take_the_row_route(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    good = [torch.zeros((2, NB, BS, H, D), dtype=torch.float16) for _ in range(L)]
    bf16 = [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16) for _ in range(L)]
    others = {
        "float32": [torch.zeros((2, NB, BS, H, D), dtype=torch.float32) for _ in range(L)],
        "strides": [torch.zeros((2, NB, BS, H, 2 * D), dtype=torch.bfloat16)[..., :D] for _ in range(L)],
        "mixed": [good[0], bf16[1]],
    }
    for what, caches in others.items():
        conn = _fresh()
        assert conn._paged_geometry(caches, bf16=True, kscale=True) is None, what
        conn.load_paged([2], [0], [32], torch.arange(32, dtype=torch.int64), caches, stream=st, fused=True, kscale=True)
        assert [c[0] for c in conn.lib.calls] == ["fetch_range"] * (2 * L), what
        conn = _fresh(((2, 0),))
        conn.store_paged([2], [32], torch.arange(32, dtype=torch.int64), caches, stream=st, fused=True, kscale=True)
        assert [c[0] for c in conn.lib.calls] == ["write_runs"] and conn.length(2) == 32, what
        conn.requests[2].length = 33
        with pytest.raises(ValueError):                                      # on the row route an odd length still raises
            conn.store_paged([2], [2], torch.arange(2, dtype=torch.int64), caches, stream=st, fused=True, kscale=True)


def test_the_adapter_passes_kscale_only_on_top_of_fused():
    from cxl_speckv_amd.vllm_connector import SpeckvVllmConnector
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True, paged_fused=True, paged_kscale=True)._fused == {"fused": True, "kscale": True}
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True, paged_kscale=True)._fused == {}
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True, paged_fused=True)._fused == {"fused": True}
    assert SpeckvVllmConnector(None, num_layers=2, paged_io=True)._fused == {}
