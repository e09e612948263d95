"""-m gpu: the K pre-scale inside the one-launch paged-cache route -- speckv_ext_read_slots_kmul / speckv_ext_write_slots_kmul,
load_paged / store_paged with fused=True, kscale=True and SpeckvVllmConnector(paged_io=True, paged_fused=True, paged_kscale=True).

References: the numpy restatement of the one rule (tests/test_paged_io_kscale_cpu.py: the exact fp32 product of an element and its
channel's fp16 factor, rounded once to the destination's element type) applied to speckv_ext_fetch_range's image for a read, and to
the rows a twin allocation gets by speckv_ext_write_runs for a write; never a device multiply.  Every comparison is exact; of a NaN
only the position is compared.  The factor tables differ by layer, head and channel (a wrong index or layer changes bits), one of
them with 2^-14 and 2^14 entries; the K and V planes of the entry tests hold the same data, so V shows what K would be unscaled.
Geometry and helpers are those of tests/test_gpu_paged_io.py and tests/test_gpu_paged_io_fused.py (L = 2, T = 128, blocks of 16
slots, 12 blocks, caches between guard blocks, n_slots one block short, everything pre-filled with a pattern and compared whole).
Connector-level twins are the row route of a connector with the same pre-scale: with fp16 caches its bits are the rule's for any
data; with bf16 caches for rows of magnitude about 1 and factors 2^-4 .. 2^4 (the CPU file counts where the two part)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, dev_to_host, graph_capture, set_tuning, stored_record, torch_mod
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_paged_io import (BS, L, N_PAGES, N_SLOTS, NB, PAGE, ROOT, ROW, SPANS, STEP, T, _all_rows, _bases, _bits, _blocks, _caches,
                                     _Counting, _dev, _fill, _host, _image, _kind_stride, _random_content, _row, _span_args, u64)
from tests.test_paged_io_fused_cpu import bf16_is_nan, bf16_to_fp16_bits, equal_off_nan, fp16_is_nan, fp16_to_bf16_bits
from tests.test_paged_io_kscale_cpu import factor_bits, scaled_to_bf16_bits, scaled_to_fp16_bits, wide_factor_bits

pytestmark = pytest.mark.gpu
FP16, BF16 = 0, 1
HALF = ROW // 2                                 # elements of a row


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _to_cache(rows, elem):
    """what a cache of element type `elem` holds for the pool's fp16 bits `rows`, unscaled (V)"""
    return fp16_to_bf16_bits(rows) if elem == BF16 else rows


def _from_cache(rows, elem):
    """the fp16 bits the pool encodes for a cache row, unscaled (V)"""
    return bf16_to_fp16_bits(rows) if elem == BF16 else rows


def _k_to_cache(rows, mul, elem):
    """pool-side fp16 bits of K x factor row -> the bits of a cache row: one rounding"""
    return scaled_to_bf16_bits(rows, mul) if elem == BF16 else scaled_to_fp16_bits(rows, mul)


def _k_from_cache(rows, mul, elem):
    """cache bits of K x factor row -> pool-side fp16 bits: one rounding"""
    return scaled_to_fp16_bits(rows, mul, src_bf16=elem == BF16)


def _pool_side(flat, mul, elem):
    """[L][2][slots][1024] cache bits -> the fp16 bits the pool side gets: K scaled by its layer's factor row, V converted"""
    out = np.empty(flat.shape, dtype=np.uint16)
    for layer in range(flat.shape[0]):
        out[layer, 0] = _k_from_cache(flat[layer, 0], mul[layer][None], elem)
        out[layer, 1] = _from_cache(flat[layer, 1], elem)
    return out


def _nan_of(bits, elem):
    return bf16_is_nan(bits) if elem == BF16 else fp16_is_nan(bits)


def _same(got, want, nan, elem_out):
    return equal_off_nan(got, want, nan, bf16_is_nan if elem_out == BF16 else fp16_is_nan)


def _factors(torch, bits):
    """[n][1024] fp16 factor bits on the device, between two guard rows: returns (tensor, address of row 0, host copy with guards)"""
    host = np.concatenate([np.full((1, HALF), 0x7A11, dtype=np.uint16), bits, np.full((1, HALF), 0x7A11, dtype=np.uint16)])
    t = torch.from_numpy(host.view(np.int16).copy()).cuda()
    return t, t.data_ptr() + ROW, host


def _inverse(bits):
    return (np.float32(1.0) / bits.view(np.float16).astype(np.float32)).astype(np.float16).view(np.uint16)


def _held_block(torch, n, seed=None):
    """[n + 2][L][1024] fp16 rows between two guard rows: random (seed) or the pattern; returns (tensor, host copy)"""
    if seed is None:
        host = np.full((n + 2, L, HALF), 0x7A11, dtype=np.uint16)
    else:
        host = np.random.default_rng(seed).standard_normal((n + 2, L, HALF)).astype(np.float16).view(np.uint16)
    return torch.from_numpy(host.view(np.int16).copy()).cuda(), host


def _held_ptrs(block, which, n_spans):
    """the [n_spans][2] address array for (K block, V block): span i's rows at index 1 + i where which[i]"""
    k, v = block
    step = L * ROW
    out = np.zeros(2 * n_spans, dtype=np.uint64)
    for i in range(n_spans):
        if which[i]:
            out[2 * i], out[2 * i + 1] = k.data_ptr() + (1 + i) * step, v.data_ptr() + (1 + i) * step
    return out


def _as_bf16(content):
    """fp16 cache bits -> bf16 bits of the same values truncated (exact in fp16 again)"""
    return (content.view(np.float16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------- read_kmul
ALL_SPAN = (2, 0, 64)                           # the positions of allocation 2 whose region 0 holds all 65 536 fp16 patterns


def _patterns_alloc(lib, seed):
    """an allocation like _fill's, its hole at page 40, whose pages 0 .. 31 of region 0 (layer 0, K) hold every fp16 pattern"""
    x = _blocks(N_PAGES, seed)
    x[:32] = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(32, ROW)
    h = lib.alloc(N_PAGES * PAGE)
    _fill(lib, h, x, hole=40)
    return h


def _expect_read(want, nan, images, spans, bs, slots, mul, elem, layers=range(L), held=None):
    """fill `want` / `nan` ([L][2][slots][1024] of the big tensors) with what a read_slots_kmul of `spans` leaves; held: (has, K host
    block, V host block) -- span i's last position from row 1 + i of the held blocks where has[i].  mul[l] = the factor row the
    call hands layer layers[l]"""
    for i, ((a, first, n), b) in enumerate(zip(spans, bs)):
        for t in range(n):
            s = int(slots[int(b) + t])
            if 0 <= s < N_SLOTS:
                for li, layer in enumerate(layers):
                    for kind in (0, 1):
                        row = _row(images[a], layer, kind, first + t)
                        if held is not None and held[0][i] and t == n - 1:
                            row = held[1 + kind][1 + i, li]
                        want[layer, kind, BS + s] = _k_to_cache(row, mul[li], elem) if kind == 0 else _to_cache(row, elem)
                        nan[layer, kind, BS + s] = fp16_is_nan(row)


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_read_kmul_is_the_restatement_of_fetch_range(scheme, mode, elem):
    """Spans [0, 34), [5, 32), [33, 34), [64, 64) with two -1 slots and one >= n_slots, and [0, 64) of the allocation whose first
    region holds every fp16 pattern, both wave orders, the factor table with 2^-14 and 2^14 entries: the caches, guards included, are
    fetch_range's image x factor rounded once for K and the _ex entry's bits for V."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
        for i, h in enumerate(handles):
            _fill(lib, h, _blocks(N_PAGES, 300 + 10 * scheme + i))
        handles.append(_patterns_alloc(lib, 333 + scheme))
        st = torch.cuda.Stream()
        images = [_image(lib, torch, h, st) for h in handles]
        if scheme == 0:
            assert len(np.unique(images[2][:32])) == 65536
        spans = SPANS + [ALL_SPAN]
        listed = sum(n for _, _, n in SPANS)
        slots = np.random.default_rng(5).permutation(N_SLOTS)[:listed + ALL_SPAN[2]].astype(np.int64)
        slots[[3, listed - 2]] = -1
        slots[listed // 2] = N_SLOTS + 3
        d_slots = torch.from_numpy(slots).cuda()
        hs, fs, ns, bs = _span_args(handles, spans)
        mul = wide_factor_bits(L)
        d_mul, p_mul, mul_host = _factors(torch, mul)
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches, plain = _caches(torch), _caches(torch)
            want = _host(caches)
            nan = np.zeros(want.shape, dtype=bool)
            _expect_read(want, nan, images, spans, bs, slots, mul, elem)
            before = lib.stats()
            torch.cuda.synchronize()
            lib.read_slots_kmul(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                                elem=elem, k_mul=p_mul, k_mul_stride=ROW)
            st.synchronize()
            got = _host(caches)
            assert _same(got, want, nan, elem), (scheme, mode, elem, kind_fast, np.argwhere(((got != want) & ~nan).any(axis=-1))[:8])
            pages = 2 * L * sum((f + n + 1) // 2 - f // 2 for _, f, n in spans if n)
            assert lib.stats().total_decompressions - before.total_decompressions == pages
            lib.read_slots_ex(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(plain), 0, _kind_stride(plain), STEP, st.cuda_stream, elem=elem)
            st.synchronize()
            ex = _host(plain)
            assert _same(got[:, 1], ex[:, 1], nan[:, 1], elem), "V is not the _ex entry's"
            assert (got[:, 0] != ex[:, 0]).any(), "K shows no factor"
        assert np.array_equal(d_mul.cpu().numpy().view(np.uint16), mul_host)
        if scheme == 0:                                                      # the products leave fp16's range on both sides
            k = want[0, 0][(want[0, 0] != 0x7C5A).any(axis=-1)]
            assert nan.any() and (k == 0).any()
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ write_kmul
def _plane_content(seed, elem):
    """[L][2][NB + 2][BS][1024] cache bits of type `elem`, the K and V planes alike: random rows everywhere; slots 0 .. 63 hold every
    pattern of the type; slots 64 .. 71 a page of zeros, a page of constant runs, a page with inf and NaN in random rows, a page of
    -0 and of the smallest values"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((L, 1, NB + 2, BS, HALF)).astype(np.float32)
    c = (x.view(np.uint32) >> 16).astype(np.uint16) if elem == BF16 else x.astype(np.float16).view(np.uint16)
    flat = c.reshape(L, 1, (NB + 2) * BS, HALF)
    flat[:, :, BS:BS + 64] = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(64, HALF)
    flat[:, :, BS + 64:BS + 66] = 0
    flat[:, :, BS + 66] = np.repeat(flat[:, :, BS + 66, :32], 32, axis=-1)
    flat[:, :, BS + 67] = flat[:, :, BS + 67, :1]
    special = (0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81) if elem == BF16 else (0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01)      # +-inf, NaNs
    for k, bits in enumerate(special):
        flat[:, :, BS + 68, 17 + 97 * k] = bits
        flat[:, :, BS + 69, 1000 - 31 * k] = bits
    flat[:, :, BS + 70] = 0x8000
    flat[:, :, BS + 71] = 0x3080 if elem == BF16 else 0x0001                   # 2^-30 / 2^-24: only a large factor keeps them
    return np.ascontiguousarray(np.repeat(c, 2, axis=1))


WRITE_SPANS = [(0, 0, 64), (1, 6, 26), (0, 64, 8)]


def _twin_runs(lib, torch, twin, first_pos, rows16, stream, keep, layers=range(L)):
    """write_runs of rows16 [layers][2][n][1024] fp16 bits (n even) at position first_pos (even) of allocation `twin`"""
    n = rows16.shape[2]
    assert n % 2 == 0 and first_pos % 2 == 0
    d = torch.from_numpy(np.ascontiguousarray(rows16).view(np.int16)).cuda()
    keep.append(d)
    firsts = [(2 * layer + kind) * STEP + first_pos // 2 for layer in layers for kind in (0, 1)]
    srcs = [d.data_ptr() + (li * 2 + kind) * n * ROW for li in range(len(layers)) for kind in (0, 1)]
    torch.cuda.synchronize()
    lib.write_runs(twin, firsts, srcs, n // 2, stream.cuda_stream)
    stream.synchronize()


def _compare_allocations(lib, torch, h, tw, scheme, st, what):
    """decoded bits, rec_bytes, scale and stored record bytes of every page; the FP16 scheme stores the product itself, so there a
    NaN of the twin is a NaN here and nothing more"""
    got, want = _image(lib, torch, h, st), _image(lib, torch, tw, st)
    nan = fp16_is_nan(want) if scheme == 0 else np.zeros(want.shape, dtype=bool)
    assert _same(got, want, nan, FP16), (what, "decoded bits", np.argwhere(((got != want) & ~nan).any(axis=-1))[:8])
    for p in range(N_PAGES):
        a, b = lib.translate(h, p * PAGE), lib.translate(tw, p * PAGE)
        assert a.rec_bytes == b.rec_bytes, (what, p, a.rec_bytes, b.rec_bytes)
        if scheme != 5:
            assert np.float32(a.scale).view(np.uint32) == np.float32(b.scale).view(np.uint32), (what, p)
        if a.rec_bytes:
            ra, rb = stored_record(a, a.rec_bytes), stored_record(b, b.rec_bytes)
            if scheme == 0:
                ra, rb = ra.view(np.uint16), rb.view(np.uint16)
                assert equal_off_nan(ra, rb, fp16_is_nan(rb), fp16_is_nan), (what, p, "record bytes")
            else:
                assert np.array_equal(ra, rb), (what, p, "record bytes")
    return got


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_write_kmul_is_write_runs_of_the_restated_rows(scheme, mode, elem):
    """caches whose K and V planes hold the same random rows, every pattern of their element type, zeros, constant runs, -0, inf and
    NaN, and values the factor pushes over 65504 or under 2^-24: rec_bytes, scale, record bytes and decoded bits are those of twins
    written by write_runs from the restated rows (K x factor in one rounding, V converted) laid contiguous; both wave orders; -1 slots
    and one >= n_slots store the record of a zero row; the V records are the unscaled ones; the caches are unchanged."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        content = _plane_content(50 + scheme, elem)
        flat = content.reshape(L, 2, (NB + 2) * BS, HALF)
        mul = wide_factor_bits(L)
        flat16 = _pool_side(flat, mul, elem)
        plain16 = _from_cache(flat[:, 1], elem)
        finite = ~_nan_of(flat[:, 0], elem) & ((flat[:, 0] & 0x7FFF) < (0x7F80 if elem == BF16 else 0x7C00))
        assert (finite & ((flat16[:, 0] & 0x7FFF) == 0x7C00)).any() and (finite & ((flat[:, 0] & 0x7FFF) != 0) & ((flat16[:, 0] & 0x7FFF) == 0)).any()
        assert fp16_is_nan(flat16[:, 0, BS + 68]).any() and (flat16[:, 0, BS + 70] == 0x8000).all() and (flat16[:, 0, BS + 71] != 0).any()
        d_mul, p_mul, mul_host = _factors(torch, mul)
        rng = np.random.default_rng(7)
        slots = np.concatenate([np.arange(64), 72 + rng.permutation(N_SLOTS - 72)[:26], np.arange(64, 72)]).astype(np.int64)
        slots[[64 + 7, 64 + 13]] = -1
        slots[64 + 20] = N_SLOTS + 1
        d_slots = torch.from_numpy(slots).cuda()
        st = torch.cuda.Stream()
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _caches(torch, content)
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            twins = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            hs, fs, ns, bs = _span_args(handles, WRITE_SPANS)
            before = lib.stats().total_compressions
            torch.cuda.synchronize()
            lib.write_slots_kmul(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                                 elem=elem, k_mul=p_mul, k_mul_stride=ROW)
            st.synchronize()
            assert lib.stats().total_compressions - before == 2 * L * sum(n // 2 for _, _, n in WRITE_SPANS)
            assert np.array_equal(_host(caches).reshape(content.shape), content), "write_slots_kmul changed the caches"
            keep = []
            for (a, first, n), b in zip(WRITE_SPANS, bs):
                rows = np.zeros((L, 2, n, HALF), dtype=np.uint16)
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        rows[:, :, t] = flat16[:, :, BS + s]
                _twin_runs(lib, torch, twins[a], first, rows, st, keep)
            for h, tw in zip(handles, twins):
                _compare_allocations(lib, torch, h, tw, scheme, st, (scheme, mode, elem, kind_fast))
            got = _image(lib, torch, handles[0], st)
            if scheme == 0:                                                 # the records show the product and the conversion themselves
                for i in range(64):
                    for layer in range(L):
                        for kind, want in ((0, flat16[layer, 0, BS + i]), (1, plain16[layer, BS + i])):
                            assert equal_off_nan(_row(got, layer, kind, i), want, fp16_is_nan(want), fp16_is_nan), (i, layer, kind)
            # K is scaled, V is not: rows 15 and 47 hold the patterns 0x3C00 .. 0x3FFF and 0xBC00 .. 0xBFFF, about +-1 in either type
            assert all((_row(got, layer, 0, i) != _row(got, layer, 1, i)).any() for layer in range(L) for i in (15, 47))
            image = _image(lib, torch, handles[1], st)
            for layer in range(L):
                for kind in (0, 1):
                    for t in (7, 13, 20):
                        assert not _row(image, layer, kind, 6 + t).any()
            assert image[3].any() and not image[STEP - 1].any()
            for h in handles + twins:
                lib.free(h)
        assert np.array_equal(d_mul.cpu().numpy().view(np.uint16), mul_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("scheme", [3, 5])
def test_layer_begin_1_takes_its_factor_row_relative_to_layer_begin(scheme, elem):
    """layer_begin = 1, n_layers = 1 with layer 1's factor row alone: the row at d_k_mul + 0 is layer 1's, layer 0's cache and regions
    stay as they were -- write against a write_runs twin, then read back"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        st = torch.cuda.Stream()
        content = _random_content(77)
        if elem == BF16:
            content = _as_bf16(content)
        flat = content.reshape(L, 2, (NB + 2) * BS, HALF)
        inv = factor_bits(1, first_layer=1)
        assert np.array_equal(inv[0], factor_bits(L)[1]) and not np.array_equal(inv[0], factor_bits(L)[0])
        mul = _inverse(inv)
        (d_inv, p_inv, _), (d_mul, p_mul, _) = _factors(torch, inv), _factors(torch, mul)
        caches = _caches(torch, content)
        h, tw = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
        slots = np.random.default_rng(9).permutation(N_SLOTS)[:12].astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        torch.cuda.synchronize()
        lib.write_slots_kmul(u64(h), u64(4), u64(12), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches[1:]), 1, _kind_stride(caches), STEP,
                             st.cuda_stream, elem=elem, k_mul=p_inv, k_mul_stride=ROW)
        st.synchronize()
        rows = np.stack([_k_from_cache(flat[1, 0, BS + slots], inv, elem), _from_cache(flat[1, 1, BS + slots], elem)])[None]
        _twin_runs(lib, torch, tw, 4, rows, st, [], layers=[1])
        image = _compare_allocations(lib, torch, h, tw, scheme, st, (scheme, elem, "layer_begin = 1"))
        assert not image[:2 * STEP].any() and image[2 * STEP + 2].any()
        dst = _caches(torch)
        want = _host(dst)
        nan = np.zeros(want.shape, dtype=bool)
        out_slots = np.arange(20, 32, dtype=np.int64)
        _expect_read(want, nan, [image], [(0, 4, 12)], [0], out_slots, mul, elem, layers=[1])
        torch.cuda.synchronize()
        lib.read_slots_kmul(u64(h), u64(4), u64(12), u64(0), torch.from_numpy(out_slots).cuda().data_ptr(), N_SLOTS, _bases(dst[1:]), 1,
                            _kind_stride(dst), STEP, st.cuda_stream, elem=elem, k_mul=p_mul, k_mul_stride=ROW)
        st.synchronize()
        got = _host(dst)
        assert np.array_equal(got, want) and (got[0] == 0x7C5A).all() and (got[1, 0, BS + 20] != 0x7C5A).any()
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------------------------------------------- NULL factor
@pytest.mark.parametrize("scheme", [2, 5])
def test_a_null_factor_is_the_ex_entry(scheme):
    """d_k_mul = NULL (a stride that would be refused with it): caches, held-out rows, pool records and stats equal those of
    speckv_ext_read_slots_ex / _write_slots_ex, bf16 caches and held rows included"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        st = torch.cuda.Stream()
        content = _as_bf16(_random_content(21))
        src = _caches(torch, content)
        spans = [(0, 0, 34), (1, 7, 26), (0, 40, 2)]                          # the second: held-in, and 33 is odd: held-out
        slots = np.random.default_rng(2).permutation(N_SLOTS)[:62].astype(np.int64)
        slots[[5, 40]] = -1, N_SLOTS + 2
        d_slots = torch.from_numpy(slots).cuda()
        (ik, _), (iv, _) = _held_block(torch, 3, 70), _held_block(torch, 3, 71)
        h_in = _held_ptrs((ik, iv), [False, True, False], 3)
        sides, deltas, outs = [], [], []
        for entry, extra in ((lib.write_slots_ex, {}), (lib.write_slots_kmul, dict(k_mul=0, k_mul_stride=8))):
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            (ok, _), (ov, _) = _held_block(torch, 3), _held_block(torch, 3)
            hs, fs, ns, bs = _span_args(handles, spans)
            before = lib.stats()
            torch.cuda.synchronize()
            entry(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(src), 0, _kind_stride(src), STEP, st.cuda_stream, elem=BF16, held_in=h_in,
                  held_stride=ROW, held_out=_held_ptrs((ok, ov), [False, True, False], 3), **extra)
            st.synchronize()
            after = lib.stats()
            deltas.append((after.total_compressions - before.total_compressions, after.original_bytes - before.original_bytes))
            sides.append(handles)
            outs.append((ok.cpu().numpy(), ov.cpu().numpy()))
        assert deltas[0] == deltas[1] and deltas[0][0] == 2 * L * (17 + 13 + 1)
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        for h, tw in zip(*sides):
            _compare_allocations(lib, torch, h, tw, scheme, st, "write_slots_kmul without a factor")
        rslots = np.random.default_rng(3).permutation(N_SLOTS)[:63].astype(np.int64)
        rslots[[3, 60, 31]] = -1, -1, N_SLOTS + 3
        d_r = torch.from_numpy(rslots).cuda()
        rspans = [(0, 0, 35), (1, 5, 27), (2, 33, 1), (0, 64, 0)]            # the first ends on a held row
        hs, fs, ns, bs = _span_args(sides[0] + [sides[1][0]], rspans)
        r_in = _held_ptrs((ik, iv), [True, False, False, False], 4)
        outs, deltas = [], []
        for entry, extra in ((lib.read_slots_ex, {}), (lib.read_slots_kmul, dict(k_mul=0, k_mul_stride=8))):
            dst = _caches(torch)
            before = lib.stats()
            torch.cuda.synchronize()
            entry(hs, fs, ns, bs, d_r.data_ptr(), N_SLOTS, _bases(dst), 0, _kind_stride(dst), STEP, st.cuda_stream, elem=BF16, held_in=r_in,
                  held_stride=ROW, **extra)
            st.synchronize()
            after = lib.stats()
            deltas.append((after.total_decompressions - before.total_decompressions, after.dma_completed - before.dma_completed,
                           after.dma_submitted - before.dma_submitted))
            outs.append(_host(dst))
        assert deltas[0] == deltas[1] and np.array_equal(outs[0], outs[1]) and (outs[0] != 0x7C5A).any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ held rows
@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("scheme", [2, 3, 5])
def test_read_kmul_scales_the_held_k_row_into_its_slot(scheme, elem):
    """spans that end on a held position -- [0, 35), [32, 33) (n = 1) and [40, 43) whose held position has slot -1 -- beside [5, 32)
    and [64, 64) without one: the held K rows arrive in their slots scaled, the V rows as the _ex entry leaves them, everything else
    is the restated image, the held rows and everything else keep their bits"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        handles = [lib.alloc(N_PAGES * PAGE) for _ in range(3)]
        for i, h in enumerate(handles):
            _fill(lib, h, _blocks(N_PAGES, 500 + i))
        st = torch.cuda.Stream()
        images = [_image(lib, torch, h, st) for h in handles]
        spans = [(0, 0, 35), (1, 5, 27), (2, 32, 1), (0, 40, 3), (1, 64, 0)]
        has = [True, False, True, True, False]
        hs, fs, ns, bs = _span_args(handles, spans)
        slots = np.random.default_rng(8).permutation(N_SLOTS)[:66].astype(np.int64)
        slots[[3, 50]] = -1
        slots[20] = N_SLOTS + 3
        slots[int(bs[3]) + 2] = -1                                            # the held position of [40, 43) has no row
        d_slots = torch.from_numpy(slots).cuda()
        (hk, hk_host), (hv, hv_host) = _held_block(torch, len(spans), 90), _held_block(torch, len(spans), 91)
        held = _held_ptrs((hk, hv), has, len(spans))
        mul = factor_bits(L)
        d_mul, p_mul, _ = _factors(torch, mul)
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _caches(torch)
            want = _host(caches)
            nan = np.zeros(want.shape, dtype=bool)
            _expect_read(want, nan, images, spans, bs, slots, mul, elem, held=(has, hk_host, hv_host))
            before = lib.stats().total_decompressions
            torch.cuda.synchronize()
            lib.read_slots_kmul(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                                elem=elem, held_in=held, held_stride=ROW, k_mul=p_mul, k_mul_stride=ROW)
            st.synchronize()
            got = _host(caches)
            assert np.array_equal(got, want), (scheme, elem, kind_fast, np.argwhere((got != want).any(axis=-1))[:8])
            assert lib.stats().total_decompressions - before == 2 * L * (17 + 14 + 0 + 1)
            s34 = BS + int(slots[34])                                       # position 34 of span 0: its held row, K scaled and V not
            assert np.array_equal(got[1, 0, s34], _k_to_cache(hk_host[1, 1], mul[1], elem)) and np.array_equal(got[1, 1, s34], _to_cache(hv_host[1, 1], elem))
        assert np.array_equal(hk.cpu().numpy().view(np.uint16), hk_host) and np.array_equal(hv.cpu().numpy().view(np.uint16), hv_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


#              (allocation, first, n, held-in, held-out)
HELD_WRITES = [(0, 5, 5, True, False),           # odd first, even end: pairs 2 .. 4, position 4 held in
               (0, 20, 7, False, True),          # even first, odd end: pairs 10 .. 12, position 26 held out
               (1, 3, 4, True, True),            # odd, odd: pairs 1, 2; 2 held in, 6 held out
               (1, 11, 1, True, False),          # first odd, n = 1: pair 5 from a held row and one cache row
               (1, 30, 1, False, True),          # first even, n = 1: only a row into the held-out block (its slot is -1: zeros)
               (0, 40, 6, False, False),         # no held rows
               (1, 64, 0, False, False)]         # empty


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_write_kmul_with_held_rows_in_one_call(scheme, elem):
    """every odd edge in one call, from fp16 and from bf16 caches: a held-in K row is encoded as it is (pool-side already), a cache K
    row scaled, a held-out K row is the scaled cache row as fp16, V rows go as the _ex entry moves them; the pool equals twins written
    by write_runs from the same positions; everything around the held rows, the held-in rows and the caches keep their bits"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        st = torch.cuda.Stream()
        content = _random_content(60 + scheme)
        if elem == BF16:
            content = _as_bf16(content)
            content[0, :, 5, 2, 100:104] = (0x7F80, 0x7FC0, 0xFF80, 0x0001)      # a bf16 row with inf / NaN beside a held fp16 row
        mul = factor_bits(L)
        flat16 = _pool_side(content.reshape(L, 2, (NB + 2) * BS, HALF), mul, elem)
        d_mul, p_mul, _ = _factors(torch, mul)
        spans = [(a, f, n) for a, f, n, _, _ in HELD_WRITES]
        n_spans = len(spans)
        total = sum(n for _, _, n in spans)
        slots = np.random.default_rng(12).permutation(N_SLOTS)[:total].astype(np.int64)
        begins = np.cumsum([0] + [n for _, _, n in spans])[:-1]
        slots[int(begins[2]) + 1] = 4 * BS + 2                                   # the special row: block 5 of the tensor is block 4 of the view
        slots[int(begins[4])] = -1
        slots[int(begins[5]) + 2] = -1
        d_slots = torch.from_numpy(slots).cuda()
        (ik, ik_host), (iv, iv_host) = _held_block(torch, n_spans, 70), _held_block(torch, n_spans, 71)
        h_in = _held_ptrs((ik, iv), [x[3] for x in HELD_WRITES], n_spans)
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _caches(torch, content)
            (ok, ok_host), (ov, ov_host) = _held_block(torch, n_spans), _held_block(torch, n_spans)
            h_out = _held_ptrs((ok, ov), [x[4] for x in HELD_WRITES], n_spans)
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            twins = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            hs, fs, ns, bs = _span_args(handles, spans)
            before = lib.stats().total_compressions
            torch.cuda.synchronize()
            lib.write_slots_kmul(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                                 elem=elem, held_in=h_in, held_stride=ROW, held_out=h_out, k_mul=p_mul, k_mul_stride=ROW)
            st.synchronize()
            assert lib.stats().total_compressions - before == 2 * L * (3 + 3 + 2 + 1 + 0 + 3 + 0)
            keep = []
            for i, ((a, first, n, hin, hout), b) in enumerate(zip(HELD_WRITES, bs)):
                rows = []
                if hin:
                    rows.append(np.stack([ik_host[1 + i], iv_host[1 + i]], axis=1))          # [L][2][1024]: as it is, K too
                for t in range(n):
                    s = int(slots[int(b) + t])
                    rows.append(flat16[:, :, BS + s] if 0 <= s < N_SLOTS else np.zeros((L, 2, HALF), dtype=np.uint16))
                if hout:
                    last = rows.pop()
                    ok_host[1 + i], ov_host[1 + i] = last[:, 0], last[:, 1]
                if rows:
                    _twin_runs(lib, torch, twins[a], first - (1 if hin else 0), np.stack(rows, axis=2), st, keep)
            for h, tw in zip(handles, twins):
                _compare_allocations(lib, torch, h, tw, scheme, st, (scheme, elem, kind_fast))
            got_k, got_v = ok.cpu().numpy().view(np.uint16), ov.cpu().numpy().view(np.uint16)
            nan = fp16_is_nan(ok_host)
            assert _same(got_k, ok_host, nan, FP16) and _same(got_v, ov_host, fp16_is_nan(ov_host), FP16), (scheme, elem, kind_fast, "held-out rows")
            assert not got_k[1 + 4].any() and not got_v[1 + 4].any() and got_k[1 + 1].any()    # a padding slot gives zeros
            assert np.array_equal(_host(caches).reshape(content.shape), content), "write_slots_kmul changed the caches"
            for h in handles + twins:
                lib.free(h)
        assert np.array_equal(ik.cpu().numpy().view(np.uint16), ik_host) and np.array_equal(iv.cpu().numpy().view(np.uint16), iv_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_kmul_entries_launches_nothing():
    """every refusal of the _ex entries and the two new ones (a factor pointer that is not 16-byte aligned, a stride that is no
    multiple of 16), capture included: caches, pool, held-out rows and statistics stay as they were"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(4)
        h, h2 = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
        _fill(lib, h, _blocks(N_PAGES, 7))
        lib.set_compression_scheme(3)
        other = lib.alloc(N_PAGES * PAGE)
        st = torch.cuda.Stream()
        s = st.cuda_stream
        caches = _caches(torch)
        pattern = _host(caches)
        bases, ks = _bases(caches), _kind_stride(caches)
        d_slots = torch.arange(64, dtype=torch.int64, device="cuda")
        image = _image(lib, torch, h, st)
        (ik, _), (iv, _) = _held_block(torch, 2, 1), _held_block(torch, 2, 2)
        (ok, ok_host), (ov, ov_host) = _held_block(torch, 2), _held_block(torch, 2)
        one = lambda blk, i=0: u64(*_held_ptrs(blk, [j == i for j in range(2)], 2)[2 * i:2 * i + 2])
        IN, OUT = one((ik, iv)), one((ok, ov))
        mul = factor_bits(L)
        d_mul, p_mul, _ = _factors(torch, mul)
        good = dict(handles=u64(h), firsts=u64(0), counts=u64(8), begins=u64(0), slots=d_slots.data_ptr(), n_slots=N_SLOTS, bases=bases,
                    layer_begin=0, ks=ks, step=STEP, stream=s, elem=BF16, held_in=None, held_stride=ROW, held_out=None, reserved=0,
                    k_mul=p_mul, k_mul_stride=ROW)
        inval = [
            dict(stream=0), dict(slots=0), dict(bases=u64(bases[0], 0)), dict(bases=u64(bases[0], bases[1] + 8)), dict(ks=ks + 8), dict(step=0),
            dict(handles=u64(h, other), firsts=u64(0, 0), counts=u64(8, 8), begins=u64(0, 8)),          # allocations of different schemes
            dict(elem=2), dict(elem=0xFFFFFFFF), dict(reserved=1),                                      # an unknown elem, reserved != 0
            dict(held_stride=ROW + 8),                                                                  # a stride that is no multiple of 16
            dict(k_mul=p_mul + 8), dict(k_mul=p_mul + 2),                                               # the factor rows not 16-byte aligned
            dict(k_mul_stride=ROW + 8), dict(k_mul_stride=2),                                           # their stride no multiple of 16
        ]
        read_inval = [
            dict(counts=u64(9), held_out=OUT),                                                          # d_held_out on the read side
            dict(counts=u64(9), held_in=u64(IN[0], 0)), dict(counts=u64(9), held_in=u64(0, IN[1])),     # only one of K / V
            dict(counts=u64(9), held_in=u64(IN[0] + 8, IN[1])),                                         # not 16-byte aligned
            dict(counts=u64(8), held_in=IN),                                                            # the last position is odd
            dict(counts=u64(0), held_in=IN),                                                            # a held row for an empty span
        ]
        write_inval = [
            dict(firsts=u64(1)), dict(counts=u64(7)),                                                   # odd first / end without held rows
            dict(firsts=u64(1), counts=u64(7), held_out=OUT),                                           # odd first without held-in
            dict(held_in=IN),                                                                           # held-in with an even first
            dict(counts=u64(7), held_in=IN),
            dict(held_out=OUT),                                                                         # held-out with an even end
            dict(firsts=u64(1), counts=u64(7), held_in=IN, held_out=OUT),
            dict(firsts=u64(1), counts=u64(7), held_in=u64(IN[0], 0)),                                  # only one of K / V
            dict(counts=u64(7), held_out=u64(0, OUT[1])),
            dict(counts=u64(7), held_out=u64(OUT[0] + 8, OUT[1])),                                      # not 16-byte aligned
            dict(firsts=u64(1), counts=u64(7), held_in=u64(IN[0], IN[1] + 4)),
            dict(counts=u64(7), held_out=OUT, k_mul=p_mul + 8),                                         # the new refusals with held-out rows
            dict(counts=u64(7), held_out=OUT, k_mul_stride=ROW + 4),
            dict(handles=u64(h, h), firsts=u64(0, 6), counts=u64(8, 4), begins=u64(0, 8)),              # two spans share a page ...
            dict(handles=u64(h, h), firsts=u64(0, 7), counts=u64(8, 3), begins=u64(0, 8),               # ... through the held-in pair
                 held_in=u64(0, 0, *one((ik, iv), 1))),
        ]
        general = [dict(handles=u64(h + 12345)), dict(firsts=u64(2 * STEP - 4)), dict(step=N_PAGES), dict(layer_begin=1)]

        def call(entry, a):
            entry(a["handles"], a["firsts"], a["counts"], a["begins"], a["slots"], a["n_slots"], a["bases"], a["layer_begin"], a["ks"],
                  a["step"], a["stream"], elem=a["elem"], held_in=a["held_in"], held_stride=a["held_stride"], held_out=a["held_out"],
                  reserved=a["reserved"], k_mul=a["k_mul"], k_mul_stride=a["k_mul_stride"])

        def counters():
            x = lib.stats()
            return (x.total_compressions, x.total_decompressions, x.original_bytes, x.dma_submitted, x.dma_completed)

        def untouched():
            torch.cuda.synchronize()
            assert np.array_equal(_host(caches), pattern), "a refused call wrote to the caches"
            assert np.array_equal(_image(lib, torch, h, st), image) and not _image(lib, torch, h2, st).any(), "a refused call wrote to the pool"
            assert np.array_equal(ok.cpu().numpy().view(np.uint16), ok_host) and np.array_equal(ov.cpu().numpy().view(np.uint16), ov_host), \
                "a refused call wrote to the held-out rows"

        for entry, cases in ((lib.read_slots_kmul, [(-4, inval + read_inval), (-1, general)]),
                             (lib.write_slots_kmul, [(-4, inval + write_inval), (-1, general)])):
            stats = counters()
            for status, group in cases:
                for case in group:
                    a = dict(good)
                    a.update(case)
                    with pytest.raises(SpeckvError) as e:
                        call(entry, a)
                    assert e.value.status == status, (entry.__name__, case, e.value.status)
            assert counters() == stats, "a refused call was counted"
            untouched()
        for name in ("speckv_ext_read_slots_kmul", "speckv_ext_write_slots_kmul"):                     # no options at all
            with pytest.raises(SpeckvError) as e:
                lib._ext(name, u64(h).ctypes.data, u64(0).ctypes.data, u64(8).ctypes.data, u64(0).ctypes.data, 1, d_slots.data_ptr(), N_SLOTS,
                         bases.ctypes.data, 0, L, ks, STEP, None, p_mul, ROW, s)
            assert e.value.status == -4, name
        untouched()
        bump = torch.zeros(4, device="cuda")                                # a capturing stream: the descriptors are staged per call
        torch.cuda.synchronize()
        stats = counters()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            for entry, case in ((lib.read_slots_kmul, dict(counts=u64(9), held_in=IN)), (lib.write_slots_kmul, dict(counts=u64(7), held_out=OUT))):
                with pytest.raises(SpeckvError) as e:
                    call(entry, dict(good, **case))
                assert e.value.status == -4
            bump.add_(1)
        g.replay()
        assert counters() == stats                                          # (before untouched(): its fetch_range calls are counted)
        untouched()
        del g
        for entry in (lib.read_slots_kmul, lib.write_slots_kmul):         # nothing to do: fine
            call(entry, dict(good, handles=u64(), firsts=u64(), counts=u64(), begins=u64()))
            call(entry, dict(good, bases=u64()))
            call(entry, dict(good, handles=u64(h, h2), firsts=u64(0, 64), counts=u64(0, 0), begins=u64(0, 0)))
        untouched()
        call(lib.read_slots_kmul, dict(good, counts=u64(9), held_in=IN))  # ... and the good calls do their work
        st.synchronize()
        got = _host(caches)
        for t in range(8):
            assert np.array_equal(got[1, 1, BS + t], fp16_to_bf16_bits(_row(image, 1, 1, t)))
            assert np.array_equal(got[1, 0, BS + t], scaled_to_bf16_bits(_row(image, 1, 0, t), mul[1]))
        assert np.array_equal(got[1, 1, BS + 8], fp16_to_bf16_bits(iv.cpu().numpy().view(np.uint16)[1, 1]))
        assert np.array_equal(got[1, 0, BS + 8], scaled_to_bf16_bits(ik.cpu().numpy().view(np.uint16)[1, 1], mul[1]))
        call(lib.write_slots_kmul, dict(good, handles=u64(h2), counts=u64(7), held_out=OUT))
        st.synchronize()
        assert _image(lib, torch, h2, st)[:3].any() and not _image(lib, torch, h2, st)[3].any()
        assert not np.array_equal(ok.cpu().numpy().view(np.uint16)[1], ok_host[1])
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ placement
def _held_write_against_twin(lib, torch, h, tw, st, seed, mul, p_mul):
    """one write_slots_kmul from bf16 caches with a held-in and a held-out row -- positions [3, 9) of h: pairs 1 .. 3 -- and the same
    positions, restated, by write_runs into tw; checks the held-out rows"""
    content = _as_bf16(_random_content(seed))
    flat16 = _pool_side(content.reshape(L, 2, (NB + 2) * BS, HALF), mul, BF16)
    caches = _caches(torch, content)
    slots = np.asarray([30, 31, 32, 33, 34, 35], dtype=np.int64)
    d_slots = torch.from_numpy(slots).cuda()
    (ik, ik_host), (iv, iv_host) = _held_block(torch, 1, seed + 1), _held_block(torch, 1, seed + 2)
    (ok, _), (ov, _) = _held_block(torch, 1), _held_block(torch, 1)
    torch.cuda.synchronize()
    lib.write_slots_kmul(u64(h), u64(3), u64(6), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                         elem=BF16, held_in=_held_ptrs((ik, iv), [True], 1), held_stride=ROW, held_out=_held_ptrs((ok, ov), [True], 1),
                         k_mul=p_mul, k_mul_stride=ROW)
    st.synchronize()
    rows = [np.stack([ik_host[1], iv_host[1]], axis=1)] + [flat16[:, :, BS + int(s)] for s in slots[:5]]
    _twin_runs(lib, torch, tw, 2, np.stack(rows, axis=2), st, [])
    assert np.array_equal(ok.cpu().numpy().view(np.uint16)[1], flat16[:, 0, BS + 35]) and np.array_equal(ov.cpu().numpy().view(np.uint16)[1], flat16[:, 1, BS + 35])


def _held_read_check(lib, torch, h, image, st, first, n, slot0, mul, p_mul, what):
    """read_slots_kmul of [first, first + n) into bf16 blocks, the last position from a held row: against the restated image"""
    caches = _caches(torch)
    want = _host(caches)
    slots = np.arange(slot0, slot0 + n, dtype=np.int64)
    (ik, ik_host), (iv, iv_host) = _held_block(torch, 1, 5), _held_block(torch, 1, 6)
    _expect_read(want, np.zeros(want.shape, dtype=bool), [image], [(0, first, n)], [0], slots, mul, BF16, held=([True], ik_host, iv_host))
    d_slots = torch.from_numpy(slots).cuda()
    torch.cuda.synchronize()
    lib.read_slots_kmul(u64(h), u64(first), u64(n), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP,
                        st.cuda_stream, elem=BF16, held_in=_held_ptrs((ik, iv), [True], 1), held_stride=ROW, k_mul=p_mul, k_mul_stride=ROW)
    st.synchronize()
    assert np.array_equal(_host(caches), want), what


def test_placement_striped_migrated_sealed_and_cached_with_the_factor():
    torch = torch_mod()
    mul = factor_bits(L)
    for scheme in (4, 5):
        lib = open_lib(SPECKV_POOL_DEVICES="0,0,0")
        try:
            d_mul, p_mul, _ = _factors(torch, mul)
            lib.set_compression_scheme(scheme)
            h, tw = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
            for a in (h, tw):
                _fill(lib, a, _blocks(N_PAGES, 40))
            lib.migrate(h, 1, 4, 1)                                       # pages 1 .. 4 and a page of another region now lie elsewhere
            lib.migrate(h, 2 * STEP + 15, 3, 2)
            st = torch.cuda.Stream()
            _held_write_against_twin(lib, torch, h, tw, st, 80, mul, p_mul)
            got, want = _image(lib, torch, h, st), _image(lib, torch, tw, st)
            assert np.array_equal(got, want), ("striped / migrated write", scheme)
            _held_read_check(lib, torch, h, got, st, 2, 7, 40, mul, p_mul, ("striped / migrated read", scheme))
        finally:
            lib.finalize()
    lib = open_lib()
    try:
        d_mul, p_mul, _ = _factors(torch, mul)
        lib.set_compression_scheme(2)
        h, tw, h3 = (lib.alloc(N_PAGES * PAGE) for _ in range(3))
        for a in (h, tw, h3):
            _fill(lib, a, _blocks(N_PAGES, 60))
        lib.compact(h)
        lib.compact(h3)
        assert lib.stats().sealed_allocations == 2
        st = torch.cuda.Stream()
        image = _image(lib, torch, h, st)
        _held_read_check(lib, torch, h, image, st, 10, 5, 10, mul, p_mul, "sealed read")
        assert lib.stats().sealed_allocations == 2, "read_slots_kmul leaves a sealed allocation sealed"
        _held_write_against_twin(lib, torch, h, tw, st, 81, mul, p_mul)
        assert lib.stats().sealed_allocations == 1, "write_slots_kmul unpacks a sealed destination"
        assert np.array_equal(_image(lib, torch, h, st), _image(lib, torch, tw, st))
        # a page cached by speckv_access before the write
        page = 2 * STEP + 2                                            # layer 1, K, positions 4 and 5
        h4, tw4 = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
        for a in (h4, tw4):
            _fill(lib, a, _blocks(N_PAGES, 61))
        ptr = lib.access(h4, page * PAGE, 64)
        old = dev_to_host(ptr, PAGE).view(np.uint16).copy()
        assert lib.translate(h4, page * PAGE).flags & 3
        _held_write_against_twin(lib, torch, h4, tw4, st, 82, mul, p_mul)
        new = dev_to_host(lib.access(h4, page * PAGE, 64), PAGE).view(np.uint16)
        want = _image(lib, torch, tw4, st)[page]
        assert np.array_equal(new, want) and not np.array_equal(new, old), "a cached page shows the bytes of before the write"
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------- ordering
@pytest.mark.parametrize("scheme", [2, 4])
def test_ordering_of_the_kmul_entries_on_one_stream_and_across_streams(scheme):
    """write_slots_kmul then read_slots_kmul on one busy, non-current stream with nothing between them, and a read on stream B behind
    a write on stream A: the read returns what was written, the held-out row of the write included (it is the read's held-in row)"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        content = _as_bf16(_random_content(31))
        n = 63
        slots = np.random.default_rng(3).permutation(N_SLOTS)[:n].astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        out_slots = torch.from_numpy(np.arange(n, dtype=np.int64)).cuda()
        mul = factor_bits(L)
        inv = _inverse(mul)
        (d_mul, p_mul, _), (d_inv, p_inv, _) = _factors(torch, mul), _factors(torch, inv)
        flat16 = _pool_side(content.reshape(L, 2, (NB + 2) * BS, HALF), inv, BF16)
        busy = torch.randn((2048, 2048), device="cuda")
        for two_streams in (False, True):
            h = lib.alloc(N_PAGES * PAGE)
            src, dst = _caches(torch, content), _caches(torch)
            (tk, _), (tv, _) = _held_block(torch, 1), _held_block(torch, 1)
            tail = _held_ptrs((tk, tv), [True], 1)
            a, b = torch.cuda.Stream(), torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(a):
                for _ in range(20):
                    busy = busy @ busy * 1e-3                          # the stream has work queued in front of the write
            lib.write_slots_kmul(u64(h), u64(0), u64(n), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(src), 0, _kind_stride(src), STEP, a.cuda_stream,
                                 elem=BF16, held_out=tail, held_stride=ROW, k_mul=p_inv, k_mul_stride=ROW)
            rs = b if two_streams else a
            if two_streams:
                b.wait_stream(a)                                       # the held row is the caller's memory: the caller orders it
            lib.read_slots_kmul(u64(h), u64(0), u64(n), u64(0), out_slots.data_ptr(), N_SLOTS, _bases(dst), 0, _kind_stride(dst), STEP, rs.cuda_stream,
                                elem=BF16, held_in=tail, held_stride=ROW, k_mul=p_mul, k_mul_stride=ROW)
            torch.cuda.synchronize()
            image = _image(lib, torch, h, a)
            got = _host(dst)
            assert image[0].any()
            for layer in range(L):
                for kind in (0, 1):
                    back = (lambda r: scaled_to_bf16_bits(r, mul[layer])) if kind == 0 else fp16_to_bf16_bits
                    for t in range(n - 1):
                        assert np.array_equal(got[layer, kind, BS + t], back(_row(image, layer, kind, t))), (two_streams, layer, kind, t)
                    assert np.array_equal(got[layer, kind, BS + n - 1], back(flat16[layer, kind, BS + int(slots[n - 1])]))
    finally:
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------- the connector
class _CountingKmul(_Counting):
    NAMES = _Counting.NAMES + ("read_slots_ex", "write_slots_ex", "read_slots_kmul", "write_slots_kmul", "write_strided", "write_strided_batch")


def _typed_caches(torch, content, elem):
    """_caches with the views typed by `elem`"""
    return [(big, big.view(torch.bfloat16)[:, 1:-1] if elem == BF16 else view) for big, view in _caches(torch, content)]


def _unit_content(seed):
    """bf16 cache bits of magnitude about 1: +-[0.5, 2), a row of zeros and a constant row -- where one rounding and the row route's
    two give the same bits for factors 2^-4 .. 2^4 (tests/test_paged_io_kscale_cpu.py)"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.5, 2.0, (L, 2, NB + 2, BS, H * D)) * rng.choice([-1.0, 1.0], (L, 2, NB + 2, BS, H * D))).astype(np.float32)
    x[:, :, 2, 3] = 0
    x[:, :, 4] = x[:, :, 4, :1, :1]
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def _cache_content(seed, elem):
    """fp16: unrestricted (random rows, some that compress); bf16: magnitude about 1"""
    return _unit_content(seed) if elem == BF16 else _random_content(seed)


def _prescale(torch):
    """[L][H][D] powers of two 2^-4 .. 2^4 that differ by layer, head and channel"""
    return _dev(torch, factor_bits(L).view(np.float16).astype(np.float32).reshape(L, H, D))


CHUNKS = (5, 1, 1, 2, 3, 21)


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_connector_with_a_prescale_chunked_store_append_and_load(scheme, elem):
    """A connector with a K pre-scale built by store_paged(fused=True, kscale=True) in chunks of 5, 1, 1, 2, 3 and 21 positions against
    a twin with the same pre-scale built by write_prefill + append from the same rows: attend out and lse equal to the bit after every
    chunk, kv_rows at the end; exactly one library call per store_paged / load_paged; a lockstep append straight after a store pairs
    the batched tails; load_paged(fused=True, kscale=True) equals the row route, for odd ends and a tail."""
    torch = torch_mod()
    lib = _CountingKmul(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        rng = np.random.default_rng(41)
        paged, twin = SpeckvKVConnector(lib, L, H, D, T, scheme), SpeckvKVConnector(lib, L, H, D, T, scheme)
        for c in (paged, twin):
            c.set_k_channel_scale(_prescale(torch))
        content = _cache_content(43, elem)
        flat16 = _from_cache(content, elem).reshape(L, 2, (NB + 2) * BS, H, D)
        caches = [v for _, v in _typed_caches(torch, content, elem)]
        perm = rng.permutation(N_SLOTS).astype(np.int64)
        ids, tids = [1, 2], [101, 102]
        maps = {1: perm[:40], 2: perm[40:80]}
        for rid, tid in zip(ids, tids):
            paged.add_request(rid)
            twin.add_request(tid)
        rows = {rid: (_dev(torch, flat16[:, 0, BS + maps[rid]].view(np.float16)), _dev(torch, flat16[:, 1, BS + maps[rid]].view(np.float16))) for rid in ids}
        keep = []
        G, sm = 4, 1.0 / np.sqrt(D)

        def attend_equal(a_ids, b_ids, what):
            for layer in range(L):
                q = _dev(torch, rng.standard_normal((1, len(a_ids), H, G, D)).astype(np.float16))
                out_a, lse_a, _ = paged._attend_layers_lse(layer, 1, a_ids, q, sm, None, None)
                out_b, lse_b, _ = twin._attend_layers_lse(layer, 1, b_ids, q, sm, None, None)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(out_a), _bits(out_b)) and np.array_equal(_bits(lse_a), _bits(lse_b)), (scheme, elem, what, layer)
                assert bool(torch.isfinite(out_a).all())

        at = 0
        for ci, c in enumerate(CHUNKS):                                   # request 1 alone, chunk by chunk
            torch.cuda.synchronize()
            lib.calls.clear()
            keep += paged.store_paged([1], [c], _dev(torch, maps[1][at:at + c]), caches, fused=True, kscale=True)
            assert lib.calls == ["write_slots_kmul"], lib.calls
            k, v = rows[1]
            if ci == 0:
                keep += twin.write_prefill(101, k[:, :c].contiguous(), v[:, :c].contiguous())
            else:
                for t in range(at, at + c):
                    keep.append(twin.append([101], k[:, t][None].contiguous(), v[:, t][None].contiguous()))
            at += c
            assert paged.length(1) == twin.length(101) == at
            attend_equal([1], [101], ("chunk", ci))
        assert at == 33
        a, b = _all_rows(paged, 1), _all_rows(twin, 101)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (scheme, elem, "stored rows")
        # ---- both requests to an odd length by one call, then a lockstep append: the batched tails are paired as they are
        torch.cuda.synchronize()
        lib.calls.clear()
        keep += paged.store_paged([2, 1], [7, 2], _dev(torch, np.concatenate([maps[2][:7], maps[1][33:35]])), caches, fused=True, kscale=True)
        assert lib.calls == ["write_slots_kmul"], lib.calls
        k2, v2 = rows[2]
        keep += twin.write_prefill(102, k2[:, :7].contiguous(), v2[:, :7].contiguous())
        for t in (33, 34):
            keep.append(twin.append([101], rows[1][0][:, t][None].contiguous(), rows[1][1][:, t][None].contiguous()))
        assert paged._tail_ids == (2, 1) and tuple(paged._tail_k.shape) == (2, L, H, D)
        k_new, v_new = _dev(torch, rng.standard_normal((2, L, H, D)).astype(np.float16)), _dev(torch, rng.standard_normal((2, L, H, D)).astype(np.float16))
        lib.calls.clear()
        keep.append(paged.append([2, 1], k_new, v_new))
        assert lib.calls == ["write_strided_batch"] and paged._tail_ids == ()
        keep.append(twin.append([102, 101], k_new, v_new))
        attend_equal([2, 1], [102, 101], "lockstep append after a store")
        for rid, tid in zip(ids, tids):
            assert paged.length(rid) == twin.length(tid)
            assert all(np.array_equal(x, y) for x, y in zip(_all_rows(paged, rid), _all_rows(twin, tid))), (scheme, elem, rid, "after the append")
        # ---- one more position each (tails again), then load into fresh blocks of the same type: against the row route
        keep += paged.store_paged([1, 2], [1, 1], _dev(torch, np.concatenate([maps[1][36:37], maps[2][8:9]])), caches, fused=True, kscale=True)
        assert paged.length(1) == 37 and paged.length(2) == 9
        loads = [(1, 3, 34), (2, 1, 6), (1, 0, 37), (2, 8, 1)]          # odd ends up to the tail; odd ends; a whole request; only the tail
        lmap = rng.permutation(N_SLOTS).astype(np.int64)[:sum(n for _, _, n in loads)]
        lmap[5] = -1
        d_lmap = _dev(torch, lmap)
        fresh = _typed_caches(torch, None, elem)
        torch.cuda.synchronize()
        lib.calls.clear()
        paged.load_paged([r for r, _, _ in loads], [f for _, f, _ in loads], [n for _, _, n in loads], d_lmap, [v for _, v in fresh], fused=True,
                         kscale=True)
        torch.cuda.synchronize()
        assert lib.calls == ["read_slots_kmul"], lib.calls
        route = _typed_caches(torch, None, elem)                           # the row route a pre-scaled connector takes without the keyword
        keep_map = d_lmap.clone()
        keep_map[5] = int(lmap[4])                                         # (index_copy_ takes no -1: the row is written twice instead)
        lib.calls.clear()
        paged.load_paged([r for r, _, _ in loads], [f for _, f, _ in loads], [n for _, _, n in loads], keep_map, [v for _, v in route], fused=True)
        torch.cuda.synchronize()
        assert "read_slots_kmul" not in lib.calls and "read_slots_ex" not in lib.calls and "fetch_range" in lib.calls
        got, want = _host(fresh), _host(route)
        s4 = BS + int(lmap[4])
        got[:, :, s4] = want[:, :, s4] = 0
        assert np.array_equal(got, want), (scheme, elem, "load_paged(fused=True, kscale=True) is not the row route")
        assert (got[:, 0] != 0x7C5A).any()
    finally:
        lib.finalize()


@pytest.mark.parametrize("elem", [FP16, BF16])
def test_connector_without_a_prescale_gives_the_fused_call(elem):
    """no pre-scale: the keyword gives the bits and the calls of fused=True"""
    torch = torch_mod()
    lib = _CountingKmul(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        a, b = SpeckvKVConnector(lib, L, H, D, T, "int4"), SpeckvKVConnector(lib, L, H, D, T, "int4")
        content = _cache_content(47, elem)
        caches = [v for _, v in _typed_caches(torch, content, elem)]
        slots = _dev(torch, np.random.default_rng(1).permutation(N_SLOTS).astype(np.int64)[:40])
        out = []
        for conn, kw in ((a, dict(fused=True, kscale=True)), (b, dict(fused=True))):
            conn.add_request(1)
            lib.calls.clear()
            keep = conn.store_paged([1], [33], slots[:33], caches, **kw)
            keep += conn.store_paged([1], [4], slots[33:37], caches, **kw)
            fresh = _typed_caches(torch, None, elem)
            conn.load_paged([1, 1], [1, 30], [30, 7], slots[:37], [v for _, v in fresh], **kw)
            torch.cuda.synchronize()
            assert lib.calls == ["write_slots_ex", "write_slots_ex", "read_slots_ex"], lib.calls
            out.append((_host(fresh), _all_rows(conn, 1)))
        assert np.array_equal(out[0][0], out[1][0]) and all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))
        assert (out[0][0] != 0x7C5A).any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------- the adapter
def test_adapter_paged_kscale_on_bf16_equals_the_row_route():
    """the walk of test_adapter_paged_fused_on_bf16_equals_the_row_route on connectors with a K pre-scale: paged_io=True,
    paged_fused=True, paged_kscale=True against paged_io=False -- store, freed blocks, a prefix hit, a resumed request, a foreign
    kv_layer, an odd prompt; caches and pools equal to the bit after every step, one _kmul call per step on the paged side"""
    torch = torch_mod()
    from types import SimpleNamespace as NS
    from cxl_speckv_amd.vllm_connector import SpeckvVllmConnector, slot_mapping_for
    lib = _CountingKmul(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        names = [f"model.layers.{i}.self_attn.attn" for i in range(L)]
        sides = {}
        for paged in (True, False):
            c = SpeckvVllmConnector(lib, num_layers=L, num_kv_heads=H, head_dim=D, block_size=BS, max_tokens=T, scheme="int4", paged_io=paged,
                                    paged_fused=paged, paged_kscale=paged)
            c.conn.set_k_channel_scale(_prescale(torch))
            big = _typed_caches(torch, None, BF16)
            for b, _ in big:
                b.zero_()
            caches = {n: v for n, (_, v) in zip(names, big)}
            c.register_kv_caches(caches)
            if not paged:
                c._next_id = 1001
            sides[paged] = (c, caches, big)
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        prompts = {"req-a": (40, [3, 9, 4]), "req-b": (64, [10, 1, 7, 0]), "req-c": (33, [2, 5, 8]), "req-d": (35, [11, 0, 6])}

        def each(f):
            for paged in (True, False):
                lib.calls.clear()
                f(paged, *sides[paged][:2])

        def same(what):
            torch.cuda.synchronize()
            assert np.array_equal(_host(sides[True][2]), _host(sides[False][2])), (what, "caches")
            a, b = sides[True][0], sides[False][0]
            ids_a, ids_b = {rid: eid for eid, rid in a._live.items()}, {rid: eid for eid, rid in b._live.items()}
            assert sorted(ids_a) == sorted(ids_b) and ids_a, what
            for rid, eid in ids_a.items():
                assert a.conn.length(eid) == b.conn.length(ids_b[rid]), (what, rid)
                for layer in range(L):
                    for kind in (0, 1):
                        assert np.array_equal(_bits(a.conn.kv_rows(eid, layer, kind)), _bits(b.conn.kv_rows(ids_b[rid], layer, kind))), (what, rid, layer, kind)

        def unit(n):                                                       # magnitude about 1: +-[0.5, 2)
            mag = torch.rand((2, n, H, D), generator=gen, device="cuda") * 1.5 + 0.5
            sign = (torch.rand((2, n, H, D), generator=gen, device="cuda") < 0.5).to(torch.float32) * 2 - 1
            return (mag * sign).to(torch.bfloat16)

        rows = {(rid, li): unit(n) for rid, (n, _) in prompts.items() for li in range(L)}

        def store(rids, foreign=False):
            def run(paged, c, caches):
                new = [NS(req_id=rid, prompt_token_ids=list(range(prompts[rid][0])), block_ids=[prompts[rid][1]]) for rid in rids]
                meta = c.build_connector_meta(NS(scheduled_new_reqs=new))
                c.bind_connector_metadata(meta)
                c.start_load_kv(None)
                for li, name in enumerate(names):
                    flat = caches[name].reshape(2, NB * BS, H, D)
                    for rid in rids:
                        n, blk = prompts[rid]
                        flat[:, torch.tensor(slot_mapping_for(blk, BS, n), device="cuda")] = rows[(rid, li)]
                    layer = caches[name].clone() if foreign and li == 1 else caches[name]
                    c.save_kv_layer(name, layer, None)
                c.wait_for_save()
                c.clear_connector_metadata()
                torch.cuda.synchronize()
                if paged and not foreign:
                    assert lib.calls == ["write_slots_kmul"], lib.calls
                if paged and foreign:
                    assert "write_slots_kmul" not in lib.calls and lib.calls.count("write_runs") == len(rids), lib.calls
            each(run)

        def load(rids, blocks, computed, resumed, what):
            def run(paged, c, caches):
                for t in caches.values():
                    t.zero_()
                for rid in rids:
                    n = prompts[rid][0]
                    req = NS(request_id=rid, num_tokens=n)
                    matched, is_async = c.get_num_new_matched_tokens(req, computed)
                    assert matched == (n - 1) // BS * BS - computed and is_async is False
                    c.update_state_after_alloc(req, NS(get_block_ids=lambda b=blocks[rid]: [b]), matched)
                if resumed:
                    out = NS(scheduled_new_reqs=[], scheduled_cached_reqs=NS(req_ids=list(rids), new_block_ids=[[blocks[r]] for r in rids],
                                                                              num_computed_tokens=[computed] * len(rids),
                                                                              resumed_from_preemption=[True] * len(rids)))
                else:
                    out = NS(scheduled_new_reqs=[NS(req_id=rid, prompt_token_ids=list(range(prompts[rid][0])), block_ids=[blocks[rid]]) for rid in rids])
                meta = c.build_connector_meta(out)
                assert [m.is_store for m in meta.requests] == [False] * len(rids)
                c.bind_connector_metadata(meta)
                c.start_load_kv(None)
                c.clear_connector_metadata()
                torch.cuda.synchronize()
                if paged:
                    assert lib.calls == ["read_slots_kmul"], (what, lib.calls)
                else:
                    assert not any(name.startswith("read_slots") for name in lib.calls)
            each(run)
            same(what)

        store(["req-a", "req-b"])
        same("store")
        load(["req-a", "req-b"], {"req-a": [6, 0, 2], "req-b": [1, 3, 5, 7]}, 0, False, "load into other blocks")
        load(["req-b"], {"req-b": [9, 8, 4, 2]}, 16, False, "prefix hit: the first block is vLLM's own")
        load(["req-a"], {"req-a": [10, 9, 8]}, 0, True, "a preempted request resumed with a new block table")
        store(["req-c"], foreign=True)
        same("a kv_layer that is not the registered tensor")
        load(["req-c"], {"req-c": [4, 6, 1]}, 0, False, "load of the request stored by the stash route")
        store(["req-d"])                                                    # an odd prompt by the launch: its last position is held out
        same("an odd prompt stored by the one launch")
        load(["req-d"], {"req-d": [7, 3, 9]}, 0, False, "load of the odd prompt")
    finally:
        lib.finalize()


def test_the_kscale_example_runs():
    """examples/paged_cache_kscale_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "paged_cache_kscale_example.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "paged cache kscale example ok" in out.stdout
