"""-m gpu: the fused paged-cache route -- speckv_ext_read_slots_ex / speckv_ext_write_slots_ex (bf16 caches, held rows),
load_paged / store_paged with fused=True and SpeckvVllmConnector(paged_io=True, paged_fused=True).

References: the numpy restatement of the two conversion rules (tests/test_paged_io_fused_cpu.py) applied to
speckv_ext_fetch_range's image for a read, and to the rows a twin allocation gets by speckv_ext_write_runs for a write; never a
device cast.  Every comparison is exact; of a NaN only the position is compared.  Geometry and helpers are those of
tests/test_gpu_paged_io.py (L = 2, T = 128, blocks of 16 slots, 12 blocks, caches between guard blocks, n_slots one block short)."""
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

pytestmark = pytest.mark.gpu
FP16, BF16 = 0, 1
HALF = ROW // 2                                 # elements of a row


def _to_cache(rows, elem):
    """what a cache of element type `elem` holds for the pool's fp16 bits `rows`"""
    return fp16_to_bf16_bits(rows) if elem == BF16 else rows


def _from_cache(rows, elem):
    """the fp16 bits the pool encodes for a cache row"""
    return bf16_to_fp16_bits(rows) if elem == BF16 else rows


def _same(got, want, nan, elem_out):
    return equal_off_nan(got, want, nan, bf16_is_nan if elem_out == BF16 else fp16_is_nan)


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


# ------------------------------------------------------------------------------------------------------------------- read_ex
ALL_SPAN = (2, 0, 64)                           # the positions of allocation 2 whose region 0 holds all 65 536 fp16 patterns


def _patterns_alloc(lib, seed):
    """an allocation like _fill's, its hole at page 40, whose pages 0 .. 31 of region 0 hold every fp16 pattern"""
    x = _blocks(N_PAGES, seed)
    x[:32] = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).reshape(32, ROW)
    h = lib.alloc(N_PAGES * PAGE)
    _fill(lib, h, x, hole=40)
    return h


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_read_ex_to_bf16_is_the_restatement_of_fetch_range(scheme, mode):
    """Spans [0, 34), [5, 32), [33, 34), [64, 64) with two -1 slots and one >= n_slots, and [0, 64) of the allocation whose first
    region holds every fp16 pattern (what the FP16 scheme returns as it is), both wave orders: the caches, guards included, are the
    restatement applied to fetch_range's image."""
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
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _caches(torch)
            want = _host(caches)
            nan = np.zeros(want.shape, dtype=bool)
            for (a, first, n), b in zip(spans, bs):
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        for layer in range(L):
                            for kind in (0, 1):
                                row = _row(images[a], layer, kind, first + t)
                                want[layer, kind, BS + s] = fp16_to_bf16_bits(row)
                                nan[layer, kind, BS + s] = fp16_is_nan(row)
            before = lib.stats()
            torch.cuda.synchronize()
            lib.read_slots_ex(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream, elem=BF16)
            st.synchronize()
            got = _host(caches)
            assert _same(got, want, nan, BF16), (scheme, mode, kind_fast, np.argwhere(((got != want) & ~nan).any(axis=-1))[:8])
            pages = 2 * L * sum((f + n + 1) // 2 - f // 2 for _, f, n in spans if n)
            assert lib.stats().total_decompressions - before.total_decompressions == pages
        assert nan.any() or scheme != 0
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ write_ex
def _bf16_content(seed):
    """[L][2][NB + 2][BS][1024] bf16 bits: random rows everywhere; slots 0 .. 63 hold every bf16 pattern; slots 64 .. 71 a page of
    zeros, a page of constant runs, a page with inf and NaN in random rows, a page of -0 and subnormals"""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((L, 2, NB + 2, BS, HALF)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    flat = c.reshape(L, 2, (NB + 2) * BS, HALF)
    flat[:, :, BS:BS + 64] = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(64, HALF)
    flat[:, :, BS + 64:BS + 66] = 0
    flat[:, :, BS + 66] = np.repeat(flat[:, :, BS + 66, :32], 32, axis=-1)
    flat[:, :, BS + 67] = flat[:, :, BS + 67, :1]
    for k, bits in enumerate((0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81)):               # +-inf, NaNs
        flat[:, :, BS + 68, 17 + 97 * k] = bits
        flat[:, :, BS + 69, 1000 - 31 * k] = bits
    flat[:, :, BS + 70] = 0x8000
    flat[:, :, BS + 71] = 0x0080                                                      # 2^-126: rounds to +0 in fp16
    return c


WRITE_SPANS = [(0, 0, 64), (1, 6, 26), (0, 64, 8)]


def _twin_runs(lib, torch, twin, first_pos, rows16, stream, keep):
    """write_runs of rows16 [L][2][n][1024] fp16 bits (n even) at position first_pos (even) of allocation `twin`"""
    n = rows16.shape[2]
    assert n % 2 == 0 and first_pos % 2 == 0
    d = torch.from_numpy(np.ascontiguousarray(rows16).view(np.int16)).cuda()
    keep.append(d)
    firsts = [(2 * layer + kind) * STEP + first_pos // 2 for layer in range(L) for kind in (0, 1)]
    srcs = [d.data_ptr() + (layer * 2 + kind) * n * ROW for layer in range(L) for kind in (0, 1)]
    torch.cuda.synchronize()
    lib.write_runs(twin, firsts, srcs, n // 2, stream.cuda_stream)
    stream.synchronize()


def _compare_allocations(lib, torch, h, tw, scheme, st, what):
    """decoded bits, rec_bytes, scale and stored record bytes of every page; the FP16 scheme stores the conversion itself, so there a
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


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_write_ex_from_bf16_is_write_runs_of_the_converted_rows(scheme, mode):
    """bf16 caches that hold random rows, every bf16 pattern, zeros, constant runs, inf and NaN: rec_bytes, scale, record bytes and
    decoded bits are those of twins written by write_runs from the restatement of the same rows laid contiguous; both wave orders; a
    -1 slot and one >= n_slots store the record of a zero row; the caches are unchanged."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        content = _bf16_content(50 + scheme)
        flat16 = bf16_to_fp16_bits(content).reshape(L, 2, (NB + 2) * BS, HALF)
        assert fp16_is_nan(flat16[:, :, BS + 68]).any() and (flat16[0, 0, BS + 71] == 0).all()
        rng = np.random.default_rng(7)
        slots = np.concatenate([np.arange(64), 72 + rng.permutation(N_SLOTS - 72)[:26], np.arange(64, 72)]).astype(np.int64)
        slots[64 + 7] = -1
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
            lib.write_slots_ex(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream, elem=BF16)
            st.synchronize()
            assert lib.stats().total_compressions - before == 2 * L * sum(n // 2 for _, _, n in WRITE_SPANS)
            assert np.array_equal(_host(caches).reshape(content.shape), content), "write_slots_ex changed the caches"
            keep = []
            for (a, first, n), b in zip(WRITE_SPANS, bs):
                rows = np.zeros((L, 2, n, HALF), dtype=np.uint16)
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        rows[:, :, t] = flat16[:, :, BS + s]
                _twin_runs(lib, torch, twins[a], first, rows, st, keep)
            for h, tw in zip(handles, twins):
                image = _compare_allocations(lib, torch, h, tw, scheme, st, (scheme, mode, kind_fast))
            if scheme == 0:                                                 # the records show the conversion itself
                got = _image(lib, torch, handles[0], st)
                for i in range(64):
                    want = flat16[0, 0, BS + i]
                    assert equal_off_nan(_row(got, 0, 0, i), want, fp16_is_nan(want), fp16_is_nan), i
            image = _image(lib, torch, handles[1], st)
            for layer in range(L):
                for kind in (0, 1):
                    assert not _row(image, layer, kind, 6 + 7).any() and not _row(image, layer, kind, 6 + 20).any()
            assert image[3].any() and not image[STEP - 1].any()
            for h in handles + twins:
                lib.free(h)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


@pytest.mark.parametrize("scheme", [2, 5])
def test_fp16_without_held_rows_is_the_existing_entry(scheme):
    """elem = FP16 and no held arrays: caches, pool records and stats equal those of speckv_ext_read_slots / _write_slots"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        st = torch.cuda.Stream()
        content = _random_content(21)
        src = _caches(torch, content)
        spans = [(0, 0, 34), (1, 6, 26), (0, 40, 2)]
        slots = np.random.default_rng(2).permutation(N_SLOTS)[:62].astype(np.int64)
        slots[[5, 40]] = -1, N_SLOTS + 2
        d_slots = torch.from_numpy(slots).cuda()
        sides, deltas = [], []
        for entry in (lib.write_slots, lib.write_slots_ex):
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            hs, fs, ns, bs = _span_args(handles, spans)
            before = lib.stats()
            torch.cuda.synchronize()
            entry(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(src), 0, _kind_stride(src), STEP, st.cuda_stream)
            st.synchronize()
            after = lib.stats()
            deltas.append((after.total_compressions - before.total_compressions, after.original_bytes - before.original_bytes))
            sides.append(handles)
        assert deltas[0] == deltas[1] and deltas[0][0] == 2 * L * 31
        for h, tw in zip(*sides):
            _compare_allocations(lib, torch, h, tw, scheme, st, "write_slots_ex with elem = FP16")
        rspans = SPANS
        rslots = np.random.default_rng(3).permutation(N_SLOTS)[:62].astype(np.int64)
        rslots[[3, 60, 31]] = -1, -1, N_SLOTS + 3
        d_r = torch.from_numpy(rslots).cuda()
        hs, fs, ns, bs = _span_args(sides[0] + [sides[1][0]], rspans)
        outs, deltas = [], []
        for entry in (lib.read_slots, lib.read_slots_ex):
            dst = _caches(torch)
            before = lib.stats()
            torch.cuda.synchronize()
            entry(hs, fs, ns, bs, d_r.data_ptr(), N_SLOTS, _bases(dst), 0, _kind_stride(dst), STEP, st.cuda_stream)
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
def test_read_ex_takes_a_spans_last_position_from_its_held_row(scheme, elem):
    """spans that end on a held position -- [0, 35), [32, 33) (n = 1) and [40, 43) whose held position has slot -1 -- beside [5, 32)
    and [64, 64) without one: the held rows arrive in their slots (converted for bf16), everything else is fetch_range's image, the
    pages of the held positions are not counted, the held rows and everything else keep their bits"""
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
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _caches(torch)
            want = _host(caches)
            for i, ((a, first, n), b) in enumerate(zip(spans, bs)):
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        for layer in range(L):
                            for kind in (0, 1):
                                row = _row(images[a], layer, kind, first + t)
                                if has[i] and t == n - 1:
                                    row = (hk_host, hv_host)[kind][1 + i, layer]
                                want[layer, kind, BS + s] = _to_cache(row, elem)
            before = lib.stats().total_decompressions
            torch.cuda.synchronize()
            lib.read_slots_ex(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                              elem=elem, held_in=held, held_stride=ROW)
            st.synchronize()
            got = _host(caches)
            assert np.array_equal(got, want), (scheme, elem, kind_fast, np.argwhere((got != want).any(axis=-1))[:8])
            assert lib.stats().total_decompressions - before == 2 * L * (17 + 14 + 0 + 1)
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
def test_write_ex_with_held_rows_in_one_call(scheme, elem):
    """every odd edge in one call, from fp16 and from bf16 caches (then a pair made of a held fp16 row and a bf16 cache row is
    mixed): the pool equals twins written by write_runs from the same positions, the held-out rows are the fp16 of the last
    positions, everything around them, the held-in rows and the caches keep their bits"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        st = torch.cuda.Stream()
        content = _random_content(60 + scheme)
        if elem == BF16:
            content = (content.view(np.float16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
            content[0, 1, 5, 2, 100:104] = (0x7F80, 0x7FC0, 0xFF80, 0x0001)     # a bf16 row with inf / NaN beside a held fp16 row
        flat16 = _from_cache(content, elem).reshape(L, 2, (NB + 2) * BS, HALF)
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
            lib.write_slots_ex(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                               elem=elem, held_in=h_in, held_stride=ROW, held_out=h_out)
            st.synchronize()
            assert lib.stats().total_compressions - before == 2 * L * (3 + 3 + 2 + 1 + 0 + 3 + 0)
            keep = []
            for i, ((a, first, n, hin, hout), b) in enumerate(zip(HELD_WRITES, bs)):
                rows = []
                if hin:
                    rows.append(np.stack([ik_host[1 + i], iv_host[1 + i]], axis=1))          # [L][2][1024]
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
            assert np.array_equal(_host(caches).reshape(content.shape), content), "write_slots_ex changed the caches"
            for h in handles + twins:
                lib.free(h)
        assert np.array_equal(ik.cpu().numpy().view(np.uint16), ik_host) and np.array_equal(iv.cpu().numpy().view(np.uint16), iv_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_ex_entries_launches_nothing():
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
        good = dict(handles=u64(h), firsts=u64(0), counts=u64(8), begins=u64(0), slots=d_slots.data_ptr(), n_slots=N_SLOTS, bases=bases,
                    layer_begin=0, ks=ks, step=STEP, stream=s, elem=BF16, held_in=None, held_stride=ROW, held_out=None, reserved=0)
        inval = [
            dict(stream=0), dict(slots=0), dict(bases=u64(bases[0], 0)), dict(bases=u64(bases[0], bases[1] + 8)), dict(ks=ks + 8), dict(step=0),
            dict(handles=u64(h, other), firsts=u64(0, 0), counts=u64(8, 8), begins=u64(0, 8)),          # allocations of different schemes
            dict(elem=2), dict(elem=0xFFFFFFFF), dict(reserved=1),                                      # an unknown elem, reserved != 0
            dict(held_stride=ROW + 8),                                                                  # a stride that is no multiple of 16
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
            dict(handles=u64(h, h), firsts=u64(0, 6), counts=u64(8, 4), begins=u64(0, 8)),              # two spans share a page ...
            dict(handles=u64(h, h), firsts=u64(0, 7), counts=u64(8, 3), begins=u64(0, 8),               # ... through the held-in pair
                 held_in=u64(0, 0, *one((ik, iv), 1))),
        ]
        general = [dict(handles=u64(h + 12345)), dict(firsts=u64(2 * STEP - 4)), dict(step=N_PAGES), dict(layer_begin=1)]

        def call(entry, a):
            entry(a["handles"], a["firsts"], a["counts"], a["begins"], a["slots"], a["n_slots"], a["bases"], a["layer_begin"], a["ks"],
                  a["step"], a["stream"], elem=a["elem"], held_in=a["held_in"], held_stride=a["held_stride"], held_out=a["held_out"],
                  reserved=a["reserved"])

        def untouched():
            torch.cuda.synchronize()
            assert np.array_equal(_host(caches), pattern), "a refused call wrote to the caches"
            assert np.array_equal(_image(lib, torch, h, st), image) and not _image(lib, torch, h2, st).any(), "a refused call wrote to the pool"
            assert np.array_equal(ok.cpu().numpy().view(np.uint16), ok_host) and np.array_equal(ov.cpu().numpy().view(np.uint16), ov_host), \
                "a refused call wrote to the held-out rows"

        for entry, cases in ((lib.read_slots_ex, [(-4, inval + read_inval), (-1, general)]),
                             (lib.write_slots_ex, [(-4, inval + write_inval), (-1, general)])):
            for status, group in cases:
                for case in group:
                    a = dict(good)
                    a.update(case)
                    with pytest.raises(SpeckvError) as e:
                        call(entry, a)
                    assert e.value.status == status, (entry.__name__, case, e.value.status)
            untouched()
        for name in ("speckv_ext_read_slots_ex", "speckv_ext_write_slots_ex"):                         # no options at all
            with pytest.raises(SpeckvError) as e:
                lib._ext(name, u64(h).ctypes.data, u64(0).ctypes.data, u64(8).ctypes.data, u64(0).ctypes.data, 1, d_slots.data_ptr(), N_SLOTS,
                         bases.ctypes.data, 0, L, ks, STEP, None, s)
            assert e.value.status == -4, name
        untouched()
        bump = torch.zeros(4, device="cuda")                                # a capturing stream: the descriptors are staged per call
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            for entry, case in ((lib.read_slots_ex, dict(counts=u64(9), held_in=IN)), (lib.write_slots_ex, dict(counts=u64(7), held_out=OUT))):
                with pytest.raises(SpeckvError) as e:
                    call(entry, dict(good, **case))
                assert e.value.status == -4
            bump.add_(1)
        g.replay()
        untouched()
        del g
        for entry in (lib.read_slots_ex, lib.write_slots_ex):             # nothing to do: fine
            call(entry, dict(good, handles=u64(), firsts=u64(), counts=u64(), begins=u64()))
            call(entry, dict(good, bases=u64()))
            call(entry, dict(good, handles=u64(h, h2), firsts=u64(0, 64), counts=u64(0, 0), begins=u64(0, 0)))
        untouched()
        call(lib.read_slots_ex, dict(good, counts=u64(9), held_in=IN))    # ... and the good calls do their work
        st.synchronize()
        got = _host(caches)
        for t in range(8):
            assert np.array_equal(got[1, 1, BS + t], fp16_to_bf16_bits(_row(image, 1, 1, t)))
        assert np.array_equal(got[1, 1, BS + 8], fp16_to_bf16_bits(iv.cpu().numpy().view(np.uint16)[1, 1]))
        call(lib.write_slots_ex, dict(good, handles=u64(h2), counts=u64(7), held_out=OUT))
        st.synchronize()
        assert _image(lib, torch, h2, st)[:3].any() and not _image(lib, torch, h2, st)[3].any()
        assert not np.array_equal(ok.cpu().numpy().view(np.uint16)[1], ok_host[1])
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ placement
def _held_write_against_twin(lib, torch, h, tw, scheme, st, seed):
    """one write_slots_ex from bf16 caches with a held-in and a held-out row -- positions [3, 9) of h: pairs 1 .. 3 -- and the same
    positions by write_runs into tw; returns the expected held-out rows check"""
    content = (_random_content(seed).view(np.float16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    flat16 = bf16_to_fp16_bits(content).reshape(L, 2, (NB + 2) * BS, HALF)
    caches = _caches(torch, content)
    slots = np.asarray([30, 31, 32, 33, 34, 35], dtype=np.int64)
    d_slots = torch.from_numpy(slots).cuda()
    (ik, ik_host), (iv, iv_host) = _held_block(torch, 1, seed + 1), _held_block(torch, 1, seed + 2)
    (ok, _), (ov, _) = _held_block(torch, 1), _held_block(torch, 1)
    torch.cuda.synchronize()
    lib.write_slots_ex(u64(h), u64(3), u64(6), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                       elem=BF16, held_in=_held_ptrs((ik, iv), [True], 1), held_stride=ROW, held_out=_held_ptrs((ok, ov), [True], 1))
    st.synchronize()
    rows = [np.stack([ik_host[1], iv_host[1]], axis=1)] + [flat16[:, :, BS + int(s)] for s in slots[:5]]
    keep = []
    _twin_runs(lib, torch, tw, 2, np.stack(rows, axis=2), st, keep)
    assert np.array_equal(ok.cpu().numpy().view(np.uint16)[1], flat16[:, 0, BS + 35]) and np.array_equal(ov.cpu().numpy().view(np.uint16)[1], flat16[:, 1, BS + 35])


def test_placement_striped_migrated_sealed_and_cached_with_bf16_and_held_rows():
    torch = torch_mod()
    for scheme in (4, 5):
        lib = open_lib(SPECKV_POOL_DEVICES="0,0,0")
        try:
            lib.set_compression_scheme(scheme)
            h, tw = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
            for a in (h, tw):
                _fill(lib, a, _blocks(N_PAGES, 40))
            lib.migrate(h, 1, 4, 1)                                       # pages 1 .. 4 and a page of another region now lie elsewhere
            lib.migrate(h, 2 * STEP + 15, 3, 2)
            st = torch.cuda.Stream()
            _held_write_against_twin(lib, torch, h, tw, scheme, st, 80)
            got, want = _image(lib, torch, h, st), _image(lib, torch, tw, st)
            assert np.array_equal(got, want), ("striped / migrated write", scheme)
            # ... and read back into bf16 blocks with position 8 from a held row
            caches = _caches(torch)
            want_c = _host(caches)
            d_slots = torch.arange(40, 47, dtype=torch.int64, device="cuda")
            (ik, ik_host), (iv, iv_host) = _held_block(torch, 1, 5), _held_block(torch, 1, 6)
            for t in range(7):
                for layer in range(L):
                    for kind in (0, 1):
                        row = _row(got, layer, kind, 2 + t) if t < 6 else (ik_host, iv_host)[kind][1, layer]
                        want_c[layer, kind, BS + 40 + t] = fp16_to_bf16_bits(row)
            torch.cuda.synchronize()
            lib.read_slots_ex(u64(h), u64(2), u64(7), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP,
                              st.cuda_stream, elem=BF16, held_in=_held_ptrs((ik, iv), [True], 1), held_stride=ROW)
            st.synchronize()
            assert np.array_equal(_host(caches), want_c), ("striped / migrated read", scheme)
        finally:
            lib.finalize()
    lib = open_lib()
    try:
        lib.set_compression_scheme(2)
        h, tw, h3 = (lib.alloc(N_PAGES * PAGE) for _ in range(3))
        for a in (h, tw, h3):
            _fill(lib, a, _blocks(N_PAGES, 60))
        lib.compact(h)
        lib.compact(h3)
        assert lib.stats().sealed_allocations == 2
        st = torch.cuda.Stream()
        image = _image(lib, torch, h, st)
        caches = _caches(torch)
        want_c = _host(caches)
        d_slots = torch.arange(10, 15, dtype=torch.int64, device="cuda")
        (ik, ik_host), (iv, iv_host) = _held_block(torch, 1, 5), _held_block(torch, 1, 6)
        for t in range(5):
            for layer in range(L):
                for kind in (0, 1):
                    row = _row(image, layer, kind, 10 + t) if t < 4 else (ik_host, iv_host)[kind][1, layer]
                    want_c[layer, kind, BS + 10 + t] = fp16_to_bf16_bits(row)
        torch.cuda.synchronize()
        lib.read_slots_ex(u64(h), u64(10), u64(5), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP,
                          st.cuda_stream, elem=BF16, held_in=_held_ptrs((ik, iv), [True], 1), held_stride=ROW)
        st.synchronize()
        assert np.array_equal(_host(caches), want_c) and lib.stats().sealed_allocations == 2, "read_slots_ex leaves a sealed allocation sealed"
        _held_write_against_twin(lib, torch, h, tw, 2, st, 81)
        assert lib.stats().sealed_allocations == 1, "an odd write_slots_ex unpacks a sealed destination"
        assert np.array_equal(_image(lib, torch, h, st), _image(lib, torch, tw, st))
        # a page cached by speckv_access before the write
        page = 3 * STEP + 2                                            # layer 1, V, positions 4 and 5
        h4, tw4 = lib.alloc(N_PAGES * PAGE), lib.alloc(N_PAGES * PAGE)
        for a in (h4, tw4):
            _fill(lib, a, _blocks(N_PAGES, 61))
        ptr = lib.access(h4, page * PAGE, 64)
        old = dev_to_host(ptr, PAGE).view(np.uint16).copy()
        assert lib.translate(h4, page * PAGE).flags & 3
        _held_write_against_twin(lib, torch, h4, tw4, 2, st, 82)
        new = dev_to_host(lib.access(h4, page * PAGE, 64), PAGE).view(np.uint16)
        want = _image(lib, torch, tw4, st)[page]
        assert np.array_equal(new, want) and not np.array_equal(new, old), "a cached page shows the bytes of before the write"
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------- ordering
@pytest.mark.parametrize("scheme", [2, 4])
def test_ordering_of_the_ex_entries_on_one_stream_and_across_streams(scheme):
    """write_slots_ex then read_slots_ex on one busy, non-current stream with nothing between them, and a read on stream B behind a
    write on stream A: the read returns what was written, the held-out row of the write included (it is the read's held-in row)"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        content = (_random_content(31).view(np.float16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        n = 63
        slots = np.random.default_rng(3).permutation(N_SLOTS)[:n].astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        out_slots = torch.from_numpy(np.arange(n, dtype=np.int64)).cuda()
        flat16 = bf16_to_fp16_bits(content).reshape(L, 2, (NB + 2) * BS, HALF)
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
            lib.write_slots_ex(u64(h), u64(0), u64(n), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(src), 0, _kind_stride(src), STEP, a.cuda_stream,
                               elem=BF16, held_out=tail, held_stride=ROW)
            rs = b if two_streams else a
            if two_streams:
                b.wait_stream(a)                                       # the held row is the caller's memory: the caller orders it
            lib.read_slots_ex(u64(h), u64(0), u64(n), u64(0), out_slots.data_ptr(), N_SLOTS, _bases(dst), 0, _kind_stride(dst), STEP, rs.cuda_stream,
                              elem=BF16, held_in=tail, held_stride=ROW)
            torch.cuda.synchronize()
            image = _image(lib, torch, h, a)
            got = _host(dst)
            assert image[0].any()
            for layer in range(L):
                for kind in (0, 1):
                    for t in range(n - 1):
                        assert np.array_equal(got[layer, kind, BS + t], fp16_to_bf16_bits(_row(image, layer, kind, t))), (two_streams, layer, kind, t)
                    assert np.array_equal(got[layer, kind, BS + n - 1], fp16_to_bf16_bits(flat16[layer, kind, BS + int(slots[n - 1])]))
    finally:
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------- the connector
class _CountingEx(_Counting):
    NAMES = _Counting.NAMES + ("read_slots_ex", "write_slots_ex", "write_strided", "write_strided_batch")


def _typed_caches(torch, content, elem):
    """_caches with the views typed by `elem`"""
    return [(big, big.view(torch.bfloat16)[:, 1:-1] if elem == BF16 else view) for big, view in _caches(torch, content)]


def _cache_content(seed, elem):
    c = _random_content(seed)
    return (c.view(np.float16).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) if elem == BF16 else c


CHUNKS = (5, 1, 1, 2, 3, 21)


@pytest.mark.parametrize("elem", [FP16, BF16])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_connector_chunked_store_append_and_load(scheme, elem):
    """A request built by store_paged(fused=True) in chunks of 5, 1, 1, 2, 3 and 21 positions against a twin built by write_prefill +
    append from the same rows (the restatement's fp16 for bf16 caches): attend out and lse equal to the bit after every chunk, kv_rows
    at the end; one library call per store_paged / load_paged; a lockstep append straight after a fused store pairs the batched
    tails; load_paged(fused=True) equals the row route of the same tree, for odd ends and a tail."""
    torch = torch_mod()
    lib = _CountingEx(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        rng = np.random.default_rng(41)
        paged, twin = SpeckvKVConnector(lib, L, H, D, T, scheme), SpeckvKVConnector(lib, L, H, D, T, scheme)
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
            keep += paged.store_paged([1], [c], _dev(torch, maps[1][at:at + c]), caches, fused=True)
            assert lib.calls == ["write_slots_ex"], lib.calls
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
        keep += paged.store_paged([2, 1], [7, 2], _dev(torch, np.concatenate([maps[2][:7], maps[1][33:35]])), caches, fused=True)
        assert lib.calls == ["write_slots_ex"], lib.calls
        k2, v2 = rows[2]
        keep += twin.write_prefill(102, k2[:, :7].contiguous(), v2[:, :7].contiguous())
        for t in (33, 34):
            keep.append(twin.append([101], rows[1][0][:, t][None].contiguous(), rows[1][1][:, t][None].contiguous()))
        assert paged._tail_ids == (2, 1) and tuple(paged._tail_k.shape) == (2, L, H, D)
        tail_k = paged._tail_k
        k_new, v_new = _dev(torch, rng.standard_normal((2, L, H, D)).astype(np.float16)), _dev(torch, rng.standard_normal((2, L, H, D)).astype(np.float16))
        lib.calls.clear()
        keep.append(paged.append([2, 1], k_new, v_new))
        assert lib.calls == ["write_strided_batch"] and paged._tail_ids == () and tail_k is not None
        keep.append(twin.append([102, 101], k_new, v_new))
        attend_equal([2, 1], [102, 101], "lockstep append after a fused store")
        for rid, tid in zip(ids, tids):
            assert paged.length(rid) == twin.length(tid)
            assert all(np.array_equal(x, y) for x, y in zip(_all_rows(paged, rid), _all_rows(twin, tid))), (scheme, elem, rid, "after the append")
        # ---- one more position each (tails again), then load into fresh blocks of the same type: against the row route
        keep += paged.store_paged([1, 2], [1, 1], _dev(torch, np.concatenate([maps[1][36:37], maps[2][8:9]])), caches, fused=True)
        assert paged.length(1) == 37 and paged.length(2) == 9
        loads = [(1, 3, 34), (2, 1, 6), (1, 0, 37), (2, 8, 1)]          # odd ends up to the tail; odd ends; a whole request; only the tail
        lmap = rng.permutation(N_SLOTS).astype(np.int64)[:sum(n for _, _, n in loads)]
        lmap[5] = -1
        d_lmap = _dev(torch, lmap)
        fresh, ref = _typed_caches(torch, None, elem), _typed_caches(torch, None, elem)
        torch.cuda.synchronize()
        lib.calls.clear()
        paged.load_paged([r for r, _, _ in loads], [f for _, f, _ in loads], [n for _, _, n in loads], d_lmap, [v for _, v in fresh], fused=True)
        torch.cuda.synchronize()
        assert lib.calls == ["read_slots_ex"], lib.calls
        at = 0
        for rid, f, n in loads:                                            # the row route, and its rule for bf16: kv_rows restated
            for layer, (big, _) in enumerate(ref):
                for kind in (0, 1):
                    rows_ = _to_cache(_bits(paged.kv_rows(rid, layer, kind, f, f + n)), elem).view(np.int16)        # [n][H][D]
                    for t in range(n):
                        s = int(lmap[at + t])
                        if s >= 0:
                            big[kind, 1 + s // BS, s % BS] = _dev(torch, rows_[t])
            at += n
        torch.cuda.synchronize()
        assert np.array_equal(_host(fresh), _host(ref)), (scheme, elem, "load_paged(fused=True) is not the restated row route")
        route = _typed_caches(torch, None, elem)                           # ... and the row route itself (a device cast for bf16)
        keep_map = d_lmap.clone()
        keep_map[5] = int(lmap[4])                                         # (index_copy_ takes no -1: the row is written twice instead)
        paged.load_paged([r for r, _, _ in loads], [f for _, f, _ in loads], [n for _, _, n in loads], keep_map, [v for _, v in route], fused=False)
        torch.cuda.synchronize()
        got, want = _host(fresh), _host(route)
        s4 = BS + int(lmap[4])
        got[:, :, s4] = want[:, :, s4] = 0
        assert np.array_equal(got, want), (scheme, elem, "load_paged(fused=True) is not the row route")
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------- the adapter
def test_adapter_paged_fused_on_bf16_equals_the_row_route():
    """the walk of test_adapter_paged_io_equals_the_row_route on bf16 caches: paged_io=True, paged_fused=True against paged_io=False --
    store, freed blocks, a prefix hit, a resumed request, a foreign kv_layer; caches and pools equal to the bit after every step, one
    _ex call per step on the fused side"""
    torch = torch_mod()
    from types import SimpleNamespace as NS
    from cxl_speckv_amd.vllm_connector import SpeckvVllmConnector, slot_mapping_for
    lib = _CountingEx(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        names = [f"model.layers.{i}.self_attn.attn" for i in range(L)]
        sides = {}
        for paged in (True, False):
            c = SpeckvVllmConnector(lib, num_layers=L, num_kv_heads=H, head_dim=D, block_size=BS, max_tokens=T, scheme="fp8", paged_io=paged,
                                    paged_fused=paged)
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

        rows = {(rid, li): torch.randn((2, n, H, D), generator=gen, device="cuda").to(torch.bfloat16) for rid, (n, _) in prompts.items() for li in range(L)}

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
                    assert lib.calls == ["write_slots_ex"], lib.calls
                if paged and foreign:
                    assert "write_slots_ex" not in lib.calls and lib.calls.count("write_runs") == len(rids), lib.calls
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
                    assert lib.calls == ["read_slots_ex"], (what, lib.calls)
                else:
                    assert "read_slots_ex" not in lib.calls and "read_slots" not in lib.calls
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
        same("an odd prompt stored by the fused launch")
        load(["req-d"], {"req-d": [7, 3, 9]}, 0, False, "load of the odd prompt")
    finally:
        lib.finalize()


def test_the_bf16_example_runs():
    """examples/paged_cache_bf16_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "paged_cache_bf16_example.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "paged cache bf16 example ok" in out.stdout
