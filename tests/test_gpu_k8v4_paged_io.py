"""-m gpu: paged-cache transfers of the split pool ("K8V4") -- speckv_ext_read_slots_kv / speckv_ext_write_slots_kv (one launch over
a request's FP8_E4M3 K allocation and its MXFP4 V allocation) and SpeckvSplitKVConnector.load_paged / store_paged / kv_rows.

References: speckv_ext_fetch_range of the K allocation for the K plane of a slot and of the V allocation for the V plane (through the
numpy restatement fp16_to_bf16_bits for bf16 caches); for a write, twin allocations written by speckv_ext_write_runs from the same
rows laid out contiguously (the restatement bf16_to_fp16_bits of bf16 rows): rec_bytes, stored record bytes, decoded bits, and the
entry's scale for the FP8 allocation -- an MXFP4 entry's scale word is the offset of its code plane, which stored_record follows.
Every comparison is exact.

Geometry and helpers are those of tests/test_gpu_paged_io.py (L = 2, T = 128: page_step 64, blocks of 16 slots, 12 blocks, caches
between guard blocks, n_slots one block short); a split request is what SpeckvSplitKVConnector.add_request makes: two allocations of
L regions of 64 pages, 128 pages each.  Pool contents follow tests/_k8v4_cases.py: every MXFP4 (page, head, block) its own power of
two, every FP8 page its own factor, K and V from different seeds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, graph_capture, set_tuning, stored_record, torch_mod
from tests._k8v4_cases import content
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_paged_io import (BS, L, N_SLOTS, NB, PAGE, ROOT, ROW, SPANS, STEP, T, _bases, _bits, _Counting, _dev, _host, _kind_stride,
                                     _slot_list, u64)
from tests.test_gpu_paged_io_fused import (BF16, FP16, HALF, HELD_WRITES, _bf16_content, _cache_content, _from_cache, _held_block, _held_ptrs,
                                           _to_cache, _typed_caches)
from tests.test_paged_io_fused_cpu import bf16_to_fp16_bits, equal_off_nan, fp16_is_nan

pytestmark = pytest.mark.gpu
KV_PAGES = L * STEP                             # pages of either allocation of a split request
SM = 1.0 / np.sqrt(D)


class _CountingKV(_Counting):
    NAMES = _Counting.NAMES + ("read_slots_kv", "write_slots_kv", "read_slots_ex", "write_slots_ex", "write_pairs")


def _fill_kv(lib, h, x, hole=None):
    """every page of a single-kind allocation from x [KV_PAGES][2048] fp16, except page `hole` of every layer's region"""
    x = np.ascontiguousarray(x).reshape(KV_PAGES, ROW)
    for layer in range(L):
        lo, hi = layer * STEP, (layer + 1) * STEP
        parts = ((lo, hi),) if hole is None else ((lo, lo + hole), (lo + hole + 1, hi))
        for a, b in parts:
            part = np.ascontiguousarray(x[a:b])
            lib.write(h, a * PAGE, part.ctypes.data, part.nbytes, False)


def _pool(lib, conn, ids, seed, hole=8):
    """split requests `ids` whose K allocations hold content(seed + i)'s K and whose V allocations content(seed + 50 + i)'s V;
    -> [(K handle, V handle)]"""
    pairs = []
    for i, rid in enumerate(ids):
        kh, vh = conn.add_request(rid)
        _fill_kv(lib, kh, content(seed + i, T)[0], hole)
        _fill_kv(lib, vh, content(seed + 50 + i, T)[1], hole)
        pairs.append((kh, vh))
    return pairs


def _image_kv(lib, torch, h, stream):
    out = torch.empty((KV_PAGES, ROW), dtype=torch.float16, device="cuda")
    lib.fetch_range(h, 0, KV_PAGES, out.data_ptr(), False, stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy().view(np.uint16)


def _row_kv(image, layer, pos):
    return image[layer * STEP + pos // 2].reshape(2, HALF)[pos & 1]


def _kv_span_args(pairs, spans):
    begins = np.cumsum([0] + [n for _, _, n in spans])[:-1]
    return (u64(*[pairs[a][0] for a, _, _ in spans]), u64(*[pairs[a][1] for a, _, _ in spans]), u64(*[f for _, f, _ in spans]),
            u64(*[n for _, _, n in spans]), u64(*begins))


def _twin_runs_kv(lib, torch, twin, first_pos, rows16, stream, keep):
    """write_runs of rows16 [L][2][n][1024] fp16 bits (n even) at position first_pos (even): the K rows into twin[0], the V rows into
    twin[1], one call each"""
    n = rows16.shape[2]
    assert n % 2 == 0 and first_pos % 2 == 0
    d = torch.from_numpy(np.ascontiguousarray(rows16).view(np.int16)).cuda()
    keep.append(d)
    torch.cuda.synchronize()
    for kind in (0, 1):
        lib.write_runs(twin[kind], [layer * STEP + first_pos // 2 for layer in range(L)],
                       [d.data_ptr() + (layer * 2 + kind) * n * ROW for layer in range(L)], n // 2, stream.cuda_stream)
    stream.synchronize()


def _compare_kv(lib, torch, pair, twin, st, what):
    """every page of both allocations: decoded bits, rec_bytes, the FP8 entry's scale, the stored record bytes"""
    for kind, (h, tw) in enumerate(zip(pair, twin)):
        got, want = _image_kv(lib, torch, h, st), _image_kv(lib, torch, tw, st)
        nan = fp16_is_nan(want)
        assert equal_off_nan(got, want, nan, fp16_is_nan), (what, kind, "decoded bits", np.argwhere(((got != want) & ~nan).any(axis=-1))[:8])
        for p in range(KV_PAGES):
            a, b = lib.translate(h, p * PAGE), lib.translate(tw, p * PAGE)
            assert a.rec_bytes == b.rec_bytes, (what, kind, p, a.rec_bytes, b.rec_bytes)
            assert a.scheme == b.scheme == (5 if kind else 4), (what, kind, p)
            if kind == 0:
                assert np.float32(a.scale).view(np.uint32) == np.float32(b.scale).view(np.uint32), (what, p, "scale")
            if a.rec_bytes:
                assert np.array_equal(stored_record(a, a.rec_bytes), stored_record(b, b.rec_bytes)), (what, kind, p, "record bytes")


# ---------------------------------------------------------------------------------------------------------------------- read
@pytest.mark.parametrize("kind_fast", [0, 1])
@pytest.mark.parametrize("elem", [FP16, BF16])
def test_read_kv_is_fetch_range_of_each_allocation(elem, kind_fast):
    """Spans [0, 34), [5, 32), [33, 34), [64, 64) over three split requests, two slots -1 and one >= n_slots, page 8 of every region
    never written: the caches, guards included, are the K planes from fetch_range of the K allocations and the V planes from
    fetch_range of the V allocations (restated for bf16); then layers [1, 2) alone."""
    torch = torch_mod()
    lib = open_lib()
    try:
        set_tuning("slots_kind_fast", kind_fast)
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        pairs = _pool(lib, conn, [0, 1, 2], 9100)
        st = torch.cuda.Stream()
        images = [[_image_kv(lib, torch, h, st) for h in pair] for pair in pairs]                    # [request][kind]
        assert not images[0][0][8].any() and not images[1][1][STEP + 8].any() and images[0][0][0].any() and images[0][1][9].any()
        assert not np.array_equal(images[0][0], images[0][1])
        total = sum(n for _, _, n in SPANS)
        slots = _slot_list(np.random.default_rng(5), total)
        d_slots = torch.from_numpy(slots).cuda()
        ks, vs, fs, ns, bs = _kv_span_args(pairs, SPANS)
        for layer_begin, n_layers in ((0, L), (1, 1)):
            caches = _typed_caches(torch, None, elem)
            used = caches[layer_begin:layer_begin + n_layers]
            want = _host(caches)
            zeros = 0
            for (a, first, n), b in zip(SPANS, bs):
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        for layer in range(layer_begin, layer_begin + n_layers):
                            for kind in (0, 1):
                                row = _row_kv(images[a][kind], layer, first + t)
                                want[layer, kind, BS + s] = _to_cache(row, elem)
                                zeros += (first + t) // 2 == 8 and not want[layer, kind, BS + s].any()
            assert zeros == 2 * 2 * 2 * n_layers                                   # positions 16, 17 of two spans: the never-written page
            before = lib.stats()
            torch.cuda.synchronize()
            lib.read_slots_kv(ks, vs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(used), layer_begin, _kind_stride(caches), STEP,
                              st.cuda_stream, elem=elem)
            st.synchronize()
            got = _host(caches)
            assert np.array_equal(got, want), (elem, kind_fast, layer_begin, np.argwhere((got != want).any(axis=-1))[:8])
            pages = 2 * n_layers * sum((f + n + 1) // 2 - f // 2 for _, f, n in SPANS if n)
            after = lib.stats()
            assert after.total_decompressions - before.total_decompressions == pages and after.dma_completed - before.dma_completed == pages
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


@pytest.mark.parametrize("elem", [FP16, BF16])
def test_read_kv_takes_a_spans_last_position_from_its_held_row(elem):
    """spans that end on a held (even) position -- [0, 35), [32, 33) and [40, 43) whose held position has slot -1 -- beside [5, 32)
    and [64, 64) without one, both wave orders: the held rows arrive in their slots (converted for bf16), everything else is
    fetch_range's image of its allocation, the pages of the held positions are not counted, the held blocks keep their bits"""
    torch = torch_mod()
    lib = open_lib()
    try:
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        pairs = _pool(lib, conn, [0, 1, 2], 9120)
        st = torch.cuda.Stream()
        images = [[_image_kv(lib, torch, h, st) for h in pair] for pair in pairs]
        spans = [(0, 0, 35), (1, 5, 27), (2, 32, 1), (0, 40, 3), (1, 64, 0)]
        has = [True, False, True, True, False]
        ks, vs, fs, ns, bs = _kv_span_args(pairs, spans)
        slots = np.random.default_rng(8).permutation(N_SLOTS)[:66].astype(np.int64)
        slots[[3, 50]] = -1
        slots[20] = N_SLOTS + 3
        slots[int(bs[3]) + 2] = -1                                            # the held position of [40, 43) has no row
        d_slots = torch.from_numpy(slots).cuda()
        (hk, hk_host), (hv, hv_host) = _held_block(torch, len(spans), 90), _held_block(torch, len(spans), 91)
        held = _held_ptrs((hk, hv), has, len(spans))
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _typed_caches(torch, None, elem)
            want = _host(caches)
            for i, ((a, first, n), b) in enumerate(zip(spans, bs)):
                for t in range(n):
                    s = int(slots[int(b) + t])
                    if 0 <= s < N_SLOTS:
                        for layer in range(L):
                            for kind in (0, 1):
                                row = _row_kv(images[a][kind], layer, first + t)
                                if has[i] and t == n - 1:
                                    row = (hk_host, hv_host)[kind][1 + i, layer]
                                want[layer, kind, BS + s] = _to_cache(row, elem)
            before = lib.stats().total_decompressions
            torch.cuda.synchronize()
            lib.read_slots_kv(ks, vs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
                              elem=elem, held_in=held, held_stride=ROW)
            st.synchronize()
            got = _host(caches)
            assert np.array_equal(got, want), (elem, kind_fast, np.argwhere((got != want).any(axis=-1))[:8])
            assert lib.stats().total_decompressions - before == 2 * L * (17 + 14 + 0 + 1)
        assert np.array_equal(hk.cpu().numpy().view(np.uint16), hk_host) and np.array_equal(hv.cpu().numpy().view(np.uint16), hv_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------------- write
def _fp16_content(seed):
    """_bf16_content for fp16 caches: [L][2][NB + 2][BS][1024] fp16 bits, random rows everywhere; slots 0 .. 63 hold every fp16
    pattern; slots 64 .. 71 a page of zeros, a page of constant runs, a page with inf and NaN in random rows, a page of -0 and
    subnormals"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((L, 2, NB + 2, BS, HALF)).astype(np.float16).view(np.uint16)
    flat = c.reshape(L, 2, (NB + 2) * BS, HALF)
    flat[:, :, BS:BS + 64] = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(64, HALF)
    flat[:, :, BS + 64:BS + 66] = 0
    flat[:, :, BS + 66] = np.repeat(flat[:, :, BS + 66, :32], 32, axis=-1)
    flat[:, :, BS + 67] = flat[:, :, BS + 67, :1]
    for k, bits in enumerate((0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01)):               # +-inf, NaNs
        flat[:, :, BS + 68, 17 + 97 * k] = bits
        flat[:, :, BS + 69, 1000 - 31 * k] = bits
    flat[:, :, BS + 70] = 0x8000
    flat[:, :, BS + 71] = 0x0003                                                      # a subnormal
    return c


WRITE_SPANS = [(0, 0, 64), (1, 6, 26), (0, 64, 8)]


@pytest.mark.parametrize("kind_fast", [0, 1])
@pytest.mark.parametrize("elem", [FP16, BF16])
def test_write_kv_is_write_runs_into_each_allocation(elem, kind_fast):
    """Caches that hold random rows, every pattern of the element type, zeros, constant runs, inf / NaN, -0 and subnormals: every page
    of both layers in both allocations -- rec_bytes, the FP8 scale, record bytes, decoded bits -- is that of twins written by
    write_runs from the same rows laid contiguous (restated from bf16); pages outside the spans keep what they had; a -1 slot and one
    >= n_slots store the record of a zero row; the caches are unchanged."""
    torch = torch_mod()
    lib = open_lib()
    try:
        set_tuning("slots_kind_fast", kind_fast)
        cont = _bf16_content(50) if elem == BF16 else _fp16_content(51)
        flat16 = _from_cache(cont, elem).reshape(L, 2, (NB + 2) * BS, HALF)
        assert fp16_is_nan(flat16[:, :, BS + 68]).any() and len(np.unique(cont.reshape(L, 2, -1, HALF)[0, 0, BS:BS + 64])) == 65536
        rng = np.random.default_rng(7)
        slots = np.concatenate([np.arange(64), 72 + rng.permutation(N_SLOTS - 72)[:26], np.arange(64, 72)]).astype(np.int64)
        slots[64 + 7] = -1
        slots[64 + 20] = N_SLOTS + 1
        d_slots = torch.from_numpy(slots).cuda()
        st = torch.cuda.Stream()
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        pairs, twins = _pool(lib, conn, [0, 1], 9140, hole=None), _pool(lib, conn, [100, 101], 9140, hole=None)      # the same pages in both
        caches = _typed_caches(torch, cont, elem)
        ks, vs, fs, ns, bs = _kv_span_args(pairs, WRITE_SPANS)
        before = lib.stats().total_compressions
        torch.cuda.synchronize()
        lib.write_slots_kv(ks, vs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream, elem=elem)
        st.synchronize()
        assert lib.stats().total_compressions - before == 2 * L * sum(n // 2 for _, _, n in WRITE_SPANS)
        assert np.array_equal(_host(caches).reshape(cont.shape), cont), "write_slots_kv changed the caches"
        keep = []
        for (a, first, n), b in zip(WRITE_SPANS, bs):
            rows = np.zeros((L, 2, n, HALF), dtype=np.uint16)
            for t in range(n):
                s = int(slots[int(b) + t])
                if 0 <= s < N_SLOTS:
                    rows[:, :, t] = flat16[:, :, BS + s]
            _twin_runs_kv(lib, torch, twins[a], first, rows, st, keep)
        for i, (pair, twin) in enumerate(zip(pairs, twins)):
            _compare_kv(lib, torch, pair, twin, st, (elem, kind_fast, i))
        for kind in (0, 1):
            image = _image_kv(lib, torch, pairs[1][kind], st)
            for layer in range(L):
                assert not _row_kv(image, layer, 6 + 7).any() and not _row_kv(image, layer, 6 + 20).any()      # no row: a zero row
                assert _row_kv(image, layer, 6 + 8).any()
            assert image[STEP - 1].any() and image[0].any() and image[2].any()                                 # outside [6, 32): as filled
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


@pytest.mark.parametrize("elem", [FP16, BF16])
def test_write_kv_with_odd_edges_in_one_call(elem):
    """every odd edge in one call (an odd first completed by a held-in row, an odd end into a held-out row, both, n = 1 either way, a
    span without held rows, an empty one), both wave orders: both allocations equal twins written by write_runs from the same
    positions, the held-out rows are the fp16 of the last positions (restated from bf16) and are not encoded, the rows around them,
    the held-in rows and the caches keep their bits"""
    torch = torch_mod()
    lib = open_lib()
    try:
        st = torch.cuda.Stream()
        cont = _cache_content(60, elem)
        if elem == BF16:
            cont[0, 1, 5, 2, 100:104] = (0x7F80, 0x7FC0, 0xFF80, 0x0001)          # a bf16 row with inf / NaN beside a held fp16 row
        flat16 = _from_cache(cont, elem).reshape(L, 2, (NB + 2) * BS, HALF)
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
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            caches = _typed_caches(torch, cont, elem)
            (ok, ok_host), (ov, ov_host) = _held_block(torch, n_spans), _held_block(torch, n_spans)
            h_out = _held_ptrs((ok, ov), [x[4] for x in HELD_WRITES], n_spans)
            ids = [10 * kind_fast + i for i in range(4)]
            pairs, twins = [conn.add_request(r) for r in ids[:2]], [conn.add_request(r) for r in ids[2:]]
            ks, vs, fs, ns, bs = _kv_span_args(pairs, spans)
            before = lib.stats().total_compressions
            torch.cuda.synchronize()
            lib.write_slots_kv(ks, vs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream,
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
                    _twin_runs_kv(lib, torch, twins[a], first - (1 if hin else 0), np.stack(rows, axis=2), st, keep)
            for i, (pair, twin) in enumerate(zip(pairs, twins)):
                _compare_kv(lib, torch, pair, twin, st, (elem, kind_fast, i))
            got_k, got_v = ok.cpu().numpy().view(np.uint16), ov.cpu().numpy().view(np.uint16)
            assert equal_off_nan(got_k, ok_host, fp16_is_nan(ok_host), fp16_is_nan), (elem, kind_fast, "held-out K rows and their guards")
            assert equal_off_nan(got_v, ov_host, fp16_is_nan(ov_host), fp16_is_nan), (elem, kind_fast, "held-out V rows and their guards")
            assert not got_k[1 + 4].any() and not got_v[1 + 4].any() and got_k[1 + 1].any()    # a padding slot gives zeros
            assert (got_k[0] == 0x7A11).all() and (got_v[-1] == 0x7A11).all()
            image = _image_kv(lib, torch, pairs[0][0], st)
            assert not image[13].any() and image[12].any()                       # position 26 of [20, 27) is held out, not encoded
            assert np.array_equal(_host(caches).reshape(cont.shape), cont), "write_slots_kv changed the caches"
            for r in ids:
                conn.free_request(r)
        assert np.array_equal(ik.cpu().numpy().view(np.uint16), ik_host) and np.array_equal(iv.cpu().numpy().view(np.uint16), iv_host)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_kv_entries_launches_nothing():
    torch = torch_mod()
    lib = open_lib()
    try:
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        (kh, vh), = _pool(lib, conn, [0], 9160)
        kh2, vh2 = conn.add_request(1)
        kh3, vh3 = conn.add_request(2)
        st = torch.cuda.Stream()
        s = st.cuda_stream
        caches = _typed_caches(torch, None, BF16)
        pattern = _host(caches)
        bases, ks = _bases(caches), _kind_stride(caches)
        d_slots = torch.arange(64, dtype=torch.int64, device="cuda")
        everything = (kh, vh, kh2, vh2, kh3, vh3)
        images = [_image_kv(lib, torch, h, st) for h in everything]
        assert images[0][0].any() and not images[2].any() and not images[3].any()
        (ik, _), (iv, _) = _held_block(torch, 2, 1), _held_block(torch, 2, 2)
        (ok, ok_host), (ov, ov_host) = _held_block(torch, 2), _held_block(torch, 2)
        one = lambda blk, i=0: u64(*_held_ptrs(blk, [j == i for j in range(2)], 2)[2 * i:2 * i + 2])
        IN, OUT = one((ik, iv)), one((ok, ov))
        good = dict(k=u64(kh), v=u64(vh), firsts=u64(0), counts=u64(8), begins=u64(0), slots=d_slots.data_ptr(), n_slots=N_SLOTS, bases=bases,
                    layer_begin=0, ks=ks, step=STEP, stream=s, elem=BF16, held_in=None, held_stride=ROW, held_out=None, reserved=0)
        two = dict(firsts=u64(0, 6), counts=u64(8, 4), begins=u64(0, 8))
        inval = [
            dict(k=u64(vh2)),                                                     # an MXFP4 allocation given as K
            dict(v=u64(kh2)),                                                     # an FP8 allocation given as V
            dict(v=u64(kh)), dict(k=u64(vh)),                                     # the same handle in both roles
            dict(stream=0),                                                       # a NULL stream
            dict(bases=u64(bases[0], bases[1] + 8)),                              # a cache pointer not 16-byte aligned
            dict(elem=2), dict(reserved=1),                                       # an unknown elem, reserved != 0
        ]
        read_inval = [dict(counts=u64(9), held_out=OUT)]                          # held_out on a read
        write_inval = [
            dict(firsts=u64(1), counts=u64(7)),                                   # an odd first without held-in
            dict(firsts=u64(1), counts=u64(8), held_out=OUT),
            dict(k=u64(kh, kh), v=u64(vh, vh), **two),                            # two spans sharing a page in both allocations,
            dict(k=u64(kh, kh), v=u64(vh, vh3), **two),                           # in the K allocation alone,
            dict(k=u64(kh, kh3), v=u64(vh, vh), **two),                           # in the V allocation alone
        ]
        general = [dict(k=u64(kh + 12345)), dict(v=u64(vh + 12345)),              # an unknown handle
                   dict(firsts=u64(2 * STEP - 4)),                                # a span leaving its region
                   dict(layer_begin=1), dict(step=KV_PAGES)]                      # pages that leave the allocations

        def call(entry, a):
            entry(a["k"], a["v"], a["firsts"], a["counts"], a["begins"], a["slots"], a["n_slots"], a["bases"], a["layer_begin"], a["ks"],
                  a["step"], a["stream"], elem=a["elem"], held_in=a["held_in"], held_stride=a["held_stride"], held_out=a["held_out"],
                  reserved=a["reserved"])

        def untouched():
            torch.cuda.synchronize()
            assert np.array_equal(_host(caches), pattern), "a refused call wrote to the caches"
            for h, image in zip(everything, images):
                assert np.array_equal(_image_kv(lib, torch, h, st), image), "a refused call wrote to the pool"
            assert np.array_equal(ok.cpu().numpy().view(np.uint16), ok_host) and np.array_equal(ov.cpu().numpy().view(np.uint16), ov_host), \
                "a refused call wrote to the held-out rows"

        for entry, cases in ((lib.read_slots_kv, [(-4, inval + read_inval), (-1, general)]),
                             (lib.write_slots_kv, [(-4, inval + write_inval), (-1, general)])):
            stats = bytes(lib.stats())
            for status, group in cases:
                for case in group:
                    a = dict(good)
                    a.update(case)
                    with pytest.raises(SpeckvError) as e:
                        call(entry, a)
                    assert e.value.status == status, (entry.__name__, case, e.value.status)
            assert bytes(lib.stats()) == stats, (entry.__name__, "a refused call moved the statistics")
            untouched()
        bump = torch.zeros(4, device="cuda")                                # a capturing stream: the descriptors are staged per call
        torch.cuda.synchronize()
        stats = bytes(lib.stats())
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            for entry, case in ((lib.read_slots_kv, dict(counts=u64(9), held_in=IN)), (lib.write_slots_kv, dict(counts=u64(7), held_out=OUT))):
                with pytest.raises(SpeckvError) as e:
                    call(entry, dict(good, **case))
                assert e.value.status == -4
            bump.add_(1)
        g.replay()
        assert bytes(lib.stats()) == stats
        untouched()
        del g
        for entry in (lib.read_slots_kv, lib.write_slots_kv):             # nothing to do: fine
            call(entry, dict(good, k=u64(), v=u64(), firsts=u64(), counts=u64(), begins=u64()))
            call(entry, dict(good, bases=u64()))
            call(entry, dict(good, k=u64(kh, kh2), v=u64(vh, vh2), firsts=u64(0, 64), counts=u64(0, 0), begins=u64(0, 0)))
        untouched()
        call(lib.read_slots_kv, dict(good, counts=u64(9), held_in=IN))    # ... and the good calls do their work
        st.synchronize()
        got = _host(caches)
        for t in range(8):
            assert np.array_equal(got[1, 0, BS + t], _to_cache(_row_kv(images[0], 1, t), BF16))
            assert np.array_equal(got[1, 1, BS + t], _to_cache(_row_kv(images[1], 1, t), BF16))
        assert np.array_equal(got[1, 1, BS + 8], _to_cache(iv.cpu().numpy().view(np.uint16)[1, 1], BF16))
        call(lib.write_slots_kv, dict(good, k=u64(kh2), v=u64(vh2), counts=u64(7), held_out=OUT))
        st.synchronize()
        for h in (kh2, vh2):
            image = _image_kv(lib, torch, h, st)
            assert image[:3].any() and not image[3].any() and image[STEP:STEP + 3].any()
        assert not np.array_equal(ok.cpu().numpy().view(np.uint16)[1], ok_host[1])
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------- the connector
def _tensor_rows(torch, rows):
    """[L][n][1024] fp16 bits -> a [L][n][H][D] fp16 device tensor"""
    return _dev(torch, np.ascontiguousarray(rows).view(np.float16).reshape(L, -1, H, D))


def _same_request(lib, torch, conn, a, b, st, what):
    ra, rb = conn.requests[a], conn.requests[b]
    assert ra.length == rb.length, what
    _compare_kv(lib, torch, (ra.k_handle, ra.v_handle), (rb.k_handle, rb.v_handle), st, what)
    assert (ra.tail_k is None) == (rb.tail_k is None) == (ra.length % 2 == 0), what
    if ra.tail_k is not None:
        assert np.array_equal(_bits(ra.tail_k), _bits(rb.tail_k)) and np.array_equal(_bits(ra.tail_v), _bits(rb.tail_v)), (what, "tails")


@pytest.mark.parametrize("elem", [FP16, BF16])
def test_connector_load_store_walk(elem):
    """A (37 positions by write_prefill) -> caches by load_paged -> B by store_paged in calls of 19 and 18 positions (an odd seam, then
    an odd end): B's records and tail are A's (with bf16 caches: those of a request written from the restated rows), attend and
    attend(window=16) agree to the bit, every load_paged / store_paged is one library call, kv_rows is the rows written, decoded;
    then lengths 0, 6, 7 with counts 5, 0, 3 in one call."""
    torch = torch_mod()
    lib = _CountingKV(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        rng = np.random.default_rng(77)
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        k, v = content(9400, T)[0][:, :37], content(9450, T)[1][:, :37]
        A, B, C = 1, 2, 3
        for rid in (A, B, C):
            conn.add_request(rid)
        keep = conn.write_prefill(A, _dev(torch, k), _dev(torch, v))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        ra = conn.requests[A]
        images = [_image_kv(lib, torch, ra.k_handle, st), _image_kv(lib, torch, ra.v_handle, st)]
        rows_a = np.zeros((L, 2, 37, HALF), dtype=np.uint16)
        for layer in range(L):
            for kind in (0, 1):
                lib.calls.clear()
                got = _bits(conn.kv_rows(A, layer, kind)).reshape(37, HALF)
                assert lib.calls == ["fetch_range"]
                for t in range(36):
                    assert np.array_equal(got[t], _row_kv(images[kind], layer, t)), (layer, kind, t)
                assert np.array_equal(got[36], np.ascontiguousarray((k, v)[kind][layer, 36]).reshape(-1).view(np.uint16))
                assert np.array_equal(_bits(conn.kv_rows(A, layer, kind, 5, 30)).reshape(-1, HALF), got[5:30])
                assert np.array_equal(_bits(conn.kv_rows(A, layer, kind, 36, 37)).reshape(-1, HALF), got[36:])
                rows_a[layer, kind] = got
        assert not np.array_equal(rows_a[:, 0], rows_a[:, 1])
        # ---- A -> caches
        m = rng.permutation(N_SLOTS).astype(np.int64)[:37]
        big = _typed_caches(torch, None, elem)
        caches = [view for _, view in big]
        want = _host(big)
        for t in range(37):
            want[:, :, BS + int(m[t])] = _to_cache(rows_a[:, :, t], elem)
        maps = [_dev(torch, m), _dev(torch, m[:19]), _dev(torch, m[19:])]
        lib.calls.clear()
        conn.load_paged([A], [0], [37], maps[0], caches)
        torch.cuda.synchronize()
        assert lib.calls == ["read_slots_kv"], lib.calls
        assert np.array_equal(_host(big), want), (elem, "load_paged")
        conn.load_paged([A, B], [0, 0], [0, 0], maps[0][:0], caches)
        assert lib.calls == ["read_slots_kv"], "nothing is launched when every count is 0"
        # ---- caches -> B, across an odd seam
        epoch = conn._epoch
        lib.calls.clear()
        keep += conn.store_paged([B], [19], maps[1], caches)
        assert lib.calls == ["write_slots_kv"] and conn.length(B) == 19 and conn.requests[B].tail_k is not None and conn._epoch != epoch
        lib.calls.clear()
        keep += conn.store_paged([B], [18], maps[2], caches)
        torch.cuda.synchronize()
        assert lib.calls == ["write_slots_kv"] and conn.length(B) == 37
        assert np.array_equal(_host(big), want), "store_paged changed the caches"
        ref = A
        if elem == BF16:                                                  # what bf16 caches carry: the rows restated both ways
            restated = bf16_to_fp16_bits(_to_cache(rows_a, BF16))
            keep += conn.write_prefill(C, _tensor_rows(torch, restated[:, 0]), _tensor_rows(torch, restated[:, 1]))
            torch.cuda.synchronize()
            ref = C
        _same_request(lib, torch, conn, B, ref, st, (elem, "B against its reference"))
        for window in (None, 16):
            for layer in range(L):
                q = _dev(torch, rng.standard_normal((1, H, 4, D)).astype(np.float16))
                out_a, out_b = conn.attend(layer, [ref], q, SM, window=window), conn.attend(layer, [B], q, SM, window=window)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(out_a), _bits(out_b)) and bool(torch.isfinite(out_b).all()) and bool(out_b.any()), (elem, window, layer)
        for layer in range(L):
            for kind in (0, 1):
                assert np.array_equal(_bits(conn.kv_rows(B, layer, kind)), _bits(conn.kv_rows(ref, layer, kind))), (elem, layer, kind)
        # ---- the empty span, the even start and the held-in start in one call: lengths 0, 6, 7 and counts 5, 0, 3
        cont = _cache_content(43, elem)
        flat16 = _from_cache(cont, elem).reshape(L, 2, (NB + 2) * BS, HALF)
        src = [view for _, view in _typed_caches(torch, cont, elem)]
        ids, tw = [10, 11, 12], [20, 21, 22]
        for rid in ids + tw:
            conn.add_request(rid)
        six = (_dev(torch, k[:, :6]), _dev(torch, v[:, :6]))
        seven = (_dev(torch, k[:, :7]), _dev(torch, v[:, :7]))
        keep += conn.write_prefill(11, *six) + conn.write_prefill(21, *six) + conn.write_prefill(12, *seven)
        m3 = rng.permutation(N_SLOTS).astype(np.int64)[:8]
        d_m3 = _dev(torch, m3)
        lib.calls.clear()
        keep += conn.store_paged(ids, [5, 0, 3], d_m3, src)
        torch.cuda.synchronize()
        assert lib.calls == ["write_slots_kv"], lib.calls
        assert [conn.length(r) for r in ids] == [5, 6, 10]
        new0 = flat16[:, :, BS + m3[:5]]                                   # [L][2][5][1024]
        new2 = np.concatenate([np.stack([np.ascontiguousarray(x[:, :7]).reshape(L, 7, HALF).view(np.uint16) for x in (k, v)], axis=1),
                               flat16[:, :, BS + m3[5:]]], axis=2)          # [L][2][10][1024]
        keep += conn.write_prefill(20, _tensor_rows(torch, new0[:, 0]), _tensor_rows(torch, new0[:, 1]))
        keep += conn.write_prefill(22, _tensor_rows(torch, new2[:, 0]), _tensor_rows(torch, new2[:, 1]))
        torch.cuda.synchronize()
        for rid, twin in zip(ids, tw):
            _same_request(lib, torch, conn, rid, twin, st, (elem, "batch of three", rid))
        # ---- what is malformed raises before any state changes
        lengths, epoch = [conn.length(r) for r in ids], conn._epoch
        lib.calls.clear()
        for bad in (lambda: conn.store_paged([10, 10], [1, 1], d_m3[:2], src),                        # a request named twice
                    lambda: conn.store_paged([10], [T], _dev(torch, np.zeros(T, dtype=np.int64)), src),   # length + count > max_tokens
                    lambda: conn.store_paged([10], [2], d_m3[:3], src),                               # a mapping of another size
                    lambda: conn.store_paged([10], [2], d_m3[:2].to(torch.int32), src),
                    lambda: conn.store_paged([10], [2], d_m3[:2], [c.to(torch.float32) for c in src]),      # caches of another geometry
                    lambda: conn.load_paged([10], [0], [2], d_m3[:2], src[:1]),
                    lambda: conn.load_paged([10], [4], [2], d_m3[:2], src)):                          # rows the request does not hold
            with pytest.raises(ValueError):
                bad()
        assert lib.calls == [] and [conn.length(r) for r in ids] == lengths and conn._epoch == epoch
    finally:
        lib.finalize()


def test_the_k8v4_paged_example_runs():
    """examples/k8v4_paged_cache_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "k8v4_paged_cache_example.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "k8v4 paged cache example ok" in out.stdout
