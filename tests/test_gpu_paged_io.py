"""-m gpu: paged-cache transfers -- speckv_ext_read_slots / speckv_ext_write_slots (one launch each way between the pool and the slots
of per-layer paged caches), SpeckvKVConnector.load_paged / store_paged and SpeckvVllmConnector(paged_io=True) on top of them.

References: speckv_ext_fetch_range for the bits of a row that is read; for a write, a twin allocation written by
speckv_ext_write_runs from the same rows laid out contiguously (rec_bytes, scale, stored record bytes, decoded bits); for the
connector a twin built by write_prefill, and the row route (kv_rows + index_copy_) of the same tree.

Shapes: L = 2, H = 8, D = 128, T = 128 (64 pages per region), blocks of 16 slots, 12 blocks: the smallest at which odd edges,
several blocks, both layers and both halves of a page can go wrong.  Every cache is a view inside a larger tensor with one guard
block in front and one behind, the declared n_slots ends one block before the view does, and everything is pre-filled with a
pattern: a kernel that mishandles -1 or an out-of-range slot spoils a guard the test compares and touches no foreign memory."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE, ROW = 4096, 2048
L, T = 2, 128
STEP = T // 2
N_PAGES = 2 * L * STEP
BS, NB = 16, 12
N_SLOTS = (NB - 1) * BS                         # declared: one block short of the view
SENTINEL = 0x7C5A
u64 = lambda *v: np.asarray(v, dtype=np.uint64)


def _blocks(n, seed):
    """fp16 page images: random, a few that compress (constant runs, zeros)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ROW)).astype(np.float16)
    x[3] = 0
    x[5] = np.repeat(x[5, :64], 32)
    x[15, 1024:] = x[15, 1024]
    return x


def _fill(lib, h, x, hole=8):
    """every page of the allocation from x, except page `hole` of every (layer, kind) region"""
    for j in range(2 * L):
        for lo, hi in ((j * STEP, j * STEP + hole), (j * STEP + hole + 1, (j + 1) * STEP)):
            part = np.ascontiguousarray(x[lo:hi])
            lib.write(h, lo * PAGE, part.ctypes.data, part.nbytes, False)


def _image(lib, torch, h, stream):
    out = torch.empty((N_PAGES, ROW), dtype=torch.float16, device="cuda")
    lib.fetch_range(h, 0, N_PAGES, out.data_ptr(), False, stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy().view(np.uint16)


def _caches(torch, content=None):
    """per layer (big, view): big = [2][NB + 2][BS][H][D] int16 filled with the pattern (or `content`: [L][2][NB + 2][BS][H * D] host
    uint16), view = big[:, 1:-1] as fp16"""
    out = []
    for layer in range(L):
        if content is None:
            big = torch.full((2, NB + 2, BS, H, D), SENTINEL, dtype=torch.int16, device="cuda")
        else:
            big = torch.from_numpy(content[layer].view(np.int16).reshape(2, NB + 2, BS, H, D).copy()).cuda()
        out.append((big, big.view(torch.float16)[:, 1:-1]))
    return out


def _bases(caches):
    return u64(*[v.data_ptr() for _, v in caches])


def _kind_stride(caches):
    return caches[0][1].stride(0) * 2


def _host(caches):
    """[L][2][(NB + 2) * BS][1024] uint16 of the big tensors"""
    return np.stack([big.cpu().numpy().view(np.uint16).reshape(2, (NB + 2) * BS, H * D) for big, _ in caches])


def _row(image, layer, kind, pos):
    return image[(2 * layer + kind) * STEP + pos // 2].reshape(2, ROW // 2)[pos & 1]


def _slot_list(rng, n, bad=True):
    """n distinct slots of the declared range in random order; bad: two of them replaced by -1 and one by a slot >= N_SLOTS that still
    lies inside the view (its last block)"""
    s = rng.permutation(N_SLOTS)[:n].astype(np.int64)
    if bad:
        s[[3, n - 2]] = -1
        s[n // 2] = N_SLOTS + 3
    return s


SPANS = [(0, 0, 34), (1, 5, 27), (2, 33, 1), (0, 64, 0)]        # (allocation, first, count): [0, 34), [5, 32), [33, 34), [64, 64)


def _span_args(handles, spans):
    begins = np.cumsum([0] + [n for _, _, n in spans])[:-1]
    return u64(*[handles[a] for a, _, _ in spans]), u64(*[f for _, f, _ in spans]), u64(*[n for _, _, n in spans]), u64(*begins)


def _check_read(lib, torch, handles, what, spans=SPANS, seed=5):
    """read_slots of `spans` into patterned caches against an expectation built on the host from fetch_range: whole tensors, guards
    included; then layers [1, 2) alone"""
    st = torch.cuda.Stream()
    images = [_image(lib, torch, h, st) for h in handles]
    total = sum(n for _, _, n in spans)
    slots = _slot_list(np.random.default_rng(seed), total)
    d_slots = torch.from_numpy(slots).cuda()
    hs, fs, ns, bs = _span_args(handles, spans)
    for layer_begin, n_layers in ((0, L), (1, 1)):
        caches = _caches(torch)
        used = caches[layer_begin:layer_begin + n_layers]
        want = _host(caches)
        for (a, first, n), b in zip(spans, bs):
            for t in range(n):
                s = int(slots[int(b) + t])
                if 0 <= s < N_SLOTS:
                    for layer in range(layer_begin, layer_begin + n_layers):
                        for kind in (0, 1):
                            want[layer, kind, BS + s] = _row(images[a], layer, kind, first + t)
        before = lib.stats()
        torch.cuda.synchronize()
        lib.read_slots(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(used), layer_begin, _kind_stride(caches), STEP, st.cuda_stream)
        st.synchronize()
        got = _host(caches)
        assert np.array_equal(got, want), (what, layer_begin, n_layers, np.argwhere((got != want).any(axis=-1))[:8])
        pages = 2 * n_layers * sum((f + n + 1) // 2 - f // 2 for _, f, n in spans if n)
        after = lib.stats()
        assert after.total_decompressions - before.total_decompressions == pages and after.dma_completed - before.dma_completed == pages
    return images


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_read_slots_is_fetch_range_bit_for_bit(scheme, mode):
    """All schemes in both quantiser modes, both wave orders.  Spans [0, 34), [5, 32), [33, 34) and [64, 64) of three allocations, one
    of them named twice; page 8 of every region never written (zeros); the slots a random permutation with two -1 and one >=
    n_slots.  Every row not named keeps the pattern, guards included; layer_begin = 1, n_layers = 1 gives layer 1's bits and leaves
    layer 0's cache alone."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        handles = [lib.alloc(N_PAGES * PAGE) for _ in range(3)]
        for i, h in enumerate(handles):
            _fill(lib, h, _blocks(N_PAGES, 100 + 10 * scheme + i))
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            images = _check_read(lib, torch, handles, (scheme, mode, kind_fast))
        assert not images[0][8].any() and images[0][0].any()
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


WRITE_SPANS = [(0, 0, 34), (1, 6, 26), (0, 40, 2)]


def _random_content(seed):
    """cache contents: random rows, some that compress"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((L, 2, NB + 2, BS, H * D)).astype(np.float16)
    c[:, :, 2, 3] = 0
    c[:, :, 3, 5] = np.repeat(c[:, :, 3, 5, :32], 32, axis=-1)
    c[:, :, 4] = c[:, :, 4, :1, :1]
    return c.view(np.uint16)


def _write_twin(lib, torch, twin_handles, spans, slots, begins, content, stream):
    """the same rows laid out contiguously, written by write_runs: one call per span"""
    keep = []
    flat = content.reshape(L, 2, (NB + 2) * BS, H * D)
    for (a, first, n), b in zip(spans, begins):
        if not n:
            continue
        img = np.zeros((L, 2, n, H * D), dtype=np.uint16)
        for t in range(n):
            s = int(slots[int(b) + t])
            if 0 <= s < N_SLOTS:
                img[:, :, t] = flat[:, :, BS + s]
        d = torch.from_numpy(img.view(np.int16)).cuda()
        keep.append(d)
        firsts = [(2 * layer + kind) * STEP + first // 2 for layer in range(L) for kind in (0, 1)]
        srcs = [d.data_ptr() + (layer * 2 + kind) * n * ROW for layer in range(L) for kind in (0, 1)]
        torch.cuda.synchronize()
        lib.write_runs(twin_handles[a], firsts, srcs, n // 2, stream.cuda_stream)
    stream.synchronize()
    return keep


def _check_write(lib, torch, handles, twins, scheme, what, spans=WRITE_SPANS, seed=9, records=True):
    st = torch.cuda.Stream()
    content = _random_content(seed)
    caches = _caches(torch, content)
    total = sum(n for _, _, n in spans)
    slots = _slot_list(np.random.default_rng(seed + 1), total, bad=False)
    slots[7] = -1
    slots[total - 1] = N_SLOTS + 1
    d_slots = torch.from_numpy(slots).cuda()
    hs, fs, ns, bs = _span_args(handles, spans)
    before = lib.stats().total_compressions
    torch.cuda.synchronize()
    lib.write_slots(hs, fs, ns, bs, d_slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream)
    st.synchronize()
    assert lib.stats().total_compressions - before == 2 * L * sum(n // 2 for _, _, n in spans)
    assert np.array_equal(_host(caches).reshape(content.shape), content), (what, "write_slots changed the caches")
    _write_twin(lib, torch, twins, spans, slots, bs, content, st)
    for h, tw in zip(handles, twins):
        got, want = _image(lib, torch, h, st), _image(lib, torch, tw, st)
        assert np.array_equal(got, want), (what, "decoded bits", np.argwhere((got != want).any(axis=-1))[:8])
        if not records:
            continue
        for p in range(N_PAGES):
            a, b = lib.translate(h, p * PAGE), lib.translate(tw, p * PAGE)
            assert a.rec_bytes == b.rec_bytes, (what, p)
            if scheme != 5:
                assert np.float32(a.scale).view(np.uint32) == np.float32(b.scale).view(np.uint32), (what, p)
            if a.rec_bytes:
                assert np.array_equal(stored_record(a, a.rec_bytes), stored_record(b, b.rec_bytes)), (what, p, "record bytes")
    # the -1 slot: position 7 of the first span is the record of a zero row
    image = _image(lib, torch, handles[spans[0][0]], st)
    for layer in range(L):
        for kind in (0, 1):
            assert not _row(image, layer, kind, spans[0][1] + 7).any(), (what, "a padding slot is a row of zeros")
    return image


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_write_slots_is_write_runs_of_the_rows_laid_contiguous(scheme, mode):
    """All schemes and modes, both wave orders.  Spans [0, 34) and [40, 42) of one allocation and [6, 32) of another; rec_bytes, scale,
    the stored record bytes and fetch_range's bits equal those of twins written by write_runs; a -1 slot and one >= n_slots store the
    record of a zero row; the caches are unchanged."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        for kind_fast in (0, 1):
            set_tuning("slots_kind_fast", kind_fast)
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            twins = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            image = _check_write(lib, torch, handles, twins, scheme, (scheme, mode, kind_fast), seed=9 + scheme)
            assert image[0].any() and not image[STEP - 1].any()
            for h in handles + twins:
                lib.free(h)
    finally:
        set_tuning("slots_kind_fast", 0)
        lib.finalize()


def test_placement_striped_migrated_sealed_and_cached():
    """A pool striped over 3 with pages migrated (FP8 and MXFP4: reads and writes); an INT8_DELTA_RLE allocation sealed by compact --
    read_slots leaves it sealed, write_slots unpacks it; a page cached by speckv_access before the write reads the new bytes after."""
    torch = torch_mod()
    for scheme in (4, 5):
        lib = open_lib(SPECKV_POOL_DEVICES="0,0,0")
        try:
            lib.set_compression_scheme(scheme)
            handles = [lib.alloc(N_PAGES * PAGE) for _ in range(3)]
            for i, h in enumerate(handles):
                _fill(lib, h, _blocks(N_PAGES, 40 + i))
                lib.migrate(h, 1, 4, (i + 1) % 3)                     # pages 1..4 and a page of another region now lie elsewhere
                lib.migrate(h, 2 * STEP + 15, 3, i % 3)
            _check_read(lib, torch, handles, ("striped / migrated", scheme))
            twins = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
            for i, h in enumerate(twins):                             # the same records before, where they were allocated
                _fill(lib, h, _blocks(N_PAGES, 40 + i))
            _check_write(lib, torch, handles[:2], twins, scheme, ("striped / migrated", scheme), records=False)
        finally:
            lib.finalize()
    lib = open_lib()
    try:
        lib.set_compression_scheme(2)
        handles = [lib.alloc(N_PAGES * PAGE) for _ in range(3)]
        for i, h in enumerate(handles):
            _fill(lib, h, _blocks(N_PAGES, 60 + i))
            lib.compact(h)
        sealed = lib.stats().sealed_allocations
        assert sealed == 3
        _check_read(lib, torch, handles, "sealed")
        assert lib.stats().sealed_allocations == sealed, "read_slots leaves a sealed allocation sealed"
        # write into sealed allocations: the twins hold the same records before (unsealed), so afterwards everything is equal
        twins = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
        for i, h in enumerate(twins):
            _fill(lib, h, _blocks(N_PAGES, 60 + i))
        _check_write(lib, torch, handles[:2], twins, 2, "sealed destination", records=False)
        assert lib.stats().sealed_allocations == sealed - 2, "write_slots unpacks a sealed destination"
        # a cached page
        st = torch.cuda.Stream()
        h = handles[2]
        lib.set_compression_scheme(2)
        page = 3 * STEP + 2                                            # layer 1, V, positions 4 and 5
        ptr = lib.access(h, page * PAGE, 64)
        old = dev_to_host(ptr, PAGE).view(np.uint16).copy()
        assert lib.translate(h, page * PAGE).flags & 3
        content = _random_content(77)
        caches = _caches(torch, content)
        slots = torch.tensor([20, 21], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        lib.write_slots(u64(h), u64(4), u64(2), u64(0), slots.data_ptr(), N_SLOTS, _bases(caches), 0, _kind_stride(caches), STEP, st.cuda_stream)
        st.synchronize()
        new = dev_to_host(lib.access(h, page * PAGE, 64), PAGE).view(np.uint16)
        want = _image(lib, torch, h, st)[page]
        assert np.array_equal(new, want) and not np.array_equal(new, old), "a cached page shows the bytes of before the write"
    finally:
        lib.finalize()


def test_every_refusal_launches_nothing():
    """every SPECKV_ERR_INVAL and SPECKV_ERR_GENERAL case of the header, a capturing stream included, for both entries: the caches
    keep the pattern and the pool's records stay; the calls with nothing to do succeed and do nothing; then the good calls work"""
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
        good = dict(handles=u64(h), firsts=u64(0), counts=u64(8), begins=u64(0), slots=d_slots.data_ptr(), n_slots=N_SLOTS, bases=bases,
                    layer_begin=0, ks=ks, step=STEP, stream=s)
        inval = [
            dict(stream=0),                                            # NULL stream
            dict(slots=0),                                             # NULL slot mapping
            dict(bases=u64(bases[0], 0)),                              # a NULL cache pointer
            dict(bases=u64(bases[0], bases[1] + 8)),                   # ... one not 16-byte aligned
            dict(ks=ks + 8),                                           # a plane stride that is no multiple of 16
            dict(step=0),
            dict(handles=u64(h, other), firsts=u64(0, 0), counts=u64(8, 8), begins=u64(0, 8)),      # allocations of different schemes
        ]
        write_inval = [
            dict(firsts=u64(1)),                                       # odd first / count on the write side
            dict(counts=u64(7)),
            dict(handles=u64(h, h), firsts=u64(0, 6), counts=u64(8, 4), begins=u64(0, 8)),          # two spans share a page
        ]
        general = [
            dict(handles=u64(h + 12345)),                              # an unknown handle
            dict(firsts=u64(2 * STEP - 4)),                            # the span leaves its (layer, kind) region
            dict(step=N_PAGES),                                        # ... the allocation
            dict(layer_begin=1),                                       # layers [1, 3) of an allocation of two
        ]

        def call(entry, a):
            entry(a["handles"], a["firsts"], a["counts"], a["begins"], a["slots"], a["n_slots"], a["bases"], a["layer_begin"], a["ks"],
                  a["step"], a["stream"])

        def untouched():
            torch.cuda.synchronize()
            assert np.array_equal(_host(caches), pattern), "a refused call wrote to the caches"
            assert np.array_equal(_image(lib, torch, h, st), image) and not _image(lib, torch, h2, st).any(), "a refused call wrote to the pool"

        for entry, cases in ((lib.read_slots, [(-4, inval), (-1, general)]), (lib.write_slots, [(-4, inval + write_inval), (-1, general)])):
            for status, group in cases:
                for case in group:
                    a = dict(good)
                    a.update(case)
                    with pytest.raises(SpeckvError) as e:
                        call(entry, a)
                    assert e.value.status == status, (entry.__name__, case, e.value.status)
            untouched()
        for name in ("speckv_ext_read_slots", "speckv_ext_write_slots"):
            for k in range(4):                                         # NULL arrays
                arrs = [u64(h), u64(0), u64(8), u64(0)]
                ptrs = [x.ctypes.data for x in arrs]
                ptrs[k] = None
                with pytest.raises(SpeckvError) as e:
                    lib._ext(name, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 1, d_slots.data_ptr(), N_SLOTS, bases.ctypes.data, 0, L, ks, STEP, s)
                assert e.value.status == -4, (name, k)
            with pytest.raises(SpeckvError) as e:
                lib._ext(name, u64(h).ctypes.data, u64(0).ctypes.data, u64(8).ctypes.data, u64(0).ctypes.data, 1, d_slots.data_ptr(), N_SLOTS, None,
                         0, L, ks, STEP, s)
            assert e.value.status == -4, name
        untouched()
        # a capturing stream: the descriptors are staged per call
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            for entry in (lib.read_slots, lib.write_slots):
                with pytest.raises(SpeckvError) as e:
                    call(entry, good)
                assert e.value.status == -4
            bump.add_(1)
        g.replay()
        untouched()
        del g
        for entry in (lib.read_slots, lib.write_slots):               # nothing to do: fine
            call(entry, dict(good, handles=u64(), firsts=u64(), counts=u64(), begins=u64()))
            call(entry, dict(good, bases=u64()))
            call(entry, dict(good, handles=u64(h, h2), firsts=u64(0, 64), counts=u64(0, 0), begins=u64(0, 0)))
        untouched()
        call(lib.read_slots, good)                                     # ... and the good calls do their work
        st.synchronize()
        got = _host(caches)
        for layer in range(L):
            for kind in (0, 1):
                for t in range(8):
                    assert np.array_equal(got[layer, kind, BS + t], _row(image, layer, kind, t))
        filled = _caches(torch, _random_content(1))
        torch.cuda.synchronize()
        call(lib.write_slots, dict(good, handles=u64(h2), bases=_bases(filled)))
        st.synchronize()
        assert _image(lib, torch, h2, st)[:4].any()
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", [2, 4])
def test_ordering_on_one_stream_and_across_streams(scheme):
    """write_slots then read_slots on one busy, non-current stream with no synchronisation between them returns what was written; a
    read_slots on stream B behind a write_slots on stream A sees the write"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        content = _random_content(31)
        flat = content.reshape(L, 2, (NB + 2) * BS, H * D)
        n = 64
        slots = np.random.default_rng(3).permutation(N_SLOTS)[:n].astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        out_slots = torch.from_numpy(np.arange(n, dtype=np.int64)).cuda()
        busy = torch.randn((2048, 2048), device="cuda")
        for two_streams in (False, True):
            h = lib.alloc(N_PAGES * PAGE)
            src, dst = _caches(torch, content), _caches(torch)
            a, b = torch.cuda.Stream(), torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(a):
                for _ in range(20):
                    busy = busy @ busy * 1e-3                          # the stream has work queued in front of the write
            lib.write_slots(u64(h), u64(0), u64(n), u64(0), d_slots.data_ptr(), N_SLOTS, _bases(src), 0, _kind_stride(src), STEP, a.cuda_stream)
            rs = b if two_streams else a
            lib.read_slots(u64(h), u64(0), u64(n), u64(0), out_slots.data_ptr(), N_SLOTS, _bases(dst), 0, _kind_stride(dst), STEP, rs.cuda_stream)
            torch.cuda.synchronize()
            image = _image(lib, torch, h, a)
            got = _host(dst)
            assert image[0].any()
            for layer in range(L):
                for kind in (0, 1):
                    for t in range(n):
                        assert np.array_equal(got[layer, kind, BS + t], _row(image, layer, kind, t)), (two_streams, layer, kind, t)
    finally:
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------- the connector
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


class _Counting:
    """wraps a SpeckvLib and counts the data calls a connector makes"""
    NAMES = ("read_slots", "write_slots", "fetch_range", "write_runs")

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name in self.NAMES:
            def counted(*a, **k):
                self.calls.append(name)
                return f(*a, **k)
            return counted
        return f


def _all_rows(conn, rid):
    return [_bits(conn.kv_rows(rid, layer, kind)) for layer in range(L) for kind in (0, 1)]


@pytest.mark.parametrize("prescale", [False, True])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_connector_store_and_load(scheme, prescale):
    """store_paged of prompts of 33, 64 and 2 positions against a twin built by write_prefill from the same rows: six append + attend
    steps give out and lse equal to the bit; load_paged into fresh blocks equals the kv_rows + index_copy_ route to the bit for a range
    with odd ends and for one that includes a tail; with a K pre-scale both calls give the row route's bits (they ARE the row route
    then); the library calls are counted: three requests x two layers loaded = one read_slots and no fetch_range, two requests stored =
    one write_slots and no write_runs."""
    torch = torch_mod()
    lib = _Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        rng = np.random.default_rng(41)
        lengths = {1: 33, 2: 64, 3: 2}
        paged, twin = SpeckvKVConnector(lib, L, H, D, T, scheme), SpeckvKVConnector(lib, L, H, D, T, scheme)
        if prescale:
            kscale = np.ones((L, H, D), np.float32)
            kscale[:, :, 0::8] = 4.0; kscale[:, :, 3::8] = 0.25
            for c in (paged, twin):
                c.set_k_channel_scale(_dev(torch, kscale))
        content = _random_content(43)
        caches = [v for _, v in _caches(torch, content)]
        perm = rng.permutation(N_SLOTS).astype(np.int64)
        mapping, at = {}, 0
        for rid, n in lengths.items():
            mapping[rid] = perm[at:at + n]
            at += n
        keep = []
        ids = list(lengths)
        for rid in ids:
            paged.add_request(rid)
            twin.add_request(100 + rid)
            sl = _dev(torch, mapping[rid])
            k = torch.stack([c[0].reshape(-1, H, D).index_select(0, sl) for c in caches])
            v = torch.stack([c[1].reshape(-1, H, D).index_select(0, sl) for c in caches])
            keep += twin.write_prefill(100 + rid, k, v)
        torch.cuda.synchronize()
        lib.calls.clear()
        d_map = _dev(torch, np.concatenate([mapping[r] for r in ids[:2]]))
        keep += paged.store_paged(ids[:2], [lengths[r] for r in ids[:2]], d_map, caches)
        if not prescale:
            assert lib.calls == ["write_slots"], lib.calls
        else:
            assert lib.calls == ["write_runs", "write_runs"], lib.calls
        keep += paged.store_paged([3], [2], _dev(torch, mapping[3]), caches)
        torch.cuda.synchronize()
        for rid in ids:
            assert paged.length(rid) == twin.length(100 + rid) == lengths[rid]
            a, b = _all_rows(paged, rid), _all_rows(twin, 100 + rid)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (scheme, rid, "stored rows")
        with pytest.raises(ValueError):
            paged.store_paged([1], [2], _dev(torch, mapping[3]), caches)              # an odd length: not built
        # ---- load into fresh blocks: against the row route
        loads = [(1, 3, 30), (2, 1, 62), (3, 0, 2)]                   # an odd start up to the tail (position 32); odd ends; a whole request
        lmap = rng.permutation(N_SLOTS).astype(np.int64)[:sum(n for _, _, n in loads)]
        d_lmap = _dev(torch, lmap)
        fresh = _caches(torch)
        ref = _caches(torch)
        torch.cuda.synchronize()
        lib.calls.clear()
        paged.load_paged([r for r, _, _ in loads], [f for _, f, _ in loads], [n for _, _, n in loads], d_lmap, [v for _, v in fresh])
        torch.cuda.synchronize()
        if not prescale:
            assert lib.calls == ["read_slots"], lib.calls
        at = 0
        for rid, f, n in loads:
            sl = d_lmap[at:at + n]
            at += n
            for layer, (_, view) in enumerate(ref):
                for kind in (0, 1):
                    view[kind].reshape(-1, H, D).index_copy_(0, sl, paged.kv_rows(rid, layer, kind, f, f + n))
        torch.cuda.synchronize()
        assert np.array_equal(_host(fresh), _host(ref)), (scheme, prescale, "load_paged is not the row route")
        # ---- six decode steps on both sides
        G, sm = 4, 1.0 / np.sqrt(D)
        tids = [100 + r for r in ids]
        for step in range(6):
            k_new, v_new = _dev(torch, rng.standard_normal((3, L, H, D)).astype(np.float16)), _dev(torch, rng.standard_normal((3, L, H, D)).astype(np.float16))
            keep.append(paged.append(ids, k_new, v_new))
            keep.append(twin.append(tids, k_new, v_new))
            for layer in range(L):
                q = _dev(torch, rng.standard_normal((1, 3, H, G, D)).astype(np.float16))
                out_a, lse_a, _ = paged._attend_layers_lse(layer, 1, ids, q, sm, None, None)
                out_b, lse_b, _ = twin._attend_layers_lse(layer, 1, tids, q, sm, None, None)
                torch.cuda.synchronize()
                assert np.array_equal(_bits(out_a), _bits(out_b)) and np.array_equal(_bits(lse_a), _bits(lse_b)), (scheme, prescale, step, layer)
                assert bool(torch.isfinite(out_a).all())
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------------- the adapter
def test_adapter_paged_io_equals_the_row_route():
    """The scheduler / worker stand-ins of test_vllm_shaped_connector_round_trip drive two SpeckvVllmConnectors, paged_io=True and False,
    each with caches of its own: store, free the blocks, a prefix hit into different blocks, a preempted request resumed with a new block
    table, and a store whose kv_layer is not the registered tensor (the stash route).  After every step the two sets of caches and
    the two pools' kv_rows are equal to the bit; the paged side issues one read_slots / write_slots per step and no fetch_range /
    write_runs."""
    torch = torch_mod()
    from types import SimpleNamespace as NS
    from cxl_speckv_amd.vllm_connector import SpeckvVllmConnector, slot_mapping_for
    lib = _Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        names = [f"model.layers.{i}.self_attn.attn" for i in range(L)]
        sides = {}
        for paged in (True, False):
            c = SpeckvVllmConnector(lib, num_layers=L, num_kv_heads=H, head_dim=D, block_size=BS, max_tokens=T, scheme="fp8", paged_io=paged)
            big = _caches(torch)
            for b, _ in big:
                b.zero_()
            caches = {n: v for n, (_, v) in zip(names, big)}
            c.register_kv_caches(caches)
            if not paged:
                c._next_id = 1001                                       # the two pools live in one engine: ids of their own
            sides[paged] = (c, caches, big)
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        prompts = {"req-a": (40, [3, 9, 4]), "req-b": (64, [10, 1, 7, 0]), "req-c": (33, [2, 5, 8])}

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

        rows = {(rid, li): torch.randn((2, n, H, D), generator=gen, device="cuda").to(torch.float16) for rid, (n, _) in prompts.items() for li in range(L)}

        def store(rids, foreign=False):
            def run(paged, c, caches):
                new = [NS(req_id=rid, prompt_token_ids=list(range(prompts[rid][0])), block_ids=[prompts[rid][1]]) for rid in rids]
                meta = c.build_connector_meta(NS(scheduled_new_reqs=new))
                assert [m.is_store for m in meta.requests] == [True] * len(rids)
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
                    assert lib.calls == ["write_slots"], lib.calls
                if paged and foreign:
                    assert "write_slots" not in lib.calls and lib.calls.count("write_runs") == len(rids), lib.calls
            each(run)

        def load(rids, blocks, computed, resumed, what):
            def run(paged, c, caches):
                for t in caches.values():
                    t.zero_()                                           # the blocks were freed and handed to somebody else
                reqs = []
                for rid in rids:
                    n = prompts[rid][0]
                    req = NS(request_id=rid, num_tokens=n)
                    matched, is_async = c.get_num_new_matched_tokens(req, computed)
                    assert matched == (n - 1) // BS * BS - computed and is_async is False
                    c.update_state_after_alloc(req, NS(get_block_ids=lambda b=blocks[rid]: [b]), matched)
                    reqs.append(n)
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
                    assert lib.calls == ["read_slots"], (what, lib.calls)
                for li, name in enumerate(names):
                    assert bool(caches[name].reshape(2, NB * BS, H, D)[:, torch.tensor(slot_mapping_for(blocks[rids[0]], BS, 16, computed), device="cuda")].any())
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
    finally:
        lib.finalize()


def test_the_example_runs():
    """examples/paged_cache_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "paged_cache_example.py")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "paged cache example ok" in out.stdout
