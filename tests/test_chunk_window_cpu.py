"""Not -m gpu: the windowed chunk attention (speckv_ext_attend_chunk_window, speckv_ext_chunk_window_walk,
SpeckvKVConnector.attend_chunk(window=...) / chunk_window_walk / chunk_pieces(window=...)).

The declarations, the entry on the device-less engine, the walk rule of the library against the connector's restatement and against a
brute-force restatement written here (the tiles that hold a position a live row of the block sees), the pieces of the split form under
a window, the connector's refusals against a library that must not be called and what it calls with and without a window, and a
float64 emulation of the kernel's walk, masks and staging that shows what each mutation of them would compute."""
import ctypes as C
import fnmatch
import itertools
import math
import os
import re
import sys
import types

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests.test_chunk_cpu import _Shape, _SilentLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_END = [0, 2, 30, 32, 34, 64, 98, 200, 480]
N_Q = [1, 2, 16, 17, 33, 70, 200]
RPPS = [1, 4, 16]
WINDOWS = [1, 2, 3, 31, 32, 33, 40, 64, 65, 100, 300, 10 ** 6]
LONG = [(32768, 0, 1), (32768, 1, 1), (32768, 0, 70), (32768, 1, 70), (32768, 0, 512)]      # (pos_end, base, n_q) with W 1024 / 4096
LONG_WINDOWS = [1024, 4096]


def test_the_window_entry_and_the_walk_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_attend_chunk_window\s*\(", header)
    assert re.search(r"speckv_status_t\s+speckv_ext_chunk_window_walk\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # additive entries: the version stays
    doc = header[header.index("speckv_ext_attend_chunk_window:"):]
    assert "window == 0" in doc and "NOT capturable" in doc and "nothing is freed" in doc
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    for name in ("speckv_ext_attend_chunk_window", "speckv_ext_chunk_window_walk"):
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), patterns
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_window"]
    split = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_split"]
    # the split entry's signature with the mask pair (d_mask, mask_words) replaced by one c_uint32
    assert len(sig) == len(split) - 1 == 22
    assert sig[:16] == split[:16] and sig[16] is C.c_uint32 and sig[17:] == split[18:]
    assert split[16] is C.c_void_p and split[17] is C.c_uint32
    walk = speckv_ctypes._EXT_SIGNATURES["speckv_ext_chunk_window_walk"]
    assert len(walk) == 8 and [walk[k] for k in (0, 4, 5)] == [C.c_uint32] * 3 and all(walk[k] is C.c_void_p for k in (1, 2, 3, 6, 7))
    assert callable(speckv_ctypes.SpeckvLib.attend_chunk_window) and callable(speckv_ctypes.SpeckvLib.chunk_window_walk)
    assert callable(SpeckvKVConnector.chunk_window_walk)


def test_the_library_exports_both_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_chunk_window") and hasattr(lib, "speckv_ext_chunk_window_walk")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_window_entry_on_the_null_engine_answers_as_the_split_entry_does():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call; nothing is counted"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        before = bytes(lib.stats())
        with pytest.raises(SpeckvError) as split:
            lib.attend_chunk_split(u64(a), 0, at, 1, 1, np.asarray([0], np.uint32), np.asarray([1], np.uint32), at, at, 1024, 1024, None, 0,
                                   0, 0, 0, 1, 5, 1.0, at, 0, 1)
        for window, n_splits in ((0, 1), (1, 1), (7, 0), (7, 5), (10 ** 6, 64)):
            with pytest.raises(SpeckvError) as chunk:
                lib.attend_chunk_window(u64(a), 0, at, 1, 1, np.asarray([0], np.uint32), np.asarray([1], np.uint32), at, at, 1024, 1024, None,
                                        0, 0, 0, window, n_splits, 1.0, at, 0, 1)
            assert chunk.value.status == split.value.status == -2              # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- the walk rule
def _ceil(a, b):
    return -(-a // b)


def _brute_walk(pos_end, base, n_q, rpp, window):
    """per query block the sorted tiles that hold a position visible to a live row of the block, from the semantics alone: row j at the
    absolute position P = pos_end + base + j sees the absolute positions max(0, P + 1 - W) .. P; a stored position t lies in tile
    t >> 5, a held position t (the absolute position pos_end + t) in tile n_pool + (t >> 5)"""
    per, n_pool = 64 // rpp, _ceil(pos_end, 32)
    total = pos_end + base + n_q
    tile_of = np.concatenate([np.arange(pos_end) >> 5, n_pool + (np.arange(base + n_q) >> 5)]).astype(np.int64)
    blocks = []
    for j_first in range(0, n_q, per):
        seen = np.zeros(total, bool)
        for j in range(j_first, min(j_first + per, n_q)):
            P = pos_end + base + j
            seen[max(0, P + 1 - window):P + 1] = True
        blocks.append(np.unique(tile_of[seen]).tolist())
    return blocks


@pytest.fixture(scope="module")
def clib():
    lib = C.CDLL(pkg.build_library())
    lib.speckv_ext_chunk_window_walk.restype = C.c_int
    lib.speckv_ext_chunk_window_walk.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.speckv_ext_chunk_split_plan.restype = C.c_int
    lib.speckv_ext_chunk_split_plan.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def _lib_walk(clib, seqs, rpp, window, with_base=True):
    n, per = len(seqs), 64 // rpp
    pe, bs, nq = ((C.c_uint32 * n)(*[s[k] for s in seqs]) for k in range(3))
    total = sum(_ceil(s[2], per) for s in seqs)
    first, count = (C.c_uint32 * (total + 1))(), (C.c_uint32 * (total + 1))()
    first[total] = count[total] = 0xABCD
    assert clib.speckv_ext_chunk_window_walk(n, pe, bs if with_base else None, nq, rpp, window, first, count) == 0
    assert first[total] == count[total] == 0xABCD                       # nothing beyond the blocks is written
    out, at = [], 0
    for s in seqs:
        k = _ceil(s[2], per)
        out.append(list(zip(first[at:at + k], count[at:at + k])))
        at += k
    return out


def _check_walks(clib, seqs, rpp, window):
    """the library, the connector and the brute force agree on every (sequence, block); returns the number of blocks"""
    per = 64 // rpp
    got = _lib_walk(clib, seqs, rpp, window)
    py = SpeckvKVConnector.chunk_window_walk([s[2] for s in seqs], [s[0] + s[1] for s in seqs], rpp, window)
    assert got == py, (rpp, window)
    bound, n = _ceil(window + per - 1, 32) + 2, 0
    for (pos_end, base, n_q), walk in zip(seqs, got):
        brute = _brute_walk(pos_end, base, n_q, rpp, window)
        assert len(walk) == len(brute)
        for blk, ((t_first, count), tiles) in enumerate(zip(walk, brute)):
            what = (pos_end, base, n_q, rpp, window, blk)
            assert tiles == list(range(t_first, t_first + count)), what   # exactly the tiles seen, and they are one range
            assert count <= bound, what
            j_last = min((blk + 1) * per, n_q) - 1
            assert t_first + count == _ceil(pos_end, 32) + ((base + j_last) >> 5) + 1, what
        n += len(walk)
    return n


@pytest.mark.parametrize("rpp", RPPS)
def test_the_walk_against_the_connector_and_a_brute_force_restatement(clib, rpp):
    """every block of the grid is exact -- the range [t_first, t_first + count) IS the set of tiles that hold a position visible to a
    live row of the block -- and never longer than ceil((W + per_blk - 1) / 32) + 2 tiles; works without speckv_init"""
    seqs = [(p, b, n) for p in POS_END for b in (0, 1) for n in N_Q]
    blocks = sum(_check_walks(clib, seqs, rpp, w) for w in WINDOWS)
    assert blocks == len(WINDOWS) * len(POS_END) * 2 * sum(_ceil(n, 64 // rpp) for n in N_Q)
    for w in LONG_WINDOWS:
        _check_walks(clib, LONG, rpp, w)
    # a 1024-position window over 32k stored positions walks 1/32 of the pool tiles and change, not 1024 of them
    (t_first, count), = _lib_walk(clib, [(32768, 0, 1)], rpp, 1024)[0]
    assert (t_first, count) == (992, 33)


def test_the_walk_without_a_window_is_the_whole_walk_and_bad_input_is_refused(clib):
    seqs = [(p, b, n) for p in POS_END for b in (0, 1) for n in N_Q]
    for rpp in (1, 2, 4, 8, 16):
        per = 64 // rpp
        for walk, (pos_end, base, n_q) in zip(_lib_walk(clib, seqs, rpp, 0), seqs):
            assert walk == [(0, _ceil(pos_end, 32) + ((base + min((blk + 1) * per, n_q) - 1) >> 5) + 1) for blk in range(_ceil(n_q, per))]
        assert SpeckvKVConnector.chunk_window_walk([s[2] for s in seqs], [s[0] + s[1] for s in seqs], rpp, None) == _lib_walk(clib, seqs, rpp, 0)
    assert _lib_walk(clib, [(64, 0, 5)], 4, 40, with_base=False) == _lib_walk(clib, [(64, 0, 5)], 4, 40)     # base NULL: no tails
    out, one, two = (C.c_uint32 * 4)(7, 7, 7, 7), (C.c_uint32 * 1)(64), (C.c_uint32 * 1)(1)
    for rpp in (0, 3, 32):
        assert clib.speckv_ext_chunk_window_walk(1, one, None, one, rpp, 5, out, out) == -4                  # SPECKV_ERR_INVAL
    assert clib.speckv_ext_chunk_window_walk(1, two, None, one, 4, 5, out, out) == -4                        # an odd pos_end
    assert clib.speckv_ext_chunk_window_walk(1, one, one, one, 4, 5, out, out) == -4                         # base 64
    assert clib.speckv_ext_chunk_window_walk(1, None, None, one, 4, 5, out, out) == -4
    assert clib.speckv_ext_chunk_window_walk(1, one, None, one, 4, 5, None, out) == -4
    assert list(out) == [7] * 4
    for bad in (-1, True, 2.5, "3", 1 << 32):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_window_walk([1], [64], 4, bad)


# ----------------------------------------------------------------------------- the pieces under a window
def _piece_ranges(pos_end, base, n_q, rpp, window, pieces, tpp, first):
    """per query block the tile range [a, b) of every piece as k_attend_chunk computes it: piece p starts at pool tile first + p tpp,
    ends before first + (p + 1) tpp or n_pool -- the last piece behind the block's last held tile -- and is clipped from below by
    the block's first tile"""
    n_pool = _ceil(pos_end, 32)
    walk = SpeckvKVConnector.chunk_window_walk([n_q], [pos_end + base], rpp, window)[0]
    out = []
    for t_first, count in walk:
        ranges = []
        for p in range(pieces):
            piece_first = first + p * tpp
            t_begin = max(piece_first, t_first)
            t_end = t_first + count if p + 1 == pieces else min(piece_first + tpp, n_pool)
            ranges.append((t_begin, t_end))
        out.append(((t_first, t_first + count), ranges))
    return out


@pytest.mark.parametrize("n_splits", [2, 3, 5, 64, 0])
def test_the_pieces_under_a_window_partition_the_walk(clib, n_splits):
    """for forced 2, 3, 5 and 64 pieces and for the library's rule: the pieces' ranges, clipped by the block's first tile, are disjoint
    and ascending and cover exactly the block's walk; empty pieces occur, never as the last piece.  The plan is the UNCHANGED
    speckv_ext_chunk_split_plan over the pool tiles left from the sequence's first tile on"""
    seqs = [(p, b, n, w) for p in POS_END for b in (0, 1) for n in N_Q for w in WINDOWS] + [s + (w,) for s in LONG for w in LONG_WINDOWS]
    empty = late = 0
    for rpp in RPPS:
        for pos_end, base, n_q, w in seqs:
            what = (pos_end, base, n_q, rpp, w, n_splits)
            pieces, tpps, firsts, first_tiles = SpeckvKVConnector.chunk_pieces([n_q], [pos_end + base], rpp, n_splits, 256, window=w)
            n_pool = _ceil(pos_end, 32)
            lo0 = max(0, pos_end + base + 1 - w)
            assert first_tiles == [lo0 >> 5 if lo0 < pos_end else n_pool], what
            rest = (C.c_uint32 * 1)(32 * (n_pool - first_tiles[0]))
            p_lib, t_lib = (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
            assert clib.speckv_ext_chunk_split_plan(1, rest, (C.c_uint32 * 1)(n_q), rpp, n_splits, 256, p_lib, t_lib) == 0
            assert (pieces, tpps, firsts) == ([p_lib[0]], [t_lib[0]], [0]), what
            late += first_tiles[0] > 0
            for (t_first, n_tiles), ranges in _piece_ranges(pos_end, base, n_q, rpp, w, pieces[0], tpps[0], first_tiles[0]):
                covered = []
                for a, b in ranges:
                    empty += a >= b
                    covered += list(range(a, b))
                assert covered == list(range(t_first, n_tiles)), (what, ranges)          # ascending, disjoint, exactly the walk
                assert ranges[-1][0] < ranges[-1][1], what                                # the last piece holds the row itself
    assert late > 0
    if n_splits != 0:
        assert empty > 0                                                 # later blocks have empty pieces


def test_chunk_pieces_without_a_window_is_unchanged():
    for window in (None, 0):
        for splits in (0, 1, 3, 64):
            assert SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, splits, 256, window=window) == \
                SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, splits, 256)
    assert len(SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, 0)) == 3
    # a window that cuts nothing: today's plan, and first tiles of 0
    assert SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, 5, 256, window=10 ** 6)[:3] == SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, 5)
    assert SpeckvKVConnector.chunk_pieces([70, 1], [4000, 32769], 8, 5, 256, window=10 ** 6)[3] == [0, 0]
    # 32k stored positions under a 1024-position window: the 33 tiles that are left, not 1024, are cut
    pieces, tpp, _, first = SpeckvKVConnector.chunk_pieces([1], [32768], 8, 64, 256, window=1024)
    assert (pieces, tpp, first) == ([32], [1], [992])
    for bad in (-1, True, 2.5, "3"):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_pieces([1], [64], 4, 0, 256, window=bad)


# ----------------------------------------------------------------------------- the connector
@pytest.mark.parametrize("bad", [-1, True, False, 2.5, "8", [8]])
def test_attend_chunk_refuses_a_bad_window_before_any_library_call(bad):
    L, H, D, T, S, R = 2, 8, 128, 64, 5, 4
    conn = SpeckvKVConnector(_SilentLib(), L, H, D, T, "fp8")
    conn.add_request(1)
    q, kv = _Shape(1, S, H, R, D), _Shape(1, S, L, H, D)
    with pytest.raises(ValueError, match="window"):
        conn.attend_chunk(0, [1], q, kv, kv, 1.0, window=bad)
    with pytest.raises(ValueError, match="window"):
        conn.attend_chunk(0, [1], q, kv, kv, 1.0, splits=0, window=bad)


@pytest.mark.parametrize("splits", [0, 1, 5])
def test_attend_chunk_refuses_a_window_with_parents_before_any_library_call(splits):
    L, H, D, T, S, R = 2, 8, 128, 64, 5, 4
    conn = SpeckvKVConnector(_SilentLib(), L, H, D, T, "fp8")
    conn.add_request(1)
    q, kv = _Shape(1, S, H, R, D), _Shape(1, S, L, H, D)
    for window in (1, 8, 10 ** 6):
        with pytest.raises(ValueError, match="window"):
            conn.attend_chunk(0, [1], q, kv, kv, 1.0, parents=[-1, 0, 0, 1, 1], splits=splits, window=window)
    # the other refusals hold under a window
    with pytest.raises(ValueError):
        conn.attend_chunk(0, [1], _Shape(1, S, H, 3, D), kv, kv, 1.0, window=8)
    with pytest.raises(ValueError, match="splits"):
        conn.attend_chunk(0, [1], q, kv, kv, 1.0, splits=65, window=8)


class _Tensor:
    """what attend_chunk asks of a contiguous tensor, without a device"""

    def __init__(self, shape, ptr):
        self.shape, self.ptr = tuple(shape), ptr
        self.strides = tuple(int(np.prod(shape[k + 1:])) for k in range(len(shape)))

    def contiguous(self): return self
    def stride(self, k=None): return self.strides if k is None else self.strides[k]
    def data_ptr(self): return self.ptr


def _stub_torch():
    """a stand-in for the torch module as attend_chunk uses it on its way to the library: streams, and the output tensor"""
    stream = types.SimpleNamespace(cuda_stream=0x5000, wait_stream=lambda other: None)

    class _Ctx:
        def __init__(self, *a): pass
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    cuda = types.SimpleNamespace(current_stream=lambda: stream, Stream=lambda: stream, stream=_Ctx)
    make = lambda shape, dtype=None, device=None: _Tensor(shape, 0x9000)
    return types.SimpleNamespace(cuda=cuda, empty=make, zeros=make, float32="float32")


class _Recorder(_SilentLib):
    """a library that notes the attention entry a call reaches and its arguments"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def _note(self, name):
        def call(*args):
            self.calls.append((name,) + tuple(a.tolist() if isinstance(a, np.ndarray) else list(a) if isinstance(a, C.Array) else a for a in args))
        return call

    def __getattr__(self, name):
        if name in ("attend_chunk", "attend_chunk_split", "attend_chunk_masked", "attend_chunk_window"):
            return self._note(name)
        return super().__getattr__(name)


def test_without_a_window_attend_chunk_calls_what_it_calls_today_and_with_one_the_new_entry(monkeypatch):
    """window=None / 0 reaches the entry the call reaches without the argument, with the same arguments; window=W reaches
    speckv_ext_attend_chunk_window with the split entry's arguments, the mask pair replaced by W and `splits` passed through"""
    monkeypatch.setitem(sys.modules, "torch", _stub_torch())
    L, H, D, T, S, R = 2, 8, 128, 64, 5, 4
    lib = _Recorder()
    conn = SpeckvKVConnector(lib, L, H, D, T, "fp8")
    for rid in (1, 2):
        conn.add_request(rid)
    conn.requests[2].length = 12
    q, k, v = _Tensor((2, S, H, R, D), 0x1000), _Tensor((2, S, L, H, D), 0x2000), _Tensor((2, S, L, H, D), 0x3000)
    run = lambda **kw: conn.attend_chunk(1, [1, 2], q, k, v, 0.5, [S, 3], **kw)
    for splits in (1, 0, 7):
        del lib.calls[:]
        run(splits=splits)
        run(splits=splits, window=None)
        run(splits=splits, window=0)
        today, none, zero = lib.calls
        assert today[0] == ("attend_chunk" if splits == 1 else "attend_chunk_split")
        assert none == today and zero == today
        del lib.calls[:]
        run(splits=0 if splits == 1 else splits)
        run(splits=splits, window=9)
        split, win = lib.calls
        assert split[0] == "attend_chunk_split" and win[0] == "attend_chunk_window"
        # (name, handles, layer, q, C, R, pos_end, n_q, k, v, strides x 2, tail_idx, kt, vt, tail stride | mask, words, splits | rest)
        assert win[1:16] == split[1:16] and win[16:18] == (9, splits) and win[18:] == split[19:] and split[16:18] == (0, 0)
        assert win[6] == [0, 12] and win[7] == [S, 3]


# ----------------------------------------------------------------------------- what the kernel computes, restated in float64
def _emulate(pos_end, base, n_q, rpp, window, q, K, V, pieces=1, tpp=0, first_tile=0, mutation=None):
    """k_attend_chunk<.., WINDOW> for ONE head in float64: q [n_q][rpp] query rows as vectors [n_q][rpp][d], K / V [pos_end + base +
    n_q][d] by absolute position.  The walk (t_first, the pieces clipped by it, the held tiles behind the pool tiles), the staging
    (zeros for what no row of the block sees, beyond pos_end and beyond the held positions), the score test with the row's lower bound
    re-based per part, the skipping of tiles by a wave, the running maximum with the m_use path, and k_chunk_combine's merge in
    ascending piece order.  mutation: one of the kernel's rules broken, to show what the tests would see."""
    per, n_pool, held_n, d = 64 // rpp, _ceil(pos_end, 32), base + n_q, K.shape[1]
    lo_of = lambda j: max(0, pos_end + base + j + 1 - window - (mutation == "bound one lower") + (mutation == "bound one higher"))
    out = np.zeros((n_q, rpp, d))
    lse = np.zeros((n_q, rpp))
    for j_first in range(0, n_q, per):
        j_last = min(j_first + per, n_q) - 1
        n_tiles = n_pool + ((base + j_last) >> 5) + 1
        lo_blk = max(0, pos_end + base + j_first + 1 - window)
        t_first = lo_blk >> 5 if lo_blk < pos_end else n_pool + ((lo_blk - pos_end) >> 5)
        if mutation == "walk one tile late":
            t_first += 1
        lo_held = max(0, lo_blk - pos_end)
        parts = []
        for piece in range(pieces):
            piece_first = first_tile + piece * tpp
            t_begin = max(piece_first, t_first)
            t_end = n_tiles if piece + 1 == pieces else min(piece_first + tpp, n_pool)
            if mutation == "empty piece walks its first tile" and piece + 1 != pieces:
                t_end = max(t_end, t_begin + 1)
            acc, m_run, l_run = np.zeros((per, rpp, d)), np.full((per, rpp), -np.inf), np.zeros((per, rpp))
            for tile in range(t_begin, t_end):
                held = tile >= n_pool
                t_base = 32 * (tile - n_pool) if held else 32 * tile
                Kt, Vt = np.zeros((32, d)), np.zeros((32, d))                # staging: zeros unless a live row of the block may see it
                for t in range(t_base, t_base + 32):
                    if held and t < held_n and t >= lo_held:
                        Kt[t - t_base], Vt[t - t_base] = K[pos_end + t], V[pos_end + t]
                    if not held and t < pos_end and t >= lo_blk:
                        Kt[t - t_base], Vt[t - t_base] = K[t], V[t]
                    if mutation == "stage below the bound" and (t < pos_end if not held else t < held_n):
                        Kt[t - t_base], Vt[t - t_base] = (K[t], V[t]) if not held else (K[pos_end + t], V[pos_end + t])
                for jj in range(per):
                    j = j_first + jj
                    if j >= n_q:
                        continue
                    wave_j = j_first + (16 * ((jj * rpp) // 16)) // rpp                   # the first row of the wave that owns row jj
                    wave_lo = max(0, pos_end + base + wave_j + 1 - window)
                    wave_lo_part = max(0, wave_lo - pos_end) if held else wave_lo
                    wave_t_last = base + min(j_first + (16 * ((jj * rpp) // 16) + 15) // rpp, j_last)
                    if (held and t_base > wave_t_last) or t_base + 31 < wave_lo_part:
                        continue
                    limit = base + j + 1 if held else pos_end
                    lower = max(0, lo_of(j) - pos_end) if held else lo_of(j)
                    if mutation == "pool bound dropped" and not held:
                        lower = 0
                    if mutation == "held bound dropped" and held:
                        lower = 0
                    t = np.arange(t_base, t_base + 32)
                    seen = (t >= lower) & (t < limit)
                    for r in range(rpp):
                        s = np.where(seen, Kt @ q[j, r], -np.inf)
                        m_new = max(m_run[jj, r], s.max())
                        m_use = 0.0 if m_new == -np.inf else m_new
                        alpha = np.exp(m_run[jj, r] - m_use)
                        p = np.exp(s - m_use)
                        l_run[jj, r] = l_run[jj, r] * alpha + p.sum()
                        m_run[jj, r] = m_new
                        acc[jj, r] = acc[jj, r] * alpha + p @ Vt
            parts.append((acc, m_run, l_run))
        M = np.max([p[1] for p in parts], axis=0)
        m_use = np.where(M == -np.inf, 0.0, M)
        num, den = np.zeros((per, rpp, d)), np.zeros((per, rpp))
        for acc, m, l in parts:
            w = np.exp(m - m_use)
            num += acc * w[..., None]
            den += l * w
        n = j_last + 1 - j_first
        with np.errstate(invalid="ignore", divide="ignore"):
            out[j_first:j_last + 1] = (num / den[..., None])[:n]
            lse[j_first:j_last + 1] = (M + np.log(den))[:n]
    return out, lse


def _reference(pos_end, base, n_q, rpp, window, q, K, V):
    out, lse = np.zeros((n_q, rpp, K.shape[1])), np.zeros((n_q, rpp))
    for j in range(n_q):
        P = pos_end + base + j
        lo = max(0, P + 1 - window)
        for r in range(rpp):
            s = K[lo:P + 1] @ q[j, r]
            p = np.exp(s - s.max())
            out[j, r], lse[j, r] = (p @ V[lo:P + 1]) / p.sum(), s.max() + np.log(p.sum())
    return out, lse


# (pos_end, base, n_q, rows_per_pos, window): the bound inside a pool tile and on its edge, inside the last partial pool tile, on the
# pool / held seam and on the tail, inside held tiles (later blocks read no pool tile); odd and even bounds; windows of 1 and 2
EMULATED = [(98, 0, 70, 4, 40), (98, 1, 70, 4, 33), (64, 1, 33, 16, 32), (64, 0, 33, 1, 31), (36, 1, 17, 4, 2), (2, 0, 70, 1, 64),
            (0, 1, 70, 4, 1), (98, 1, 20, 16, 100), (200, 0, 70, 4, 100), (480, 1, 70, 1, 300), (480, 0, 1, 8, 65), (481 - 1, 1, 1, 8, 3)]


def _emulation_inputs(pos_end, base, n_q, rpp, hostile=True):
    """random rows; with `hostile`, V rows of +-1000 everywhere -- a row that wrongly sees one position more or less moves by far more
    than rounding, as the GPU tests' replaced and hostile rows do"""
    rng = np.random.default_rng(pos_end * 7 + base * 3 + n_q + rpp)
    total, d = pos_end + base + n_q, 8
    q, K, V = rng.standard_normal((n_q, rpp, d)), rng.standard_normal((total, d)), rng.standard_normal((total, d))
    if hostile:
        V *= 1000.0 * rng.choice([-1.0, 1.0], size=(total, 1))
    return q, K, V


def _plans(pos_end, base, window):
    """(pieces, tiles per piece, first tile) as the engine plans them: whole, and forced 2, 3, 5 and 64 pieces over the tiles left"""
    plans = [(1, 0, 0)]
    for n_splits in (2, 3, 5, 64):
        p, t, _, f = SpeckvKVConnector.chunk_pieces([1], [pos_end + base], 1, n_splits, 256, window=window)
        plans.append((p[0], t[0], f[0]))
    return plans


def test_the_emulated_kernel_is_the_windowed_softmax():
    """the walk, the staging with zeros, the two-sided test, the skipping by waves and the empty pieces, restated in float64, give the
    float64 windowed softmax to rounding -- for the whole walk and for every piece count"""
    for case in EMULATED:
        pos_end, base, n_q, rpp, window = case
        q, K, V = _emulation_inputs(pos_end, base, n_q, rpp)
        want, wlse = _reference(pos_end, base, n_q, rpp, window, q, K, V)
        for pieces, tpp, first in _plans(pos_end, base, window):
            got, lse = _emulate(pos_end, base, n_q, rpp, window, q, K, V, pieces, tpp, first)
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(lse)), (case, pieces)
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9) and np.allclose(lse, wlse, rtol=1e-9, atol=1e-9), (case, pieces)


@pytest.mark.parametrize("mutation", ["bound one lower", "bound one higher", "pool bound dropped", "held bound dropped", "walk one tile late",
                                      "empty piece walks its first tile"])
def test_every_mutation_of_the_rule_leaves_the_float64_bound(mutation):
    """each broken rule moves some row of the emulated cases far outside |err| <= 2e-3 sum p|v| + 1e-6 (or makes it non-finite): the
    float64 tests of tests/test_gpu_chunk_window.py run these shapes' like on the device and would fail"""
    broken = 0
    for case in EMULATED:
        pos_end, base, n_q, rpp, window = case
        q, K, V = _emulation_inputs(pos_end, base, n_q, rpp)
        want, _ = _reference(pos_end, base, n_q, rpp, window, q, K, V)
        mag, _ = _reference(pos_end, base, n_q, rpp, window, q, K, np.abs(V))
        for pieces, tpp, first in _plans(pos_end, base, window) if mutation.startswith("empty") else [(1, 0, 0)]:
            got, _ = _emulate(pos_end, base, n_q, rpp, window, q, K, V, pieces, tpp, first, mutation=mutation)
            with np.errstate(invalid="ignore"):
                broken += not np.all(np.abs(got - want) <= 2e-3 * mag + 1e-6)
    assert broken > 0, mutation


def test_zero_staging_keeps_hostile_rows_below_the_bound_out_of_the_product():
    """rows below the block's bound that hold inf: weighed 0 they would still poison the product as 0 x inf; staged as zeros they do
    not.  The mutation that stages them shows the NaN the zeros prevent"""
    pos_end, base, n_q, rpp, window = 98, 0, 16, 4, 40                   # lo(0) = 59: positions 0..58 are seen by no row
    q, K, V = _emulation_inputs(pos_end, base, n_q, rpp, hostile=False)
    V[:59] = np.inf
    want, _ = _reference(pos_end, base, n_q, rpp, window, q, K, V)
    got, _ = _emulate(pos_end, base, n_q, rpp, window, q, K, V)
    assert np.all(np.isfinite(got)) and np.allclose(got, want, rtol=1e-9, atol=1e-9)
    with np.errstate(invalid="ignore"):
        bad, _ = _emulate(pos_end, base, n_q, rpp, window, q, K, V, mutation="stage below the bound")
    assert np.isnan(bad).any()
