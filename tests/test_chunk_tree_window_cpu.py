"""Draft trees on sliding-window layers, without a GPU: speckv_ext_attend_chunk_tree_window is declared, exported and bound; the
connector's depth and mask tables against brute-force restatements of the semantics (a node's position is its DEPTH); attend_tree's
refusals and the calls it issues; and a float64 emulation of the kernel's MASKED + WINDOW walk -- pool bound by depth, held part by
the mask words, zeros below depth 0's bound, every block from the same first tile -- against the brute-force windowed tree softmax,
with the mutations that would break it.

The semantics restated HERE (never taken from the code under test): a request holds length = pos_end + base positions; node j of depth
d sits at P = length + d and, under a window W, sees [lo, P] on its root path, lo = max(0, P + 1 - W): stored t iff lo <= t < pos_end,
the tail (absolute position pos_end) iff base == 1 and pos_end >= lo, ancestor a iff length + depth(a) >= lo, itself always."""
import ctypes as C
import fnmatch
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
WINDOWS = [1, 2, 3, 31, 32, 33, 64, 10 ** 6]
SIZES = [1, 5, 16, 33, 70]


# ----------------------------------------------------------------------------- declared, exported, bound
def test_the_tree_window_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_attend_chunk_tree_window\s*\(", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    # declared at the end of the header, behind every other entry
    last = [m.group(1) for m in re.finditer(r"speckv_status_t\s+(speckv_ext_\w+)\s*\(", header)][-1]
    assert last == "speckv_ext_attend_chunk_tree_window"
    doc = header[header.index("speckv_ext_attend_chunk_tree_window:"):]
    assert "STORED POSITIONS ONLY" in doc and "MUST COME FROM THE SAME TREE" in doc and "NOT" in doc and "nothing is freed" in doc
    # the split entry's parameters in order, with `d_depth, window` directly behind mask_words
    params = lambda name: [p.split("/*")[0].split()[-1].lstrip("*") for p in
                           re.search(name + r"\s*\((.*?)\);", header[header.index("speckv_status_t " + name + "("):], re.S).group(1).split(",")]
    split, tree = params("speckv_ext_attend_chunk_split"), params("speckv_ext_attend_chunk_tree_window")
    at = split.index("mask_words") + 1
    assert tree == split[:at] + ["d_depth", "window"] + split[at:]
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", exports, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_attend_chunk_tree_window", p) for p in patterns), patterns
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_tree_window"]
    ssig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_attend_chunk_split"]
    assert len(sig) == len(ssig) + 2 == 25
    assert sig[:18] == ssig[:18] and sig[18] is C.c_void_p and sig[19] is C.c_uint32 and sig[20:] == ssig[18:]
    assert callable(speckv_ctypes.SpeckvLib.attend_chunk_tree_window)
    assert callable(SpeckvKVConnector.attend_tree) and callable(SpeckvKVConnector.chunk_tree_depths)
    capi = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_attend_chunk_tree_window\s*\(", capi)


def test_the_library_exports_the_entry_and_keeps_its_abi_version():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_chunk_tree_window")
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6


def test_the_tree_window_entry_on_the_null_engine_answers_as_the_split_entry_does():
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
                                   0, 0, at, 1, 5, 1.0, at, 0, 1)
        for window, n_splits in ((0, 1), (1, 1), (7, 0), (7, 5), (10 ** 6, 64)):
            with pytest.raises(SpeckvError) as tree:
                lib.attend_chunk_tree_window(u64(a), 0, at, 1, 1, np.asarray([0], np.uint32), np.asarray([1], np.uint32), at, at, 1024, 1024,
                                             None, 0, 0, 0, at, 1, at, window, n_splits, 1.0, at, 0, 1)
            assert tree.value.status == split.value.status == -2              # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- trees, and the semantics by brute force
def _trees(S, seed):
    """chain, star and two random trees of S nodes; one more whose node order puts deep nodes in front of roots"""
    rng = np.random.default_rng(seed)
    out = {"chain": list(range(-1, S - 1)), "star": [-1] * S,
           "random": [int(rng.integers(-1, j)) for j in range(S)], "bushy": [int(rng.integers(max(-1, j - 4), j)) for j in range(S)]}
    out["deep first"] = [-1 if j % 9 == 0 else j - 1 for j in range(S)]     # chains of 9: a root behind a node of depth 8, over and over
    return out


def _brute_depth(tree, j):
    d = 0
    while tree[j] >= 0:
        j, d = tree[j], d + 1
    return d


def _brute_live(tree, j, n):
    while j >= 0:
        if j >= n:
            return False
        j = tree[j]
    return True


def _brute_sees(tree, j, pos_end, base, window):
    """what node j sees by the semantics of the module docstring: (lo, tail seen, set of new nodes seen)"""
    length = pos_end + base
    lo = max(0, length + _brute_depth(tree, j) + 1 - window)
    nodes, a = {j}, tree[j]
    while a >= 0:
        if length + _brute_depth(tree, a) >= lo:
            nodes.add(a)
        a = tree[a]
    return lo, bool(base == 1 and pos_end >= lo), nodes


def test_chunk_tree_depths_against_a_walk_up_the_parents():
    for S in SIZES:
        trees = _trees(S, 100 + S)
        for name, tree in trees.items():
            want = [_brute_depth(tree, j) for j in range(S)]
            assert SpeckvKVConnector.chunk_tree_depths(tree) == [want], (S, name)
            assert SpeckvKVConnector.chunk_tree_depths(tree, 3) == [want] * 3
        per_request = list(trees.values())
        assert SpeckvKVConnector.chunk_tree_depths(per_request, len(per_request)) == [[_brute_depth(t, j) for j in range(S)] for t in per_request]
    for bad in ([0], [-1, 1], [-2], [], [-1, True]):
        with pytest.raises(ValueError):
            SpeckvKVConnector.chunk_tree_depths(bad)


@pytest.mark.parametrize("S", SIZES)
def test_chunk_tree_masks_under_a_window_against_the_brute_force_visibility(S):
    """every bit of every row, both bases, ragged n_new, for pos_end of 0, 2 and 64 (the rows do not depend on the length): S = 33
    and 70 cross the word boundaries at base 0 and base 1"""
    words = (S + 1 + 31) // 32
    for name, tree in _trees(S, 200 + S).items():
        for n in sorted({S, max(S - 1, 0), (2 * S) // 3, 1, 0}):
            for window in WINDOWS:
                rows = SpeckvKVConnector.chunk_tree_masks([tree, tree], [0, 1], [n, n], window=window)
                assert len(rows) == 2 and all(len(r) == S and all(len(w) == words for w in r) for r in rows)
                for base in (0, 1):
                    for j in range(S):
                        got = sum(w << (32 * k) for k, w in enumerate(rows[base][j]))
                        if not _brute_live(tree, j, n):
                            assert got == 0, (name, n, window, base, j)
                            continue
                        for pos_end in (0, 2, 64):
                            _, tail, nodes = _brute_sees(tree, j, pos_end, base, window)
                            want = (1 if tail else 0) | sum(1 << (base + a) for a in nodes)
                            assert got == want, (name, n, window, base, j, pos_end)
                        assert got >> (base + j) & 1                            # its own bit always stays


def test_chunk_tree_masks_without_a_window_is_unchanged():
    """window=None / 0 give the rows of the call without the argument, and those are the ancestor rows built here bit by bit; a window
    beyond every depth gives them too"""
    for S in SIZES:
        for name, tree in _trees(S, 300 + S).items():
            n = [S, max(S - 2, 0)]
            today = SpeckvKVConnector.chunk_tree_masks(tree, [0, 1], n)
            for window in (None, 0, S + 1, 10 ** 6):
                assert SpeckvKVConnector.chunk_tree_masks(tree, [0, 1], n, window=window) == today, (S, name, window)
            for base in (0, 1):
                for j in range(S):
                    want, a = 0, j
                    if _brute_live(tree, j, n[base]):
                        want = base
                        while a >= 0:
                            want |= 1 << (base + a)
                            a = tree[a]
                    assert sum(w << (32 * k) for k, w in enumerate(today[base][j])) == want
    for bad in (-1, True, 2.5, "8"):
        with pytest.raises(ValueError, match="window"):
            SpeckvKVConnector.chunk_tree_masks([-1, 0], [0], window=bad)


# ----------------------------------------------------------------------------- the connector
def _conn(lib, lengths=(0,)):
    L, H, D, T = 2, 8, 128, 64
    conn = SpeckvKVConnector(lib, L, H, D, T, "fp8")
    for rid, n in enumerate(lengths, 1):
        conn.add_request(rid)
        conn.requests[rid].length = n
    return conn


@pytest.mark.parametrize("window", [None, 0, 1, 8, 10 ** 6])
def test_attend_tree_refuses_before_any_library_call(window):
    L, H, D, S, R = 2, 8, 128, 5, 4
    conn = _conn(_SilentLib())
    q, kv = _Shape(1, S, H, R, D), _Shape(1, S, L, H, D)
    tree = [-1, 0, 0, 1, 1]
    for bad in (-1, True, 2.5, "8", [8]):
        with pytest.raises(ValueError, match="window"):
            conn.attend_tree(0, [1], q, kv, kv, 1.0, tree, window=bad)
    for splits in (65, -1, True, 1.5):
        with pytest.raises(ValueError, match="splits"):
            conn.attend_tree(0, [1], q, kv, kv, 1.0, tree, splits=splits, window=window)
    for parents in ([-1, 0, 0, 1], [-1, 0, 0, 1, 4], [0, 0, 0, 1, 1], [[-1, 0, 0, 1, 1]] * 2, None):
        with pytest.raises(ValueError, match="parents"):
            conn.attend_tree(0, [1], q, kv, kv, 1.0, parents, window=window)
    with pytest.raises(ValueError, match="rows_per_pos"):
        conn.attend_tree(0, [1], _Shape(1, S, H, 3, D), kv, kv, 1.0, tree, window=window)
    with pytest.raises(ValueError, match="q must be"):
        conn.attend_tree(0, [1], q, _Shape(1, S + 1, L, H, D), kv, 1.0, tree, window=window)
    with pytest.raises(ValueError, match="layer"):
        conn.attend_tree(2, [1], q, kv, kv, 1.0, tree, window=window)
    with pytest.raises(ValueError, match="n_new"):
        conn.attend_tree(0, [1], q, kv, kv, 1.0, tree, n_new=[S + 1], window=window)
    with pytest.raises(ValueError, match="max_tokens"):
        conn.attend_tree(0, [1], _Shape(1, 70, H, R, D), _Shape(1, 70, L, H, D), _Shape(1, 70, L, H, D), 1.0, [-1] * 70, window=window)


def test_attend_chunk_still_refuses_parents_with_a_window():
    L, H, D, S, R = 2, 8, 128, 5, 4
    conn = _conn(_SilentLib())
    q, kv = _Shape(1, S, H, R, D), _Shape(1, S, L, H, D)
    for splits in (0, 1, 5):
        with pytest.raises(ValueError, match="window does not combine with parents"):
            conn.attend_chunk(0, [1], q, kv, kv, 1.0, parents=[-1, 0, 0, 1, 1], splits=splits, window=8)


class _Tensor:
    """what the chunk step asks of a contiguous tensor, without a device; `array` = what a table was made from"""

    def __init__(self, shape, ptr, array=None):
        self.shape, self.ptr, self.array = tuple(shape), ptr, array
        self.strides = tuple(int(np.prod(shape[k + 1:])) for k in range(len(shape)))

    def contiguous(self): return self
    def pin_memory(self): return self
    def to(self, *a, **kw): return self
    def stride(self, k=None): return self.strides if k is None else self.strides[k]
    def data_ptr(self): return self.ptr


def _stub_torch(made):
    """a stand-in for the torch module as the chunk step uses it on its way to the library; tables made by from_numpy are kept in
    `made` (pointer -> array)"""
    stream = types.SimpleNamespace(cuda_stream=0x5000, wait_stream=lambda other: None)

    class _Ctx:
        def __init__(self, *a): pass
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    def from_numpy(a):
        ptr = 0x100000 + 0x1000 * len(made)
        made[ptr] = a.copy()
        return _Tensor(a.shape, ptr, made[ptr])

    cuda = types.SimpleNamespace(current_stream=lambda: stream, Stream=lambda: stream, stream=_Ctx)
    make = lambda shape, dtype=None, device=None: _Tensor(shape, 0x9000)
    return types.SimpleNamespace(cuda=cuda, empty=make, zeros=make, float32="float32", from_numpy=from_numpy)


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
        if name in ("attend_chunk", "attend_chunk_split", "attend_chunk_masked", "attend_chunk_window", "attend_chunk_tree_window"):
            return self._note(name)
        return super().__getattr__(name)


def test_attend_tree_without_a_window_calls_what_attend_chunk_calls_and_with_one_the_new_entry(monkeypatch):
    """window=None / 0: exactly the calls of attend_chunk(parents=...), the same table.  window=W: speckv_ext_attend_chunk_tree_window
    with the split entry's arguments, `depths, W` behind the mask pair, the mask rows those of chunk_tree_masks(window=W) and the
    depths those of chunk_tree_depths; the tables are made once per window and shared by the layers; local and global layers each
    keep theirs"""
    made = {}
    monkeypatch.setitem(sys.modules, "torch", _stub_torch(made))
    L, H, D, S, R = 2, 8, 128, 5, 4
    lib = _Recorder()
    conn = _conn(lib, (0, 12))                                         # even lengths: no tail rows to gather without a device
    q, k, v = _Tensor((2, S, H, R, D), 0x1000), _Tensor((2, S, L, H, D), 0x2000), _Tensor((2, S, L, H, D), 0x3000)
    trees = [[-1, 0, 0, 1, 1], [-1, 0, 1, 2, -1]]
    live = [S, 4]
    for splits in (1, 0, 7):
        del lib.calls[:]
        conn.attend_chunk(1, [1, 2], q, k, v, 0.5, live, parents=trees, splits=splits)
        conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, splits=splits)
        conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, splits=splits, window=0)
        today, none, zero = lib.calls
        assert today[0] == ("attend_chunk_masked" if splits == 1 else "attend_chunk_split")
        assert none == today and zero == today
        n_tables = len(made)
        del lib.calls[:]
        conn.attend_chunk(1, [1, 2], q, k, v, 0.5, live, parents=trees, splits=0 if splits == 1 else splits)
        conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, splits=splits, window=3)
        conn.attend_tree(0, [1, 2], q, k, v, 0.5, trees, live, splits=splits, window=3)          # the step's other layer
        conn.attend_tree(0, [1, 2], q, k, v, 0.5, trees, live, splits=splits)                    # a global layer in between
        conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, splits=splits, window=3)
        split, win, win0, glob, again = lib.calls
        assert split[0] == "attend_chunk_split" and win[0] == win0[0] == again[0] == "attend_chunk_tree_window"
        # (name, handles, layer, q, C, R, pos_end, n_q, k, v, strides x 2, tail_idx, kt, vt, tail stride | mask, words | depth, W | splits, rest)
        assert win[1:16] == split[1:16] and win[17] == split[17] == 1 and win[19:21] == (3, splits) and win[21:] == split[19:]
        assert win[6] == [0, 12] and win[7] == live
        assert np.array_equal(made[win[16]].view(np.uint32), np.asarray(SpeckvKVConnector.chunk_tree_masks(trees, [0, 0], live, window=3), np.uint32))
        assert np.array_equal(made[win[18]].view(np.uint32), np.asarray([[0, 1, 1, 2, 2], [0, 1, 2, 3, 0]], np.uint32))
        assert made[win[18]].shape == (2, S) and made[win[16]].shape == (2, S, 1)
        assert (win0[16], win0[18]) == (win[16], win[18]) == (again[16], again[18])              # one table per window, shared
        assert glob[16] == split[16] != win[16]                                                   # the global layers' table beside it
        assert len(made) <= n_tables + 2
    # a tree, live count or window that differs makes new tables
    del lib.calls[:]
    conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, window=3)
    conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, live, window=2)
    conn.attend_tree(1, [1, 2], q, k, v, 0.5, trees, [S, 3], window=3)
    a, b, c = lib.calls
    assert len({a[16], b[16], c[16]}) == 3
    assert np.array_equal(made[b[16]].view(np.uint32), np.asarray(SpeckvKVConnector.chunk_tree_masks(trees, [0, 0], live, window=2), np.uint32))


# ----------------------------------------------------------------------------- what the kernel computes, restated in float64
def _ceil(a, b):
    return -(-a // b)


def _emulate(pos_end, base, tree, n, rpp, window, q, K, V, pieces=1, tpp=0, first_tile=0, mutation=None):
    """k_attend_chunk<.., MASKED, .., WINDOW> for ONE head in float64: S = len(tree) nodes, the first n live by count; q [S][rpp][d],
    K / V [pos_end + base + S][d] (stored, tail, nodes).  Every block walks from the tile of depth 0's bound, positions below that
    bound are staged as zeros, a pool score needs t >= the bound of the row's DEPTH, a held score its mask bit under the causal
    bound, waves skip held tiles behind their last row only, pieces merge in ascending order.  mutation: one rule broken."""
    S = len(tree)
    per, n_pool, held_n, d = 64 // rpp, _ceil(pos_end, 32), base + n, K.shape[1]
    masks = SpeckvKVConnector.chunk_tree_masks(tree, [base], [n], window=window)[0]
    if mutation == "tail test dropped":
        masks = [[w | (1 if base and k == 0 and any(row) else 0) for k, w in enumerate(row)] for row in masks]
    depth = [_brute_depth(tree, j) for j in range(S)]
    shift = (mutation == "bound one higher") - (mutation == "bound one lower")
    lo_of = lambda dj: max(0, pos_end + base + dj + 1 - window + shift)
    lo0 = max(0, pos_end + base + 1 - window)
    t_first = lo0 >> 5 if lo0 < pos_end else n_pool
    out, lse = np.zeros((S, rpp, d)), np.zeros((S, rpp))
    for j_first in range(0, n, per):
        j_last = min(j_first + per, n) - 1
        n_tiles = n_pool + ((base + j_last) >> 5) + 1
        parts = []
        for piece in range(pieces):
            piece_first = first_tile + piece * tpp
            t_begin = max(piece_first, t_first)
            t_end = n_tiles if piece + 1 == pieces else min(piece_first + tpp, n_pool)
            acc, m_run, l_run = np.zeros((per, rpp, d)), np.full((per, rpp), -np.inf), np.zeros((per, rpp))
            for tile in range(t_begin, t_end):
                held = tile >= n_pool
                t_base = 32 * (tile - n_pool) if held else 32 * tile
                Kt, Vt = np.zeros((32, d)), np.zeros((32, d))
                for t in range(t_base, t_base + 32):
                    if held and t < held_n:
                        Kt[t - t_base], Vt[t - t_base] = K[pos_end + t], V[pos_end + t]
                    if not held and t < pos_end and t >= lo0:
                        Kt[t - t_base], Vt[t - t_base] = K[t], V[t]
                for jj in range(per):
                    j = j_first + jj
                    if j >= n or not (masks[j][(base + j) >> 5] >> ((base + j) & 31)) & 1:
                        continue
                    wave_first = j_first + (16 * ((jj * rpp) // 16)) // rpp
                    wave_t_last = base + min(j_first + (16 * ((jj * rpp) // 16) + 15) // rpp, j_last)
                    if held and t_base > wave_t_last:
                        continue
                    if mutation == "bound from the wave's first row" and not held and t_base + 31 < lo_of(depth[wave_first]):
                        continue
                    row_lo = lo_of(j if mutation == "bound from the index" else depth[j])
                    t = np.arange(t_base, t_base + 32)
                    if held:
                        word = masks[j][t_base >> 5]
                        seen = np.asarray([(word >> k) & 1 for k in range(32)], bool) & (t < base + j + 1)
                    else:
                        seen = (t >= row_lo) & (t < pos_end)
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
        cnt = j_last + 1 - j_first
        with np.errstate(invalid="ignore", divide="ignore"):
            out[j_first:j_last + 1] = (num / den[..., None])[:cnt]
            lse[j_first:j_last + 1] = (M + np.log(den))[:cnt]
    return out, lse


def _reference(pos_end, base, tree, n, rpp, window, q, K, V):
    """the windowed tree softmax by the semantics: (out, lse, live) -- rows of dead nodes stay 0"""
    S = len(tree)
    out, lse, live = np.zeros((S, rpp, K.shape[1])), np.zeros((S, rpp)), np.zeros(S, bool)
    for j in range(S):
        if not _brute_live(tree, j, n):
            continue
        live[j] = True
        lo, tail, nodes = _brute_sees(tree, j, pos_end, base, window)
        at = list(range(min(lo, pos_end), pos_end)) + ([pos_end] if tail else []) + [pos_end + base + a for a in sorted(nodes)]
        for r in range(rpp):
            s = K[at] @ q[j, r]
            p = np.exp(s - s.max())
            out[j, r], lse[j, r] = (p @ V[at]) / p.sum(), s.max() + np.log(p.sum())
    return out, lse, live


def _case_tree(kind, S):
    return _trees(S, 400 + S)[kind]


# (pos_end, base, tree, S, live, rows_per_pos, window): depth 0's bound inside a pool tile, on its edge, on the pool / held seam and
# on the tail; deep nodes in front of roots inside one wave (rows_per_pos 4: 4 nodes a wave; 1: 16) and one block; windows 1 and 2;
# a chain deeper than the window; more than one block; dead nodes
EMULATED = [(98, 0, "deep first", 70, 70, 4, 40), (98, 1, "deep first", 70, 70, 1, 33), (98, 1, "random", 70, 61, 4, 40),
            (64, 1, "bushy", 33, 33, 16, 32), (64, 0, "star", 33, 33, 1, 31), (36, 1, "chain", 17, 17, 4, 2), (2, 0, "chain", 70, 70, 1, 64),
            (0, 1, "random", 70, 70, 4, 1), (98, 1, "chain", 20, 20, 16, 100), (200, 0, "deep first", 70, 70, 4, 100),
            (480, 1, "random", 70, 70, 1, 300), (480, 0, "bushy", 5, 5, 8, 65), (480, 1, "deep first", 16, 12, 8, 3)]


def _emulation_inputs(pos_end, base, S, rpp):
    """random rows, V rows of +-1000 everywhere: a row that wrongly sees one position more or less moves by far more than rounding"""
    rng = np.random.default_rng(pos_end * 7 + base * 3 + S + rpp)
    total, d = pos_end + base + S, 8
    q, K, V = rng.standard_normal((S, rpp, d)), rng.standard_normal((total, d)), rng.standard_normal((total, d))
    V *= 1000.0 * rng.choice([-1.0, 1.0], size=(total, 1))
    return q, K, V


def _plans(pos_end, base, window):
    """(pieces, tiles per piece, first tile) as the engine plans them: whole, and forced 2, 3, 5 and 64 pieces over the tiles left"""
    plans = [(1, 0, 0)]
    for n_splits in (2, 3, 5, 64):
        p, t, _, f = SpeckvKVConnector.chunk_pieces([1], [pos_end + base], 1, n_splits, 256, window=window)
        plans.append((p[0], t[0], f[0]))
    return plans


def test_the_emulated_walk_is_the_windowed_tree_softmax():
    for case in EMULATED:
        pos_end, base, kind, S, n, rpp, window = case
        tree = _case_tree(kind, S)
        q, K, V = _emulation_inputs(pos_end, base, S, rpp)
        want, wlse, live = _reference(pos_end, base, tree, n, rpp, window, q, K, V)
        for pieces, tpp, first in _plans(pos_end, base, window):
            got, lse = _emulate(pos_end, base, tree, n, rpp, window, q, K, V, pieces, tpp, first)
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(lse)), (case, pieces)
            assert not got[~live].any() and live[:n].any()
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9) and np.allclose(lse, wlse, rtol=1e-9, atol=1e-9), (case, pieces)


def test_a_chain_given_as_a_tree_is_the_windowed_chain():
    """parents[j] = j - 1: depth = index, and the reference is the chain's: positions [max(0, P + 1 - W), P]"""
    for pos_end, base, S, rpp, window in ((98, 1, 40, 4, 33), (64, 0, 70, 1, 2), (2, 1, 33, 16, 1)):
        tree = list(range(-1, S - 1))
        q, K, V = _emulation_inputs(pos_end, base, S, rpp)
        got, _ = _emulate(pos_end, base, tree, S, rpp, window, q, K, V)
        for j in range(S):
            P = pos_end + base + j
            lo = max(0, P + 1 - window)
            for r in range(rpp):
                s = K[lo:P + 1] @ q[j, r]
                p = np.exp(s - s.max())
                assert np.allclose(got[j, r], (p @ V[lo:P + 1]) / p.sum(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("mutation", ["bound from the index", "bound from the wave's first row", "bound one lower", "bound one higher",
                                      "tail test dropped"])
def test_every_mutation_of_the_rule_leaves_the_float64_bound(mutation):
    """each broken rule moves some row of the emulated cases far outside |err| <= 2e-3 sum p|v| + 1e-6: the float64 tests of
    tests/test_gpu_chunk_tree_window.py run these shapes' like on the device and would fail"""
    broken = []
    for case in EMULATED:
        pos_end, base, kind, S, n, rpp, window = case
        tree = _case_tree(kind, S)
        q, K, V = _emulation_inputs(pos_end, base, S, rpp)
        want, _, live = _reference(pos_end, base, tree, n, rpp, window, q, K, V)
        mag, _, _ = _reference(pos_end, base, tree, n, rpp, window, q, K, np.abs(V))
        got, _ = _emulate(pos_end, base, tree, n, rpp, window, q, K, V, mutation=mutation)
        with np.errstate(invalid="ignore"):
            if not np.all(np.abs(got - want)[live] <= (2e-3 * mag + 1e-6)[live]):
                broken.append(case)
    assert broken, mutation
    if mutation == "bound from the wave's first row":                       # it takes a deep node in front of a root to see this one
        assert all(case[2] in ("deep first", "random", "bushy") for case in broken)
