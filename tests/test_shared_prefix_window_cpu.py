"""Not -m gpu: shared-prefix attention under a sliding window and under draft trees (speckv_ext_attend_prefix_fold_window,
speckv_ext_prefix_window_walk, SpeckvLib.attend_prefix_fold_window / prefix_window_walk, SpeckvKVConnector.prefix_window_walk /
attend_shared(window=) / attend_chunk_shared(window=, parents=) / attend_tree_shared) as far as it can be judged without a device.

The walk rule through the export against the connector's restatement and against a brute-force enumeration of what every row sees;
a float64 emulation of k_attend_prefix<.., WINDOW>'s walk -- the first tile, the per-row range, the skipping of tiles, pieces over
the tiles that are left, the merge, the rule that decides which rows are folded -- against a plain float64 softmax over the last W
positions of prefix + own, with what each mutation of a rule would compute; the binding against the header; the connector's
refusals against a library that must not be called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
ENTRY, PARENT = "speckv_ext_attend_prefix_fold_window", "speckv_ext_attend_prefix_fold"
ARRAYS = {"prefix_handles": (C.c_uint64, np.uint64, [901, 902]), "first_member": (C.c_uint32, np.uint32, [0, 2, 3]),
          "prefix_len": (C.c_uint32, np.uint32, [10, 20, 30]), "n_q": (C.c_uint32, np.uint32, [1, 2, 3]),
          "own_seen": (C.c_uint32, np.uint32, [7, 0, 9])}

PREFIX_LENS = [0, 2, 36, 64, 98, 254]
OWN_SEEN = [0, 1, 2, 37, 64]
WINDOWS = [1, 2, 31, 32, 33, 40, 64, 100, 300]
DEPTHS = 6                                                                # depths 0..5


def declared(entry=ENTRY):
    """[(name, is a pointer)] of the entry's parameters, in the header's order"""
    text = re.search(entry + r"\s*\((.*?)\);", HEADER[HEADER.index("speckv_status_t " + entry + "("):], re.S).group(1)
    return [(p.split()[-1].lstrip("*"), "*" in p) for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]


# ----------------------------------------------------------------------------- the binding against the header
def _call(values):
    lib, got = speckv_ctypes.SpeckvLib.__new__(speckv_ctypes.SpeckvLib), []
    lib._ext = lambda name, *args: got.append((name, args))
    lib.attend_prefix_fold_window(*[values[name] for name, _ in declared() if name != "n_groups"])
    assert len(got) == 1 and got[0][0] == ENTRY
    assert len(got[0][1]) == len(declared()) == len(speckv_ctypes._EXT_SIGNATURES[ENTRY])
    return dict(zip([name for name, _ in declared()], got[0][1]))


def _sentinels():
    values = {name: 0.375 if name == "sm_scale" else 1000 + k for k, (name, _) in enumerate(declared())}
    values.update({name: list(v[2]) for name, v in ARRAYS.items()})
    return values


def test_the_entry_is_the_fold_with_three_arguments_behind_n_q_and_keeps_the_abi_version():
    names, parent = [name for name, _ in declared()], [name for name, _ in declared(PARENT)]
    at = parent.index("n_q") + 1
    assert names == parent[:at] + ["own_seen", "d_depth", "window"] + parent[at:]
    assert [p for _, p in declared()] == [n in ARRAYS or n in ("d_q_f16", "d_depth", "d_out", "d_lse", "stream") for n in names]
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in HEADER
    doc = HEADER[HEADER.index(ENTRY + ":"):HEADER.index("speckv_status_t " + ENTRY + "(")]
    for phrase in ("own_seen", "DEAD", "prefix_len[m] + own_seen[m] + d - W", "W == 0", "may be NULL", "exactly the launches"):
        assert phrase in doc, phrase
    for (name, pointer), t in zip(declared(), speckv_ctypes._EXT_SIGNATURES[ENTRY]):
        assert (t is C.c_void_p) == pointer and (t is C.c_float) == (name == "sm_scale"), name
    walk = [name for name, _ in declared("speckv_ext_prefix_window_walk")]
    assert walk == ["n_groups", "first_member", "prefix_len", "own_seen", "n_q", "window", "out_first_tile", "out_n_tiles"]
    assert len(speckv_ctypes._EXT_SIGNATURES["speckv_ext_prefix_window_walk"]) == len(walk)


def test_every_argument_arrives_in_the_headers_position():
    values = _sentinels()
    got = _call(values)
    assert got["n_groups"] == 2
    for name, pointer in declared():
        if name in ARRAYS:
            assert isinstance(got[name], C.Array) and got[name]._type_ is ARRAYS[name][0] and list(got[name]) == values[name], name
        elif pointer:
            assert isinstance(got[name], C.c_void_p) and got[name].value == values[name], name
        elif name != "n_groups":
            assert got[name] == values[name], name


def test_numpy_arrays_arrive_by_their_own_data_pointer_and_absent_tables_as_null():
    values = _sentinels()
    arrays = {name: np.asarray(v[2], dtype=v[1]) for name, v in ARRAYS.items()}
    values.update(arrays)
    values["d_depth"] = 0
    got = _call(values)
    for name, a in arrays.items():
        assert isinstance(got[name], C.c_void_p) and got[name].value == a.ctypes.data, name
    assert got["d_depth"].value is None
    values.update(own_seen=None, d_depth=None)
    got = _call(values)
    assert got["own_seen"] is None and got["d_depth"].value is None


def test_the_entry_on_the_null_engine_answers_with_the_no_data_path_status():
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    raw = C.CDLL(pkg.build_library())
    assert hasattr(raw, ENTRY) and hasattr(raw, "speckv_ext_prefix_window_walk")
    raw.speckv_ext_abi_version.restype = C.c_uint32
    assert raw.speckv_ext_abi_version() == 6
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        before = bytes(lib.stats())
        for window in (0, 1, 40):
            with pytest.raises(SpeckvError) as err:
                lib.attend_prefix_fold_window(np.asarray([a], np.uint64), np.asarray([0, 1], np.uint32), 0, at, 1, 1, np.asarray([2], np.uint32),
                                              np.asarray([1], np.uint32), np.asarray([5], np.uint32), 0, window, 1, 1.0, at, at, 1)
            assert err.value.status == -2                                 # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- the walk rule
@pytest.fixture(scope="module")
def clib():
    lib = C.CDLL(pkg.build_library())                                     # no speckv_init: the walk needs none
    lib.speckv_ext_prefix_window_walk.restype = C.c_int
    lib.speckv_ext_prefix_window_walk.argtypes = [C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def _lib_walk(clib, first, lens, seen, n_q, window):
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)
    n = len(first) - 1
    t, c = u32([0] * n), u32([0] * n)
    assert clib.speckv_ext_prefix_window_walk(n, u32(first), u32(lens), u32(seen), u32(n_q), window, t, c) == 0
    return list(zip(list(t)[:n], list(c)[:n]))


def _seen(n_pre, own, d, window):
    """what the row of depth d sees of its prefix, from the statement alone: the row sees n_pre + own + d positions in all -- the
    prefix in front -- and under a window the last `window` of them"""
    total = n_pre + own + d
    return [t for t in range(n_pre) if not window or t >= total - window]


def _brute_walk(first, lens, seen, n_q, window):
    """per group: the tiles a row of a live pair sees something in, as (first, count) -- rows are a chain (depth = index)"""
    walks = []
    for a, b in zip(first, first[1:]):
        tiles = {t >> 5 for m in range(a, b) for d in range(n_q[m]) for t in _seen(lens[m], seen[m], d, window)}
        walks.append((min(tiles), max(tiles) + 1 - min(tiles)) if tiles else (0, 0))
    return walks


def _groups():
    """every (prefix_len, own_seen) alone, with 0, 1 and 6 live positions; then random groups of 1..7 members"""
    for n_pre in PREFIX_LENS:
        for own in OWN_SEEN:
            for live in (0, 1, DEPTHS):
                yield [0, 1], [n_pre], [own], [live]
    rng = np.random.default_rng(11)
    for _ in range(120):
        sizes = [int(rng.integers(1, 8)) for _ in range(int(rng.integers(1, 4)))]
        first = [0] + list(np.cumsum(sizes))
        n = first[-1]
        yield ([int(x) for x in first], [int(rng.choice(PREFIX_LENS)) for _ in range(n)], [int(rng.choice(OWN_SEEN)) for _ in range(n)],
               [int(rng.choice([0, 1, 3, DEPTHS])) for _ in range(n)])


def test_the_walk_rule_export_restatement_and_brute_force_agree(clib):
    kinds = set()
    for first, lens, seen, n_q in _groups():
        for window in WINDOWS + [0]:
            got = _lib_walk(clib, first, lens, seen, n_q, window)
            assert got == SpeckvKVConnector.prefix_window_walk(first, lens, seen, n_q, window or None), (first, lens, seen, n_q, window)
            assert got == _brute_walk(first, lens, seen, n_q, window), (first, lens, seen, n_q, window)
            for g, (a, b) in enumerate(zip(first, first[1:])):
                members = [m for m in range(a, b) if n_q[m] and lens[m]]
                alive = [m for m in members if _seen(lens[m], seen[m], 0, window)]
                if members:
                    kinds.add("all" if len(alive) == len(members) else "some" if alive else "none")
                # every row of every depth sees nothing below the first tile and nothing beyond the last
                for m in range(a, b):
                    for d in range(n_q[m]):
                        for t in _seen(lens[m], seen[m], d, window):
                            assert got[g][0] <= t >> 5 < got[g][0] + got[g][1]
    assert kinds == {"all", "some", "none"}


def test_the_bound_of_every_depth_through_the_export(clib):
    """prefix_window_lo depends on own_seen + depth alone, so the row of depth d of a member is the depth-0 row of a member alone
    that holds own_seen + d: the export's walk of that one-member group is (0, 0) exactly where the row is dead for the fold
    (own_seen + d >= W), and otherwise starts at the tile of the issue's lo and ends with the prefix -- lo itself to the position
    for the prefix lengths of one tile.  The brute-force reference used everywhere in this file is held to the same rule"""
    for n_pre in PREFIX_LENS[1:]:
        for own in OWN_SEEN:
            for window in WINDOWS:
                for d in range(DEPTHS):
                    got = _lib_walk(clib, [0, 1], [n_pre], [own + d], [1], window)[0]
                    assert got == SpeckvKVConnector.prefix_window_walk([0, 1], [n_pre], [own + d], [1], window)[0]
                    lo = max(0, n_pre + own + d - window)
                    if own + d >= window:
                        assert got == (0, 0) and lo >= n_pre
                    else:
                        assert got == (lo >> 5, (n_pre + 31) // 32 - (lo >> 5)) and got[1] >= 1
                    seen = _seen(n_pre, own, d, window)                   # the reference: the same rows dead, the same range
                    assert seen == (list(range(lo, n_pre)) if got[1] else [])
    # to the position: own_seen swept one by one over a 64-position prefix -- the first tile moves from 0 to 1 exactly where lo
    # passes 32, and the member stops counting exactly where lo reaches 64
    for window in (33, 40):
        for own in range(0, 45):
            lo = max(0, 64 + own - window)
            got = _lib_walk(clib, [0, 1], [64], [own], [1], window)[0]
            assert got == ((lo >> 5, 2 - (lo >> 5)) if lo < 64 else (0, 0)), (window, own)


def test_the_walk_export_refuses_what_the_header_names(clib):
    u32 = lambda *xs: (C.c_uint32 * len(xs))(*xs)
    out = u32(0, 0)
    walk = clib.speckv_ext_prefix_window_walk
    first, count = u32(9), u32(9)
    assert walk(1, u32(0, 1), u32(98), u32(37), u32(1), 40, first, count) == 0 and (first[0], count[0]) == (2, 2)
    assert walk(1, u32(0, 1), u32(98), None, u32(1), 40, first, count) == 0 and (first[0], count[0]) == (1, 3)   # own_seen NULL: zeros
    assert walk(0, None, None, None, None, 40, None, None) == 0
    assert walk(1, u32(0, 1), u32(35), u32(1), u32(1), 40, out, out) == -4                        # an odd prefix_len
    assert walk(1, u32(1, 2), u32(36, 36), u32(1, 1), u32(1, 1), 40, out, out) == -4              # not from 0
    assert walk(2, u32(0, 2, 1), u32(36, 36), u32(1, 1), u32(1, 1), 40, out, out) == -4           # not ascending
    assert walk(1, None, u32(36), u32(1), u32(1), 40, out, out) == -4
    assert walk(1, u32(0, 1), None, u32(1), u32(1), 40, out, out) == -4
    assert walk(1, u32(0, 1), u32(36), u32(1), None, 40, out, out) == -4
    assert walk(1, u32(0, 1), u32(36), u32(1), u32(1), 40, None, out) == -4
    for bad in (0, -1, True, 2.5, "4"):
        with pytest.raises(ValueError):
            SpeckvKVConnector.prefix_window_walk([0, 1], [36], [1], [1], bad)
    for args in (([0, 1], [36, 36], [1], [1]), ([0, 1], [35], [1], [1]), ([1, 2], [36, 36], [1, 1], [1, 1]), ([0, 2, 1], [36, 36], [1, 1], [1, 1]),
                 ([0, 1], [36], [1, 1], [1]), ([0, 1], [36], [1], [])):
        with pytest.raises(ValueError):
            SpeckvKVConnector.prefix_window_walk(*args, 40)


# ----------------------------------------------------------------------------- the float64 emulation
def _ceil(a, b):
    return -(-a // b)


def _emulate(lens, own_seen, n_q, depth, C_, rpp, window, q, K, V, own_out, own_lse, pieces=1, mutation=None):
    """k_attend_prefix<.., WINDOW> (+ the merge) for ONE group and ONE head in float64.  Member m sees [lo, lens[m]) of the prefix
    K / V; q [members][C][rpp][d]; own_out / own_lse what each row attended on its own; depth [members][C] or None (depth = index).
    The group's walk is prefix_window_walk's (the members that count, first_tile, max_len), a block walks [first_tile, n_pool), pieces
    cut the tiles that are LEFT (tpp = ceil(left / pieces)), staging zeros beyond max_len, a wave skips tiles none of its rows sees, a
    row is live iff lo < len, the merge takes M over the pieces (a piece that saw nothing holds -inf) in ascending order, the fold.
    Rows that are not live keep what out / lse held.  mutation: one rule broken."""
    per, members, d = 64 // rpp, len(lens), K.shape[1]
    lo_of = lambda m, dd: max(0, lens[m] + own_seen[m] + dd - window)
    counts = [m for m in range(members) if n_q[m] and lens[m] and lo_of(m, 0) < lens[m]]
    out, lse = own_out.copy(), own_lse.copy()
    if not counts:
        return out, lse
    max_len, first_tile = max(lens[m] for m in counts), min(lo_of(m, 0) for m in counts) >> 5
    assert [(first_tile, _ceil(max_len, 32) - first_tile)] == SpeckvKVConnector.prefix_window_walk([0, members], lens, own_seen, n_q, window)
    n_pool = _ceil(max_len, 32)
    if mutation == "first_tile one tile late":
        first_tile = min(first_tile + 1, n_pool - 1)
    left = n_pool - first_tile
    tpp = _ceil(left, max(1, min(pieces, left)))
    n_pieces = _ceil(left, tpp)
    for p_first in range(0, members * C_, per):
        rows = []                                                        # (row of the block, member, position, lo, len) of the live pairs
        for p in range(p_first, min(p_first + per, members * C_)):
            m, j = divmod(p, C_)
            if j >= n_q[m] or not lens[m]:
                continue
            dd = j if depth is None else depth[m][j]
            if mutation == "the bound of depth 0 for every row":
                dd = 0
            if mutation == "the row's index for its depth":
                dd = j
            lo = lo_of(m, dd) - (mutation == "lo one lower") + (mutation == "lo one higher")
            if lo < lens[m] or mutation == "a row that sees nothing folded anyway":
                rows.append((p - p_first, m, j, max(lo, 0), lens[m]))
        for jj, m, j, lo, limit in rows:
            wave_rows = [r for r in rows if (r[0] * rpp) // 16 == (jj * rpp) // 16]
            for r in range(rpp):
                parts = []
                for piece in range(n_pieces):
                    acc, m_run, l_run = np.zeros(d), -np.inf, 0.0
                    for tile in range(first_tile + piece * tpp, min(first_tile + (piece + 1) * tpp, n_pool)):
                        t = np.arange(32 * tile, 32 * tile + 32)
                        if not any(w[4] > t[0] and w[3] < t[0] + 32 for w in wave_rows):
                            continue
                        Kt, Vt = np.zeros((32, d)), np.zeros((32, d))
                        n = max(0, min(32, max_len - t[0]))
                        Kt[:n], Vt[:n] = K[t[0]:t[0] + n], V[t[0]:t[0] + n]
                        s = np.where((t >= lo) & (t < limit), Kt @ q[m, j, r], -np.inf)
                        m_new = max(m_run, s.max())
                        m_use = 0.0 if m_new == -np.inf else m_new
                        with np.errstate(invalid="ignore"):
                            alpha = np.exp(m_run - m_use)
                            p = np.exp(s - m_use)
                            l_run, m_run, acc = l_run * alpha + p.sum(), m_new, acc * alpha + p @ Vt
                    parts.append((acc, m_run, l_run))
                if mutation == "M over a piece that saw nothing taken as 0":
                    parts = [(acc, 0.0 if m_p == -np.inf else m_p, l_p) for acc, m_p, l_p in parts]
                M = max(p[1] for p in parts)
                num, den = np.zeros(d), 0.0
                with np.errstate(invalid="ignore", divide="ignore"):
                    for acc, m_p, l_p in parts:                           # ascending piece order
                        w = np.exp(m_p - M)
                        num, den = num + acc * w, den + l_p * w
                    own = own_lse[m, j, r]
                    lse_p = M + np.log(den)
                    mx = max(own, lse_p)
                    new = mx + np.log(np.exp(own - mx) + np.exp(lse_p - mx))
                    out[m, j, r] = own_out[m, j, r] * np.exp(own - new) + (num / den) * np.exp(lse_p - new)
                lse[m, j, r] = new
    return out, lse


def _case(lens, own_seen, n_q, depth, C_, rpp, window, seed=0, low=False):
    """a group: random prefix rows with V of +-1000, and per row the own keys it sees under the window -- min(W, own_seen + depth) of
    them; (q, K, V, own_out, own_lse, the plain float64 softmax over the last W positions of prefix + own, its lse, the same over
    |V|).  Rows that see nothing of the prefix want exactly what they attended on their own.  low: every prefix score is far below 0"""
    rng = np.random.default_rng(1000 * seed + sum(lens) + rpp + C_ + window)
    members, d, top = len(lens), 8, max(lens + [2])
    q = rng.standard_normal((members, C_, rpp, d))
    K, V = rng.standard_normal((top, d)), rng.standard_normal((top, d))
    if low:
        q, K = -400.0 * np.abs(q), np.abs(K)
    V *= 1000.0 * rng.choice([-1.0, 1.0], size=(top, 1))
    own_out, own_lse = np.zeros((members, C_, rpp, d)), np.full((members, C_, rpp), -np.inf)
    want, wlse, mag = np.zeros_like(own_out), np.full_like(own_lse, -np.inf), np.zeros_like(own_out)
    for m in range(members):
        for j in range(C_):
            dd = j if depth is None else depth[m][j]
            n_own = min(window, own_seen[m] + dd)
            Ko, Vo = rng.standard_normal((n_own, d)), rng.standard_normal((n_own, d))
            if low:
                Ko = -np.abs(Ko)                                          # own scores high: the prefix part weighs little but not nothing
            pre = _seen(lens[m], own_seen[m], dd, window)
            assert len(pre) + n_own == min(window, lens[m] + own_seen[m] + dd)
            for r in range(rpp):
                if n_own:
                    s = Ko @ q[m, j, r]
                    p = np.exp(s - s.max())
                    own_out[m, j, r], own_lse[m, j, r] = p @ Vo / p.sum(), s.max() + np.log(p.sum())
                want[m, j, r], wlse[m, j, r] = own_out[m, j, r], own_lse[m, j, r]
                if j < n_q[m] and pre:
                    Kc, Vc = np.concatenate([K[pre], Ko]), np.concatenate([V[pre], Vo])
                    s = Kc @ q[m, j, r]
                    p = np.exp(s - s.max())
                    want[m, j, r], wlse[m, j, r], mag[m, j, r] = p @ Vc / p.sum(), s.max() + np.log(p.sum()), p @ np.abs(Vc) / p.sum()
    return q, K, V, own_out, own_lse, want, wlse, mag


TREE = [0, 1, 2, 0, 1, 0]                                                 # deep nodes in front of roots: depth is not the index
# (prefix lengths, own_seen, n_q, depth table or None, C, rows_per_pos): decode steps with the issue's lengths mixed inside a block;
# chains and trees of 6 positions whose later rows lose the prefix; a member alone; a group that crosses a block; dead members
EMULATED = [([2, 36, 64, 98, 254], [0, 1, 2, 37, 64], [1] * 5, None, 1, 4), ([254, 98, 64, 36, 2], [64, 0, 37, 2, 1], [1] * 5, None, 1, 16),
            ([98, 254, 0, 36], [0, 2, 1, 37], [6, 3, 6, 6], None, 6, 4), ([98, 254, 36], [1, 37, 0], [6, 6, 4], [TREE] * 3, 6, 4),
            ([254], [2], [6], [TREE], 6, 1), ([2 + 2 * (m % 49) for m in range(17)], [m % 5 for m in range(17)], [1] * 17, None, 1, 4),
            ([480, 34, 98], [0, 1, 6], [1] * 3, None, 1, 4)]
EMULATED_W = [1, 2, 31, 32, 33, 40, 64, 100, 300]
PIECES = [1, 2, 3, 5, 16]


def test_the_emulated_walk_is_the_softmax_over_the_last_w_positions_of_prefix_and_own():
    folded = kept = 0
    for case in EMULATED:
        lens, own, n_q, depth, C_, rpp = case
        for window in EMULATED_W:
            q, K, V, own_out, own_lse, want, wlse, _ = _case(*case, window)
            for pieces in PIECES:
                got, lse = _emulate(lens, own, n_q, depth, C_, rpp, window, q, K, V, own_out, own_lse, pieces)
                assert np.all(np.isfinite(got)), (case, window, pieces)
                assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (case, window, pieces)
                with np.errstate(invalid="ignore"):
                    assert np.all((lse == wlse) | (np.abs(lse - wlse) < 1e-9)), (case, window, pieces)
                for m in range(len(lens)):                               # rows that are not live keep what they held, bit for bit
                    for j in range(C_):
                        dd = j if depth is None else depth[m][j]
                        if j >= n_q[m] or not _seen(lens[m], own[m], dd, window):
                            assert np.array_equal(got[m, j], own_out[m, j]) and np.array_equal(lse[m, j], own_lse[m, j])
                            kept += 1
                        else:
                            folded += 1
    assert folded > 1000 and kept > 1000


@pytest.mark.parametrize("mutation", ["lo one lower", "lo one higher", "the bound of depth 0 for every row", "the row's index for its depth",
                                      "a row that sees nothing folded anyway", "first_tile one tile late",
                                      "M over a piece that saw nothing taken as 0"])
def test_every_mutation_of_the_rule_leaves_the_float64_bound(mutation):
    """each broken rule moves some row of the emulated cases outside |err| <= 2e-3 sum p|v| + 1e-6 (or makes it NaN): the float64
    tests of tests/test_gpu_shared_prefix_window.py run these shapes on the device and would fail"""
    broken = 0
    for case in EMULATED:
        lens, own, n_q, depth, C_, rpp = case
        for window in EMULATED_W:
            q, K, V, own_out, own_lse, want, _, mag = _case(*case, window, low="piece" in mutation)
            for pieces in PIECES if "piece" in mutation else [1]:
                got, _ = _emulate(lens, own, n_q, depth, C_, rpp, window, q, K, V, own_out, own_lse, pieces, mutation=mutation)
                with np.errstate(invalid="ignore"):
                    broken += not np.all(np.abs(got - want) <= 2e-3 * mag + 1e-6)
    assert broken > 0, mutation


# ----------------------------------------------------------------------------- the connector's refusals
class _NoLib:
    """a library that must not be called: the connector refuses in front of it"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _T(*shape):
    """a host tensor of that shape: the refusals come before anything touches a device"""
    import torch
    return torch.zeros(shape, dtype=torch.float16)


class _Shape:
    """something that merely has a shape"""
    def __init__(self, *shape):
        self.shape = shape


def _connector(scheme="fp8", lengths=((1, 0), (2, 5), (50, 64), (51, 37))):
    conn = SpeckvKVConnector.__new__(SpeckvKVConnector)
    SpeckvKVConnector.__init__(conn, _NoLib(), num_layers=2, max_tokens=256, scheme=scheme)
    from cxl_speckv_amd.kv_connector import _Request
    for rid, n in lengths:
        conn.requests[rid] = _Request(1000 + rid)
        conn.requests[rid].length = n
    return conn


S = 3
METHODS = ["attend_shared", "attend_chunk_shared", "attend_tree_shared"]


def _invoke(conn, method, req_ids, prefix_ids, **kw):
    B = len(req_ids)
    if method == "attend_shared":
        return conn.attend_shared(0, req_ids, prefix_ids, _T(B, 8, 4, 128), 0.1, **kw)
    q, kv = _T(B, S, 8, 4, 128), _T(B, S, 2, 8, 128)
    if method == "attend_chunk_shared":
        return conn.attend_chunk_shared(0, req_ids, prefix_ids, q, kv, kv, 0.1, **kw)
    parents = kw.pop("parents", [-1, 0, 0])
    return conn.attend_tree_shared(0, req_ids, prefix_ids, q, kv, kv, 0.1, parents, **kw)


@pytest.mark.parametrize("method", METHODS)
def test_a_window_of_a_wrong_type_or_below_one_is_refused(method):
    conn = _connector()
    for bad in (0, -1, -40, True, False, 2.5, 40.0, "40", [40], 2 ** 32):
        with pytest.raises(ValueError, match="window"):
            _invoke(conn, method, [1, 2], [50, 50], window=bad)
        with pytest.raises(ValueError, match="window"):                   # also where no member sees a prefix
            _invoke(conn, method, [1, 2], [None, None], window=bad)


@pytest.mark.parametrize("method", METHODS)
def test_lists_of_the_wrong_length_are_refused_under_a_window(method):
    conn = _connector()
    with pytest.raises(ValueError):
        _invoke(conn, method, [1, 2], [50], window=40)
    with pytest.raises(ValueError):
        _invoke(conn, method, [1, 2], [50, 50, 50], window=40)
    with pytest.raises(ValueError):
        _invoke(conn, method, [1, 2], [50, 50], prefix_lens=[64], window=40)
    with pytest.raises(KeyError):
        _invoke(conn, method, [1, 2], [50, 99], window=40)
    with pytest.raises(ValueError, match="member of the call"):
        _invoke(conn, method, [1, 2], [50, 2], window=40)
    if method != "attend_shared":
        for bad in ([S], [S, S, S], [S, S + 1]):
            with pytest.raises(ValueError, match="n_new"):
                _invoke(conn, method, [1, 2], [50, 50], n_new=bad, window=40)


@pytest.mark.parametrize("window", [None, 40])
def test_rows_that_are_no_tensors_are_a_type_error_behind_the_judgement_of_the_lists(window):
    conn = _connector()
    q4, q5, kv = _T(2, 8, 4, 128), _T(2, S, 8, 4, 128), _T(2, S, 2, 8, 128)
    for bad in (None, _Shape(2, 8, 4, 128), [[0.0]]):
        with pytest.raises(TypeError, match="torch tensor"):
            conn.attend_shared(0, [1, 2], [50, 50], bad, 0.1, window=window)
        with pytest.raises(KeyError):                                     # the lists are judged first
            conn.attend_shared(0, [1, 2], [50, 99], bad, 0.1, window=window)
        for rows in ((bad, kv, kv), (q5, bad, kv), (q5, kv, bad)):
            with pytest.raises(TypeError, match="torch tensor"):
                conn.attend_chunk_shared(0, [1, 2], [50, 50], *rows, 0.1, window=window)
            with pytest.raises(TypeError, match="torch tensor"):
                conn.attend_tree_shared(0, [1, 2], [50, 50], *rows, 0.1, [-1, 0, 0], window=window)
    with pytest.raises(ValueError, match="q must be"):                    # a tensor of the wrong shape stays a ValueError
        conn.attend_shared(0, [1, 2], [50, 50], q5, 0.1, window=window)
    with pytest.raises(ValueError, match="q must be"):
        conn.attend_chunk_shared(0, [1, 2], [50, 50], q4, kv, kv, 0.1, window=window)


def test_parents_with_a_window_are_refused_by_attend_chunk_shared_as_attend_chunk_refuses_them():
    conn = _connector()
    with pytest.raises(ValueError, match="window does not combine with parents"):
        _invoke(conn, "attend_chunk_shared", [1, 2], [50, 50], window=40, parents=[-1, 0, 0])
    with pytest.raises(ValueError, match="window does not combine with parents"):
        _invoke(conn, "attend_chunk_shared", [1, 2], [None, None], window=40, parents=[-1, 0, 0])
    with pytest.raises(ValueError, match="window"):                       # the window is judged first
        _invoke(conn, "attend_chunk_shared", [1, 2], [50, 50], window=0, parents=[-1, 0, 0])


@pytest.mark.parametrize("window", [None, 40])
def test_malformed_trees_are_refused_in_front_of_any_library_call(window):
    conn = _connector()
    for method in ("attend_chunk_shared", "attend_tree_shared"):
        if method == "attend_chunk_shared" and window:
            continue
        for bad in ([-1, 0], [-1, 0, 0, 0], [-1, 1, 0], [-1, 0, 2], [0, 0, 0], [-1, True, 0], [[-1, 0, 0]], [[-1, 0, 0]] * 3, "tree"):
            with pytest.raises(ValueError, match="parents"):
                _invoke(conn, method, [1, 2], [50, 50], window=window, parents=bad)
    with pytest.raises(ValueError, match="parents"):
        conn.attend_tree_shared(0, [1, 2], [50, 50], _T(2, S, 8, 4, 128), _T(2, S, 2, 8, 128), _T(2, S, 2, 8, 128), 0.1, None, window=window)
