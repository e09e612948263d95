"""Not -m gpu: the sliding-window decode attention (speckv_ext_decode_window_range, speckv_ext_attend_batch_window,
speckv_ext_attend_batch_plan_window, SpeckvKVConnector.decode_window_range / attend(window=...) / plan_step(window=...)).

The declarations; the walk rule of the library and the connector's restatement against a brute force written here that enumerates the
visible set position by position; the bound on the tiles walked; and a float64 emulation of the first-tile mask of the decode kernels
(the skip, the V-scale rule of a page cut by an odd bound, the shift to the window's first tile) over random K / V with hostile rows
below the window, which shows that each mutation of them leaves the bound of tests/_gpu.py HeadChecker on this data."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("speckv_ext_attend_plan_window_bytes", "speckv_ext_attend_batch_plan_window", "speckv_ext_attend_batch_window",
       "speckv_ext_decode_window_range")


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(pkg.build_library())
    speckv_ctypes.bind_ext(lib)
    return lib


def lib_range(lib, length, window):
    b, k, n = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    assert lib.speckv_ext_decode_window_range(length, window, C.byref(b), C.byref(k), C.byref(n)) == 0
    return b.value, k.value, n.value


def brute(length, window):
    """the visible POOL positions of a member of `length` positions under `window`, position by position: the query sits at length - 1
    and sees position p iff p <= length - 1 and length - 1 - p < window; the pool holds the first length & ~1 positions"""
    p = np.arange(length & ~1)
    return p[(p <= length - 1) & ((length - 1) - p < window)]


def test_the_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # additive entries: the version stays
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    for name in NEW[1:]:
        assert name in speckv_ctypes._EXT_SIGNATURES, name
    assert lib.speckv_ext_attend_plan_window_bytes(256) == 256 * (64 + 4 + 4)          # descriptors, dispatch order, skip array
    assert lib.speckv_ext_attend_plan_window_bytes(256) == lib.speckv_ext_attend_plan_bytes(256) + 256 * 4
    for name in ("attend_plan_window_bytes", "attend_batch_plan_window", "attend_batch_window", "decode_window_range"):
        assert callable(getattr(speckv_ctypes.SpeckvLib, name)), name
    assert lib.speckv_ext_decode_window_range(10, 4, None, None, None) == -4            # SPECKV_ERR_INVAL


def check_case(lib, length, window):
    begin, skip, n_pages = lib_range(lib, length, window)
    assert (begin, skip, n_pages) == SpeckvKVConnector.decode_window_range(length, window), (length, window)
    stored = length & ~1
    seen = brute(length, window)
    assert begin % 32 == 0 and 0 <= skip < 32, (length, window, begin, skip)
    if len(seen):
        # the visible pool positions are exactly [begin + skip, stored), and the launch walks the pages from begin to stored
        assert np.array_equal(seen, np.arange(begin + skip, stored)), (length, window, begin, skip)
        assert n_pages == (stored - begin) // 2 and begin + skip < stored
    else:
        assert n_pages == 0, (length, window, n_pages)
    # a member has no pool position exactly when W = 1 with an odd length, or the length is below 2
    assert (len(seen) == 0) == ((window == 1 and length % 2 == 1) or length < 2), (length, window)
    # the tiles walked: never more than ceil((W + 31) / 32), nor than the context's
    tiles = (n_pages + 15) // 16
    assert tiles <= (window + 31 + 31) // 32 and tiles <= (stored + 31) // 32, (length, window, tiles)
    # the tail (an odd length's last position) and a step's own stored position are always visible
    if length and length % 2 == 0:
        assert len(seen) and seen[-1] == length - 1
    return tiles


def test_the_rule_against_a_brute_force(lib):
    worst = {}
    for length in range(0, 401):
        for window in range(1, 201):
            tiles = check_case(lib, length, window)
            worst[window] = max(worst.get(window, 0), tiles)
    # the bound is reached, not merely respected: ceil((W + 31) / 32) tiles at some length -- except where W = 2 (mod 32): lo has the parity of W
    # there (an even length) or sees W - 1 stored positions (an odd one), so the walk spans W + 30 positions at most, one tile less
    for window, tiles in worst.items():
        assert tiles == (window + 62) // 32 - (1 if window % 32 == 2 else 0), (window, tiles)


@pytest.mark.parametrize("window", [1024, 4096])
def test_the_rule_at_long_contexts(lib, window):
    worst = 0
    for length in list(range(0, 40001, 7)) + list(range(window - 70, window + 70)) + list(range(39900, 40001)):
        worst = max(worst, check_case(lib, length, window))
    assert worst == (window + 62) // 32
    print(f"window {window}: at most {worst} tiles walked at lengths up to 40000 (the context's: {40000 // 32})")


def test_no_window_and_the_connector_refusals(lib):
    for length in (0, 1, 2, 33, 64, 65, 4097):
        assert lib_range(lib, length, 0) == (0, 0, (length & ~1) // 2) == SpeckvKVConnector.decode_window_range(length, None)
        assert SpeckvKVConnector.decode_window_range(length, 0) == (0, 0, (length & ~1) // 2)
    for bad in (-1, 1.5, 2 ** 32):
        with pytest.raises(ValueError):
            SpeckvKVConnector.decode_window_range(10, bad)


# ----------------------------------------------------------------------------- the first-tile mask, emulated in float64
D = 16
K_HOSTILE, V_HOSTILE = 200.0, 1000.0
MUTATIONS = ("none", "skip + 1", "skip - 1", "skip rounded down to a page", "skip rounded up to a page", "half-masked page's V scale zeroed",
             "half-masked page's V scale elected as the tile's reference", "shift one tile late")


def content(T, lo, needle, seed):
    """K / V rows [T][D]: ordinary rows from lo on, hostile rows (K x 200, V = +-1000: tests/test_gpu_hostile_ranges.py) below lo;
    needle = True: position lo takes nearly all the weight; needle = "quiet": the kept rows have equal weights and V of 1 / 5000 the
    magnitude -- what a reference scale set by the hostile row would round away"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(D) * 1.5
    k = rng.standard_normal((T, D)) * rng.uniform(0.2, 3.0, (T, 1))
    v = rng.standard_normal((T, D)) * rng.uniform(0.2, 3.0, (T, 1))
    k[:lo] *= K_HOSTILE
    v[:lo] = np.sign(v[:lo]) * V_HOSTILE
    if needle == "quiet":
        k[lo:] = 0.0
        v[lo:] *= 0.0002
    elif needle and lo < T:
        k[lo] = q * 6.0
    return q, k, v


def reference(q, k, v, lo, stored, sm):
    """float64 attention over the positions [lo, stored): out, sum p|v|"""
    s = (k[lo:stored] @ q) * sm
    p = np.exp(s - s.max())
    return (p @ v[lo:stored]) / p.sum(), (p @ np.abs(v[lo:stored])) / p.sum()


def emulate(q, k, v, length, window, sm, mutation):
    """The walk of a decode kernel over one member: tiles of 32 positions from `begin`, the first `skip` positions of tile 0 and the
    positions behind `stored` scored -inf, the weights of a tile rounded to fp16 in units of the tile's reference V scale (the FP8
    kernels: a page's two positions share one scale): the largest scale among the pages that are not wholly masked, a page CUT by an
    odd bound counted with 2^-10 of its scale -- its masked row may have set it -- while its kept position keeps the whole scale."""
    begin, skip, n_pages = SpeckvKVConnector.decode_window_range(length, window)
    stored = length & ~1
    zero_half, elect_half = False, False
    if mutation == "skip + 1": skip += 1
    elif mutation == "skip - 1": skip -= 1
    elif mutation == "skip rounded down to a page": skip &= ~1
    elif mutation == "skip rounded up to a page": skip = (skip + 1) & ~1
    elif mutation == "half-masked page's V scale zeroed": zero_half = True
    elif mutation == "half-masked page's V scale elected as the tile's reference": elect_half = True
    elif mutation == "shift one tile late": begin += 32; skip = max(0, skip - 32)
    T = len(k)
    m, l, acc = -np.inf, 0.0, np.zeros(D)
    for t0 in range(begin, stored, 32):
        pos = np.arange(t0, t0 + 32)
        live = (pos < stored) & (pos < T) & ((pos >= begin + skip) if t0 == begin else True)
        kk = np.where((pos < T)[:, None], k[np.minimum(pos, T - 1)], 0.0)
        vv = np.where((pos < T)[:, None], v[np.minimum(pos, T - 1)], 0.0)
        s = np.where(live, (kk @ q) * sm, -np.inf)
        vs = np.abs(vv).reshape(16, 2 * D).max(axis=1) / 448.0                   # one scale per page of two positions
        page_live = live.reshape(16, 2)
        vs = np.where(page_live.any(axis=1) if not zero_half else page_live.all(axis=1), vs, 0.0)
        cand = np.where(page_live.all(axis=1) | elect_half, vs, vs / 1024.0)
        vref = cand.max() if cand.max() > 0 else 1.0
        m_new = max(m, s.max())
        if m_new == -np.inf:
            continue
        f = np.exp(m - m_new) if m > -np.inf else 0.0
        p = np.exp(s - m_new)
        w16 = (p * np.repeat(vs, 2) / vref).astype(np.float16).astype(np.float64)          # the weight in units of the page's scale
        codes = np.where(np.repeat(vs, 2)[:, None] > 0, vv / np.where(np.repeat(vs, 2) > 0, np.repeat(vs, 2), 1.0)[:, None], 0.0)
        acc = acc * f + vref * (w16 @ codes)
        l = l * f + p.sum()
        m = m_new
    return acc / l if l > 0 else np.zeros(D)


CASES = [(length, window) for length in (33, 64, 65, 98, 131, 255, 256) for window in (2, 31, 32, 33, 64, 100)]


def test_mutations_of_the_first_tile_mask_leave_the_bound():
    """Every mutation misses |err| <= 2e-3 sum p|v| + 1e-6 (HeadChecker's bound; float64 here: delta = 0) on at least one case of the
    data, the rule as it stands holds it on every case; a mutation that changes no result on a case is reported as such."""
    sm = 1.0 / np.sqrt(D)
    caught = {mu: 0 for mu in MUTATIONS}
    unchanged = {mu: [] for mu in MUTATIONS}
    for needle in (False, True, "quiet"):
        for length, window in CASES:
            lo = max(0, length - window)
            stored = length & ~1
            q, k, v = content(256, lo, needle, 7000 + 13 * length + window)
            want, mag = reference(q, k, v, lo, stored, sm)
            base = emulate(q, k, v, length, window, sm, "none")
            for mu in MUTATIONS:
                got = base if mu == "none" else emulate(q, k, v, length, window, sm, mu)
                ok = bool(np.all(np.abs(got - want) <= 2e-3 * mag + 1e-6))
                if mu == "none":
                    assert ok, ("the rule as it stands", length, window, needle, float(np.abs(got - want).max()))
                elif np.array_equal(got, base):
                    unchanged[mu].append((length, window, needle))
                elif not ok:
                    caught[mu] += 1
    for mu in MUTATIONS[1:]:
        print(f"mutation '{mu}': leaves the bound on {caught[mu]} of {3 * len(CASES)} cases, changes no result on {len(unchanged[mu])}: "
              f"{unchanged[mu][:8]}{' ...' if len(unchanged[mu]) > 8 else ''}")
    for mu in MUTATIONS[1:]:
        assert caught[mu] > 0, (mu, "no case of the data tells it from the rule")
