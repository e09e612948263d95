"""Not -m gpu: the launch shape of the block codec (speckv_ext_codec_launch_shape: the body launch_decompress / launch_compress size
every launch with, csrc/codec_launch_shape.hpp) against the loops of k_fetch_decompress and k_compress restated here.

Beyond the grid cap (CUs x wgs_per_cu workgroups of 4 waves) a wave owns per_wave blocks, one grid apart or -- rounds_consecutive --
next to each other.  Whether every block of [0, n) is then handled exactly once, and nothing at or beyond n, is decided by the rounding
of the rule together with the loop bounds of the two kernels: the loops are walked here, wave by wave, for every n up to a few rounds
at small caps and around the multiples of the cap at the shipped ones, also with n clipped on the device (CodecArgs::n_dev, the flush
fetch).  tests/test_gpu_codec_rounds.py asks this entry, before it trusts a run, whether its launch had several rounds at all."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = 4                                          # kWaves: waves of a codec workgroup
CUS = [1, 8, 256, 304]
WGS = [0, 1, 2, 3]                                 # tuning key wgs_per_cu; 0: the default, 256


def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_codec_launch_shape\s*\(\s*uint64_t n_blocks,\s*uint32_t n_cus,\s*uint32_t\* grid,\s*"
                     r"uint64_t\* per_wave,\s*uint64_t\* wave_step\)", header)
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header                   # an additive entry: the version stays
    doc = header[header.index("speckv_ext_codec_launch_shape:"):header.index("speckv_status_t speckv_ext_codec_launch_shape")]
    for word in ("wgs_per_cu", "rounds_consecutive", "exactly one wave", "Works without speckv_init", "256 without a device"):
        assert word in doc, word
    exports = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read()
    globals_ = re.search(r"global:(.*?)local:", exports, re.S).group(1)
    patterns = [p.strip() for p in globals_.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_codec_launch_shape", p) for p in patterns), patterns
    sig = speckv_ctypes._EXT_SIGNATURES["speckv_ext_codec_launch_shape"]
    assert sig[:2] == [C.c_uint64, C.c_uint32] and len(sig) == 5 and all(s is C.c_void_p for s in sig[2:])
    assert callable(speckv_ctypes.SpeckvLib.codec_launch_shape)
    # the launchers have no rule of their own left: one call of the shared body for decode, one for encode, and the export
    csrc = os.path.join(ROOT, "cxl-speckv_amd", "csrc")
    kernels = open(os.path.join(csrc, "kernels.hip")).read()
    assert len(re.findall(r"\bcodec_launch_shape_now\s*\(", kernels)) == 2          # its definition and shape_launch
    assert len(re.findall(r"\bshape_launch\s*\(", kernels)) == 3                     # its definition, launch_dec2, launch_compress
    assert len(re.findall(r"tuning\(\)\.(?:wgs_per_cu|rounds_consecutive)", kernels)) == 2                 # read there, once each
    assert "codec_launch_shape_now" in open(os.path.join(csrc, "c_api.cpp")).read()


@pytest.fixture(scope="module")
def clib():
    lib = C.CDLL(pkg.build_library())
    lib.speckv_ext_codec_launch_shape.restype = C.c_int
    lib.speckv_ext_codec_launch_shape.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.speckv_ext_set_tuning.restype = C.c_int
    lib.speckv_ext_set_tuning.argtypes = [C.c_char_p, C.c_longlong]
    lib.speckv_ext_abi_version.restype = C.c_uint32
    yield lib
    assert lib.speckv_ext_set_tuning(b"wgs_per_cu", 0) == 0 and lib.speckv_ext_set_tuning(b"rounds_consecutive", 0) == 0


def _shape(lib, n, cus):
    grid, per_wave, step = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    assert lib.speckv_ext_codec_launch_shape(n, cus, C.byref(grid), C.byref(per_wave), C.byref(step)) == 0
    return grid.value, per_wave.value, step.value


class _tuned:
    def __init__(self, lib, wgs, consecutive):
        self.lib, self.wgs, self.consecutive = lib, wgs, consecutive

    def __enter__(self):
        assert self.lib.speckv_ext_set_tuning(b"wgs_per_cu", self.wgs) == 0
        assert self.lib.speckv_ext_set_tuning(b"rounds_consecutive", self.consecutive) == 0

    def __exit__(self, *exc):
        assert self.lib.speckv_ext_set_tuning(b"wgs_per_cu", 0) == 0 and self.lib.speckv_ext_set_tuning(b"rounds_consecutive", 0) == 0


def _ceil(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- the kernels' loops, restated from their text
def _fetch_loop(grid, per_wave_arg, wave_step, n_launch, n_dev=None):
    """k_fetch_decompress (fetch_decompress_body): the block indices every wave of the launch decodes, in launch order"""
    out = []
    n = n_launch if n_dev is None else min(n_dev, n_launch)
    for block in range(grid):
        for wave in range(WAVES):
            per_wave = per_wave_arg if per_wave_arg else 1
            gw = block * WAVES + wave
            step = wave_step if wave_step else 1
            i = gw if wave_step else gw * per_wave
            end = n if wave_step else (i + per_wave if i + per_wave < n else n)
            if i >= n:
                continue
            while True:
                nx = i + step
                out.append(i)
                if nx >= end:
                    break
                i = nx
    return out


def _compress_loop(grid, per_wave_arg, wave_step, n):
    """k_compress: the block indices every wave of the launch encodes"""
    out = []
    for block in range(grid):
        for wave in range(WAVES):
            per_wave = per_wave_arg if per_wave_arg else 1
            gw = block * WAVES + wave
            step = wave_step if wave_step else 1
            i0 = gw if wave_step else gw * per_wave
            i1 = n if wave_step else (i0 + per_wave if i0 + per_wave < n else n)
            out.extend(range(i0, i1, step))
    return out


def _visit_counts(grid, per_wave, wave_step, n):
    """the same index sets for all waves at once (the launches too large to walk wave by wave; pinned to the two loops above on
    the small ones): how often every index is visited, over a range that reaches past n"""
    gw = np.arange(grid * WAVES, dtype=np.int64)
    if wave_step:
        k = np.arange(n // wave_step + 2, dtype=np.int64)
        idx = gw[:, None] + wave_step * k[None, :]
        idx = idx[idx < n]                                                   # (a wave's loop ends at the first index >= n)
    else:
        idx = gw[:, None] * per_wave + np.arange(per_wave, dtype=np.int64)[None, :]
        idx = idx[idx < n]                                                   # end = min(i + per_wave, n)
    return np.bincount(idx.reshape(-1), minlength=n + 1)


def _check_shape(n, cus, wgs, consecutive, shape, what):
    """the properties of a shape that do not need the loops"""
    grid, per_wave, wave_step = shape
    cap = cus * (wgs if wgs else 256)                                        # workgroups
    assert 1 <= grid <= cap, what
    assert (per_wave == 1) == (_ceil(n, WAVES) <= cap), what
    assert per_wave >= 1, what
    if per_wave == 1:
        assert wave_step == 0 and grid == max(1, _ceil(n, WAVES)), what
    else:
        assert wave_step == (0 if consecutive else grid * WAVES), what
        assert per_wave == _ceil(_ceil(n, WAVES), cap) and grid == _ceil(_ceil(n, WAVES), per_wave), what    # the rule as the header states it
        assert grid * WAVES * per_wave >= n > grid * WAVES * (per_wave - 1), what           # the waves cover n; the last round is not empty


@pytest.mark.parametrize("consecutive", [0, 1])
@pytest.mark.parametrize("wgs", [1, 2, 3])
@pytest.mark.parametrize("cus", [1, 8])
def test_small_caps_every_n_through_both_kernel_loops(clib, cus, wgs, consecutive):
    """every n from 1 to 3 x cap + 9 blocks: both kernels' loops, walked wave by wave, visit [0, n) once each and nothing else"""
    cap_blocks = cus * wgs * WAVES
    with _tuned(clib, wgs, consecutive):
        seen_rounds = set()
        for n in range(1, 3 * cap_blocks + 10):
            shape = _shape(clib, n, cus)
            what = (n, cus, wgs, consecutive, shape)
            _check_shape(n, cus, wgs, consecutive, shape, what)
            seen_rounds.add(shape[1])
            for visited in (_fetch_loop(*shape, n), _compress_loop(*shape, n)):
                assert sorted(visited) == list(range(n)), what
            assert np.array_equal(_visit_counts(*shape, n), np.r_[np.ones(n, np.int64), 0]), what        # pins the array form to the loops
        assert seen_rounds >= {1, 2, 3, 4}, seen_rounds


@pytest.mark.parametrize("consecutive", [0, 1])
@pytest.mark.parametrize("wgs", [1, 2, 3])
@pytest.mark.parametrize("cus", [1, 8])
def test_small_caps_every_device_side_count(clib, cus, wgs, consecutive):
    """the flush fetch: the grid is sized for n, the kernel clips to *n_dev <= n -- for EVERY pair the loop visits [0, n_dev) once each
    and nothing at or beyond n_dev (cus 1: walked wave by wave; cus 8: all waves at once)"""
    cap_blocks = cus * wgs * WAVES
    with _tuned(clib, wgs, consecutive):
        for n in range(1, 3 * cap_blocks + 10):
            shape = _shape(clib, n, cus)
            for n_dev in range(0, n + 1):
                if cus == 1:
                    assert sorted(_fetch_loop(*shape, n, n_dev)) == list(range(n_dev)), (n, n_dev, cus, wgs, consecutive, shape)
                counts = _visit_counts(*shape, n_dev)
                assert counts[:n_dev].all() and counts.sum() == n_dev, (n, n_dev, cus, wgs, consecutive, shape)
            assert sorted(_fetch_loop(*shape, n, n + 7)) == list(range(n)), (n, shape)                      # a count beyond n never widens it


def _chosen_sizes(cap_blocks):
    ns = {1, 2, 3, 4, 5, cap_blocks // 2, cap_blocks * 5 // 2 + 3, cap_blocks * 7 // 2 + 1}
    for k in (1, 2, 3, 4):
        for d in (-9, -5, -4, -3, -1, 0, 1, 3, 4, 5, 9):
            ns.add(k * cap_blocks + d)
        ns.add(k * cap_blocks + cap_blocks // 3)
    return sorted(x for x in ns if x >= 1)


@pytest.mark.parametrize("consecutive", [0, 1])
@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("cus", CUS)
def test_every_cap_at_sizes_around_its_multiples(clib, cus, wgs, consecutive):
    """CUs 1 .. 304 under wgs_per_cu 0 (256, the shipped cap) .. 3: n around every multiple of the cap up to 4 rounds, between them, and
    clipped on the device"""
    cap_blocks = cus * (wgs if wgs else 256) * WAVES
    with _tuned(clib, wgs, consecutive):
        for n in _chosen_sizes(cap_blocks):
            shape = _shape(clib, n, cus)
            what = (n, cus, wgs, consecutive, shape)
            _check_shape(n, cus, wgs, consecutive, shape, what)
            assert np.array_equal(_visit_counts(*shape, n), np.r_[np.ones(n, np.int64), 0]), what
            for n_dev in {0, 1, n // 3, max(0, n - cap_blocks), max(0, n - 5), n - 1}:
                counts = _visit_counts(*shape, n_dev)
                assert counts[:n_dev].all() and counts.sum() == n_dev, (what, n_dev)
            if n <= 4096:
                assert sorted(_fetch_loop(*shape, n)) == sorted(_compress_loop(*shape, n)) == list(range(n)), what


def test_the_entry_follows_the_tuning_in_force_and_needs_no_engine(clib):
    """set_tuning decides what the entry answers -- the GPU tests rely on exactly that -- and 0 restores the library's rule"""
    assert clib.speckv_ext_abi_version() == 6
    n = 4 * 304 + 1
    assert _shape(clib, n, 304) == (305, 1, 0)                               # the default cap: far away
    with _tuned(clib, 1, 0):
        assert _shape(clib, n, 304) == (153, 2, 612)
        assert _shape(clib, 5 * 4 * 304 + 3, 304) == (254, 6, 1016)
    with _tuned(clib, 1, 1):
        assert _shape(clib, n, 304) == (153, 2, 0)
    assert _shape(clib, n, 304) == (305, 1, 0)
    assert _shape(clib, 0, 8) == (1, 1, 0)
    assert _shape(clib, 4 * 256 * 256, 256) == (65536, 1, 0) and _shape(clib, 4 * 256 * 256 + 1, 256) == (32769, 2, 131076)
    assert _shape(clib, 655360, 256) == (54614, 3, 218456)                   # the 2.5-round launch of the rule's comment: three even rounds
    # n_cus 0: the device's compute units where there is one, 256 without
    mine = _shape(clib, 1 << 22, 0)
    assert mine in [_shape(clib, 1 << 22, c) for c in range(1, 1025)]
    try:
        have_device = os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK)
    except OSError:
        have_device = False
    if not have_device:
        assert mine == _shape(clib, 1 << 22, 256)
    out = C.c_uint64()
    for args in ((None, C.byref(out), C.byref(out)), (C.byref(out), None, C.byref(out)), (C.byref(out), C.byref(out), None)):
        assert clib.speckv_ext_codec_launch_shape(5, 8, *args) == -4         # SPECKV_ERR_INVAL


def test_the_binding_on_the_null_engine_answers_the_same(clib):
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        assert lib.codec_launch_shape(4 * 256 * 256 + 1, 256) == _shape(clib, 4 * 256 * 256 + 1, 256) == (32769, 2, 131076)
        lib.set_tuning("wgs_per_cu", 1)
        try:
            assert lib.codec_launch_shape(1025, 256) == (129, 2, 516)
        finally:
            lib.set_tuning("wgs_per_cu", 0)
    finally:
        lib.finalize()
