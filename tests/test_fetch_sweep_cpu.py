"""Not -m gpu: the sweep rule of fetch_range (speckv_ext_fetch_sweep_next: the body Engine::fetch_range decides every kernel-path launch
with, csrc/fetch_sweep.hpp) and the index arithmetic of a descending launch, restated here over speckv_ext_codec_launch_shape.

A fetch over the same range as the allocation's previous one walks the other way and keeps its stores in the Infinity Cache; anything
else is ascending with non-temporal stores.  A descending launch keeps the waves, rounds and strides of an ascending one: wave position
i decodes block n - 1 - i.  tests/test_gpu_fetch_sweep.py holds the two launches' outputs against each other on the GPU.

The refusal of `descending` / `keep_stores` together with the staged, ring and host-word forms (EXT 1-3) has no public entry that
reaches it: the engine sets the two fields on the kernel path of fetch_range only, and the raw codec entries take neither.  It is
pinned here in the launcher's text -- the check stands in front of every launch of launch_dec2 -- and not by a run."""
import ctypes as C
import fnmatch
import os
import re

import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cxl-speckv_amd", "csrc")
WAVES = 4
MAX_BLOCKS = 393216                                # kFetchSweepMaxBlocks


@pytest.fixture(scope="module")
def clib():
    lib = C.CDLL(pkg.build_library())
    lib.speckv_ext_fetch_sweep_next.restype = C.c_int
    lib.speckv_ext_fetch_sweep_next.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.speckv_ext_codec_launch_shape.restype = C.c_int
    lib.speckv_ext_codec_launch_shape.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.speckv_ext_set_tuning.restype = C.c_int
    lib.speckv_ext_set_tuning.argtypes = [C.c_char_p, C.c_longlong]
    yield lib
    for key in (b"wgs_per_cu", b"rounds_consecutive"):
        assert lib.speckv_ext_set_tuning(key, 0) == 0
    assert lib.speckv_ext_set_tuning(b"fetch_sweep", 1) == 0


NONE = (0, 0, 0, 0)


def nxt(lib, prev, first, n, capturing=0, mode=1):
    down, keep, state = C.c_uint32(0xDEAD), C.c_uint32(0xDEAD), (C.c_uint64 * 4)(7, 7, 7, 7)
    assert lib.speckv_ext_fetch_sweep_next(*prev, first, n, capturing, mode, C.byref(down), C.byref(keep), state) == 0
    return down.value, keep.value, tuple(state)


def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert re.search(r"speckv_status_t\s+speckv_ext_fetch_sweep_next\s*\(\s*uint64_t prev_first,\s*uint64_t prev_n,\s*uint32_t prev_descending,\s*"
                     r"uint32_t prev_valid,\s*uint64_t first,\s*uint64_t n,\s*int capturing,\s*int mode,\s*uint32_t\* out_descending,\s*"
                     r"uint32_t\* out_keep_stores,\s*uint64_t\* out_state\)", header)
    doc = header[header.index("speckv_ext_fetch_sweep_next:"):header.index("speckv_status_t speckv_ext_fetch_sweep_next")]
    for word in ("fetch_sweep", "Infinity Cache", "capturing", "Works without speckv_init", "speckv_ext_fetch_list", "393 216"):
        assert word in doc, word
    assert "fetch_sweep (" in header[header.index("Launch-form switches"):header.index("speckv_status_t speckv_ext_set_tuning")]
    exports = open(os.path.join(CSRC, "exports.map")).read()
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", exports, re.S).group(1).split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("speckv_ext_fetch_sweep_next", p) for p in patterns), patterns
    assert len(speckv_ctypes._EXT_SIGNATURES["speckv_ext_fetch_sweep_next"]) == 11
    assert callable(speckv_ctypes.SpeckvLib.fetch_sweep_next)
    # one rule: the engine and the export call the same body, and nobody else decides a direction
    engine_io = open(os.path.join(CSRC, "engine_io.cpp")).read()
    assert len(re.findall(r"\bfetch_sweep_next\s*\(", engine_io)) == 1
    assert len(re.findall(r"\.descending\s*=", engine_io)) == 1 and len(re.findall(r"\.keep_stores\s*=", engine_io)) == 1
    assert "fetch_sweep_next" in open(os.path.join(CSRC, "c_api.cpp")).read()
    for fn in os.listdir(CSRC):
        if fn.endswith((".cpp", ".hip")) and fn != "engine_io.cpp":
            text = open(os.path.join(CSRC, fn)).read()
            assert not re.search(r"\.(descending|keep_stores)\s*=[^=]", text), f"{fn} sets a sweep field of its own"


def test_the_rule(clib):
    # the first call is ascending with non-temporal stores and is remembered
    down, keep, st = nxt(clib, NONE, 0, 1000)
    assert (down, keep, st) == (0, 0, (0, 1000, 0, 1))
    # a repeat flips and keeps its stores, a third repeat flips back (and still keeps them: the fourth finds them)
    down, keep, st = nxt(clib, st, 0, 1000)
    assert (down, keep, st) == (1, 1, (0, 1000, 1, 1))
    down, keep, st = nxt(clib, st, 0, 1000)
    assert (down, keep, st) == (0, 1, (0, 1000, 0, 1))
    down, keep, st = nxt(clib, st, 0, 1000)
    assert (down, keep, st) == (1, 1, (0, 1000, 1, 1))
    # another first or another n: ascending again, and the new range is what the next call is compared with
    assert nxt(clib, st, 1, 1000) == (0, 0, (1, 1000, 0, 1))
    assert nxt(clib, st, 0, 999) == (0, 0, (0, 999, 0, 1))
    assert nxt(clib, (1, 1000, 0, 1), 0, 1000) == (0, 0, (0, 1000, 0, 1))
    # a state that is not valid (freed handle, first fetch) matches nothing, whatever it holds
    assert nxt(clib, (0, 1000, 0, 0), 0, 1000) == (0, 0, (0, 1000, 0, 1))
    # a capturing stream: ascending, non-temporal, the state left as it was -- in every mode
    for mode in (0, 1, 2, 3):
        for prev in (NONE, (0, 1000, 0, 1), (0, 1000, 1, 1), (5, 6, 1, 1)):
            assert nxt(clib, prev, 0, 1000, capturing=1, mode=mode) == (0, 0, prev)
    # tuning 0: ascending; tuning 2: descending with kept stores; both record the call
    for prev in (NONE, (0, 1000, 0, 1), (0, 1000, 1, 1)):
        assert nxt(clib, prev, 0, 1000, mode=0) == (0, 0, (0, 1000, 0, 1))
        assert nxt(clib, prev, 0, 1000, mode=2) == (1, 1, (0, 1000, 1, 1))
    # tuning 3: the directions of the rule, non-temporal stores
    assert nxt(clib, (0, 1000, 0, 1), 0, 1000, mode=3) == (1, 0, (0, 1000, 1, 1))
    assert nxt(clib, (0, 1000, 1, 1), 0, 1000, mode=3) == (0, 0, (0, 1000, 0, 1))
    assert nxt(clib, (0, 1000, 1, 1), 4, 1000, mode=3) == (0, 0, (4, 1000, 0, 1))
    # the rule's upper bound: beyond it a repeat stays as it was
    assert nxt(clib, (0, MAX_BLOCKS, 0, 1), 0, MAX_BLOCKS) == (1, 1, (0, MAX_BLOCKS, 1, 1))
    assert nxt(clib, (0, MAX_BLOCKS + 1, 0, 1), 0, MAX_BLOCKS + 1) == (0, 0, (0, MAX_BLOCKS + 1, 0, 1))
    assert nxt(clib, (0, MAX_BLOCKS + 1, 0, 1), 0, MAX_BLOCKS + 1, mode=2) == (1, 1, (0, MAX_BLOCKS + 1, 1, 1))
    # bad arguments
    down, state = C.c_uint32(), (C.c_uint64 * 4)()
    assert clib.speckv_ext_fetch_sweep_next(0, 0, 0, 0, 0, 1, 0, 1, None, C.byref(down), state) == -4
    assert clib.speckv_ext_fetch_sweep_next(0, 0, 0, 0, 0, 1, 0, 1, C.byref(down), None, state) == -4
    assert clib.speckv_ext_fetch_sweep_next(0, 0, 0, 0, 0, 1, 0, 1, C.byref(down), C.byref(down), None) == -4
    assert clib.speckv_ext_fetch_sweep_next(0, 0, 0, 0, 0, 1, 0, 4, C.byref(down), C.byref(down), state) == -4


def test_the_tuning_in_force_is_the_rule_by_default(clib):
    """mode < 0 asks for the tuning key: the shipped default alternates, and speckv_ext_set_tuning changes what the engine will do"""
    rep = (0, 1000, 0, 1)
    assert nxt(clib, rep, 0, 1000, mode=-1) == (1, 1, (0, 1000, 1, 1))
    try:
        assert clib.speckv_ext_set_tuning(b"fetch_sweep", 0) == 0
        assert nxt(clib, rep, 0, 1000, mode=-1) == (0, 0, (0, 1000, 0, 1))
        assert clib.speckv_ext_set_tuning(b"fetch_sweep", 2) == 0
        assert nxt(clib, NONE, 0, 1000, mode=-1) == (1, 1, (0, 1000, 1, 1))
    finally:
        assert clib.speckv_ext_set_tuning(b"fetch_sweep", 1) == 0
    wrapped = speckv_ctypes.SpeckvLib.fetch_sweep_next
    assert wrapped.__doc__ and "keep_stores" in wrapped.__doc__


# ----------------------------------------------------------------------------- the kernel's index arithmetic, restated from its text
def _shape(lib, n, cus):
    grid, per_wave, step = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    assert lib.speckv_ext_codec_launch_shape(n, cus, C.byref(grid), C.byref(per_wave), C.byref(step)) == 0
    return grid.value, per_wave.value, step.value


def _fetch_blocks(grid, per_wave_arg, wave_step, n, descending):
    """fetch_decompress_body: (wave, wave position i, block decoded) for every iteration of every wave of the launch"""
    out = []
    for block in range(grid):
        for wave in range(WAVES):
            per_wave = per_wave_arg if per_wave_arg else 1
            gw = block * WAVES + wave
            step = wave_step if wave_step else 1
            i = gw if wave_step else gw * per_wave
            end = n if wave_step else (i + per_wave if i + per_wave < n else n)
            if i >= n:
                continue
            cur = n - 1 - i if descending else i                     # load_desc of the current block
            while True:
                nx = i + step
                nxt_block = cur
                if nx < end:
                    nxt_block = n - 1 - nx if descending else nx     # ... and of the prefetched next one
                out.append((gw, i, cur))
                if nx >= end:
                    break
                cur = nxt_block
                i = nx
    return out


@pytest.mark.parametrize("consecutive", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 1025, 2500])
def test_a_descending_launch_decodes_every_block_once(clib, n, consecutive):
    want = -(-n // WAVES)                                             # workgroups of a one-round launch
    seen_rounds = set()
    try:
        assert clib.speckv_ext_set_tuning(b"wgs_per_cu", 1) == 0 and clib.speckv_ext_set_tuning(b"rounds_consecutive", consecutive) == 0
        for rounds in (1, 2, 3):
            if want < rounds:
                continue                                              # fewer workgroups than rounds: no cap gives this many
            cap = -(-want // rounds)                                  # n_cus x wgs_per_cu workgroups
            if -(-want // cap) != rounds:
                continue
            grid, per_wave, step = _shape(clib, n, cap)
            assert per_wave == rounds and grid <= cap and step == (0 if consecutive or rounds == 1 else grid * WAVES), (n, cap, grid, per_wave, step)
            seen_rounds.add(rounds)
            up = _fetch_blocks(grid, per_wave, step, n, False)
            down = _fetch_blocks(grid, per_wave, step, n, True)
            assert sorted(b for _, _, b in up) == list(range(n))
            assert sorted(b for _, _, b in down) == list(range(n)), "a block decoded twice, or never, or outside [0, n)"
            # the same waves at the same positions, the block mirrored
            assert [(w, i) for w, i, _ in up] == [(w, i) for w, i, _ in down]
            assert all(b == n - 1 - i for _, i, b in down) and all(b == i for _, i, b in up)
    finally:
        assert clib.speckv_ext_set_tuning(b"wgs_per_cu", 0) == 0 and clib.speckv_ext_set_tuning(b"rounds_consecutive", 0) == 0
    assert 1 in seen_rounds and (n < 5 or {2} <= seen_rounds) and (n < 1023 or {2, 3} <= seen_rounds), (n, seen_rounds)


def test_the_kernel_and_the_launcher_say_what_is_restated_here():
    text = open(os.path.join(CSRC, "kernels.hip")).read()
    body = text[text.index("void fetch_decompress_body"):text.index("__global__ __launch_bounds__(kThreads) void k_fetch_decompress")]
    assert "const bool down = EXT == 0 && a.descending;" in body
    assert "cur = load_desc<EXT>(a, down ? n - 1 - i : i, slot0);" in body
    assert "nxt = load_desc<EXT>(a, down ? n - 1 - nx : nx, slot0);" in body
    assert len(re.findall(r"load_desc<EXT>\(", body)) == 2                       # both call sites take the mirrored index
    assert "atomicOr(&a.flags[cur.page], a.set_flags)" in body                   # the residency update follows the block, not the position
    # the refusal: in front of every launch of launch_dec2
    launcher = text[text.index("hipError_t launch_dec2("):text.index("hipError_t launch_dec1(")]
    refusal = "if ((a.descending || a.keep_stores) && ext != 0) return hipErrorInvalidValue;"
    assert refusal in launcher and launcher.index(refusal) < launcher.index("hipLaunchKernelGGL")
    # k_compress has no direction
    comp = text[text.index("void k_compress(CodecArgs a)"):text.index("} // namespace", text.index("void k_compress(CodecArgs a)"))]
    assert "descending" not in comp and "keep_stores" not in comp
