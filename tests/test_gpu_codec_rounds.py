"""-m gpu: the block codec's MULTI-ROUND launch forms against the oracle, bit for bit.

Up to CUs x wgs_per_cu workgroups a wave of k_fetch_decompress / k_compress handles one block; beyond that it owns per_wave blocks, one
grid apart or (rounds_consecutive) next to each other -- the forms every pool of more than 1 GiB per launch runs.  With the shipped cap
that takes 262 145 blocks; with wgs_per_cu = 1 it takes R + 1 = 4 x CUs + 1, so every route is run here at n in {R + 1, 2R + 5, 3R - 1}
(the raw operators also at 5R + 3) under three settings: (wgs_per_cu 1, strided), (wgs_per_cu 1, consecutive) and the default cap as
the control.  Before a run is trusted, speckv_ext_codec_launch_shape -- the body the launchers size the launch with -- has to say
per_wave >= 2 for that n under the tuning in force (tests/test_codec_rounds_cpu.py pins that entry to the kernels' loops).

Every comparison is bit for bit against the oracle (NaN positions only have to match, as assert_same_float_bits has it), the control's
bits equal both small-cap runs' bits, destinations are pre-filled with NaN patterns and carry guard rows behind the last block."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from tests._gpu import N, assert_same_float_bits, dev_to_host, load_raw_lib, set_tuning, stored_record, stream_ptr, torch_mod
from tests.test_gpu_codec import make_blocks

pytestmark = pytest.mark.gpu
PAGE = 4096
GUARD = 5                                          # rows behind the last block that nothing may touch
SETTINGS = [("default cap", 0, 0), ("strided", 1, 0), ("consecutive", 1, 1)]            # the control first: the others are held against it
HINT = 0x100                                       # SPECKV_CODEC_HINT_STRUCTURED: the FLAT kernels
REC_ROOM = {0: 4096, 1: 2048, 2: 4096, 3: 1152, 4: 2048, 5: 1088}
MODES = {0: [0, 1], 1: [0, 1], 2: [0, 1], 3: [0], 4: [0], 5: [0]}


@pytest.fixture(scope="module")
def lib():
    return load_raw_lib()


@pytest.fixture(scope="module")
def cus(lib):
    """the device's compute units -- and the library's launchers count the same"""
    n = torch_mod().cuda.get_device_properties(0).multi_processor_count
    with tuned(1, 0):
        assert launch_shape(lib, 4 * n)[1] == 1 and launch_shape(lib, 4 * n + 1)[1] == 2, (n, launch_shape(lib, 4 * n + 1))
    return n


@contextlib.contextmanager
def tuned(wgs, consecutive):
    try:
        set_tuning("wgs_per_cu", wgs)
        set_tuning("rounds_consecutive", consecutive)
        yield
    finally:
        set_tuning("wgs_per_cu", 0)
        set_tuning("rounds_consecutive", 0)


def launch_shape(lib, n):
    grid, per_wave, step = C.c_uint32(), C.c_uint64(), C.c_uint64()
    raw = getattr(lib, "lib", lib)
    assert raw.speckv_ext_codec_launch_shape(int(n), 0, C.byref(grid), C.byref(per_wave), C.byref(step)) == 0
    return grid.value, per_wave.value, step.value


def prove_rounds(lib, n, wgs, consecutive):
    """the launch of n blocks under the tuning in force has the form this run is about -- asked of the entry the launchers call"""
    grid, per_wave, step = launch_shape(lib, n)
    if wgs == 0:
        assert (per_wave, step) == (1, 0), ("the control has to be a one-block-per-wave launch", n, grid, per_wave, step)
    else:
        assert per_wave >= 2 and step == (0 if consecutive else 4 * grid), (n, wgs, consecutive, grid, per_wave, step)
    return grid, per_wave, step


def same_bits(got, want, what):
    """assert_same_float_bits on the device (its numpy form words the failure)"""
    torch = torch_mod()
    it = torch.int16 if got.dtype == torch.float16 else torch.int32
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    if bool((torch.isnan(got) == nan).all()) and bool(((got.view(it) == want.view(it)) | nan).all()):
        return
    assert_same_float_bits(got.cpu().numpy(), want.cpu().numpy(), what)
    raise AssertionError(what)


def nan_filled(rows, f32=False):
    torch = torch_mod()
    return torch.full((rows, N), float("nan"), dtype=torch.float32 if f32 else torch.float16, device="cuda")


def untouched(buf, what):
    """the guard rows of a nan_filled buffer still hold the pattern they were filled with"""
    torch = torch_mod()
    it = torch.int16 if buf.dtype == torch.float16 else torch.int32
    ref = torch.full((1,), float("nan"), dtype=buf.dtype, device="cuda").view(it)
    assert bool((buf.view(it) == ref).all()), f"{what}: something was written behind the last block"


def exact(a, b, what):
    torch = torch_mod()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    assert torch.equal(a.view(it), b.view(it)), f"{what}: the small-cap launch and the control differ"


def period(lib, n, slots=None, cls=None):
    """a cycle length for the kinds of rows that is coprime to 4, to per_wave and to the grid of the small-cap launches, so that in both
    orders one wave's successive blocks (i and i + grid x 4, or i and i + 1) are of different kinds -- and, where the rows have classes
    (RLE decode), one under which every early return of the decoder meets a well-formed block on both sides in both orders"""
    with tuned(1, 0):
        grid, per_wave, step = launch_shape(lib, n)
    for p in (13, 17, 19, 23, 29, 31):
        if grid % p == 0 or per_wave % p == 0:
            continue
        if cls is None:
            return p
        rows = cls[row_index(slots, p, n)]
        if not _neighbours_missing(rows, n, (grid, per_wave, step), 0) and not _neighbours_missing(rows, n, (grid, per_wave, 0), 1):
            return p
    raise AssertionError((n, grid, per_wave))


def row_index(slots, p, n):
    """row i is entry (i // p) of slot i % p (slots beyond the listed ones repeat the well-formed first ones)"""
    i = np.arange(n)
    s = i % p
    out = np.empty(n, np.int64)
    for k in range(p):
        slot = np.asarray(slots[k] if k < len(slots) else slots[(k - len(slots)) * 2 % len(slots)])
        m = s == k
        out[m] = slot[(i[m] // p) % len(slot)]
    return out


# ----------------------------------------------------------------------------- a. raw decode
MALFORMED_SEED = 5


def _streams():
    """the malformed and ragged streams of test_decode_malformed_and_ragged"""
    rng = np.random.default_rng(MALFORMED_SEED)
    return [
        [5, 3, 7], [5, 0, 9, 2], [255, 200, 1, 255, 128, 1], [1], [], [3, 255] * 8 + [4, 8], [3, 255] * 9,
        list(rng.integers(0, 256, 4096)), [b for _ in range(2048) for b in (int(rng.integers(0, 256)), 1)], [7, 0] * 100 + [9, 5],
    ]


ZSTREAMS = [[0, 255] * 8 + [0, 8], [0, 100], [], [0, 255] * 12, [0, 0, 0, 7, 0, 0], [0, 1] * 2048, [0, 255] * 8 + [0, 8, 3]]


def _rle_class(rec, ln, scale):
    """which way decode_rle_fast leaves for an untrusted record (restated from its text): 'zero' the all-zero shortcut, 'go' a chunk
    whose running count passes 2048, 'ok' a stream that is short or has a zero count, 'well' the table path"""
    npairs = min(int(ln), 4096) >> 1
    seen = -(-npairs // 8) * 16                                  # lanes load whole 16-byte pieces
    bits = int(np.float32(scale).view(np.uint32))
    if not rec[:seen:2].any() and bits < 0x7F800000:
        return "zero"
    counts = rec[1:2 * npairs:2].astype(np.int64)
    if counts.sum() > N:
        return "go"
    if counts.sum() != N or (counts == 0).any():
        return "ok"
    return "well"


_DEC = {}


def decode_library(oracle, scheme, mode):
    """the distinct records of the decode tests with the oracle's fp16 and fp32 decode of each, computed once: `slots` lists, per kind of
    row, the entries that kind cycles through"""
    key = (scheme, mode)
    if key in _DEC:
        return _DEC[key]
    rng = np.random.default_rng(9000 + 10 * scheme + mode)
    recs, lens, scales, slots = [], [], [], []

    def add(entries):
        """entries: (record bytes, len, scale); returns their indices"""
        out = []
        for rec, ln, sc in entries:
            r = np.zeros(4096, np.uint8)
            rec = np.asarray(rec, np.uint8)[:4096]
            r[:rec.size] = rec
            recs.append(r); lens.append(ln); scales.append(sc)
            out.append(len(recs) - 1)
        return out

    def compressed(x):
        with np.errstate(over="ignore"):
            x16 = np.asarray(x).astype(np.float16).reshape(-1, N)
        s, l, r = oracle.compress_blocks_f16(x16, scheme, mode)
        return [(r[i], int(l[i]), float(s[i])) for i in range(len(l))]

    finite = make_blocks()[:14] if scheme in (3, 4) else make_blocks()          # (INT4_G32 / FP8 parity with the oracle is stated for finite data)
    blocks = compressed(finite)
    noise = compressed(rng.standard_normal((5, N)) * rng.uniform(0.1, 4.0, (5, 1)))
    runs = {run: compressed(np.repeat(rng.standard_normal((3, N // run)), run, axis=1)) for run in (8, 32, 2048)}
    zeros = compressed(np.zeros((1, N)))

    def cut(entries, cuts):
        return [(rec, c, sc) for (rec, ln, sc), c in zip(entries, cuts)]

    if scheme == 2:
        streams = [(s, len(s), 0.5) for s in _streams()]
        bad = [(s, len(s), sc) for s in ZSTREAMS for sc in (-0.5, -0.0, float("inf"), float("nan"))]     # the shortcut must NOT fire
        good = [(s, len(s), sc) for s in ZSTREAMS for sc in (0.5, 0.0, 3.0e38)]                           # ... and here it does
        overlong = [([3, 255] * 9, 18, 0.25), ([9, 255] * 8 + [2, 9], 18, 1.5)] + \
                   [(rng.integers(0, 256, 4096), 4096, 0.5) for _ in range(3)] + [(rng.integers(1, 256, 600), 600, 0.125)]
        short = cut(noise + blocks[:6], [4094, 4001, 2049, 16, 2, 1, 30, 7, 100, 33, 18])
        off_grid = compressed(np.stack([np.repeat(rng.standard_normal(N // 7 + 1), 7)[:N], np.repeat(rng.standard_normal(N // 32 + 1), 32)[5:5 + N]]))
        slots = [add(blocks), add(streams), add(noise), add(bad), add(runs[8]), add(good), add(blocks[5:] + zeros), add(runs[32]), add(overlong),
                 add(runs[2048] + compressed(np.full((1, N), 0.37))), add(short), add(noise[::-1]), add(off_grid)]
    else:
        room = REC_ROOM[scheme]
        if scheme == 0:
            ragged = [(rng.standard_normal(N).astype(np.float16).view(np.uint8), ln, 0.25) for ln in (0, 2, 3, 14, 16, 18, 4094, 4096)]
        elif scheme == 1:
            ragged = [(rng.integers(0, 256, 2048), ln, 0.25) for ln in (0, 1, 7, 8, 9, 2047, 2048)]
        elif scheme == 4:
            ragged = [(np.resize(np.arange(256, dtype=np.uint8), 2048), 2048, 0.5)] + cut(noise, [100, 0, 2047, 1, 2048])
        elif scheme == 3:
            ragged = cut(noise, [100, 0, 1151, 1152, 128])
        else:
            codes = [np.array([0, 1, 100, 101, 126, 127, 128, 140, 141, 150, 254, 255, 103, 110, 120, 130] * 4), np.arange(64) + 96,
                     np.arange(64) * 4, 255 - np.arange(64)]
            ragged = [(np.concatenate([(np.arange(1024) * 37 + 11).astype(np.uint8), c.astype(np.uint8)]), 1088, 1.0) for c in codes] + \
                     cut(noise, [1087, 0, 1088, 64, 1024])
        assert all(ln <= room for _, ln, _ in ragged)
        slots = [add(blocks), add(ragged), add(noise), add(zeros + runs[2048]), add(runs[8]), add(ragged[::-1]), add(blocks[5:]), add(runs[32]),
                 add(noise[::-1]), add(runs[2048]), add(ragged[1:] + ragged[:1]), add(blocks[::-1]), add(zeros)]
    recs = np.stack(recs); lens = np.asarray(lens, np.uint32); scales = np.asarray(scales, np.float32)
    want16 = np.zeros((len(lens), N), np.float16); want32 = np.zeros((len(lens), N), np.float32)
    for u in range(len(lens)):
        g16 = oracle.decompress_block_f16(recs[u, :lens[u]], scales[u], scheme, mode, N)
        g32 = oracle.decompress_block_f32(recs[u, :lens[u]], scales[u], scheme, mode, N)
        want16[u, :g16.size] = g16; want32[u, :g32.size] = g32
    torch = torch_mod()
    cls = np.array([_rle_class(recs[u], lens[u], scales[u]) for u in range(len(lens))]) if scheme == 2 else None
    d = dict(slots=slots, cls=cls, lens=lens,
             recs=torch.from_numpy(recs).cuda(), d_lens=torch.from_numpy(lens.view(np.int32)).cuda(), scales=torch.from_numpy(scales).cuda(),
             want16=torch.from_numpy(want16.view(np.int16)).cuda().view(torch.float16), want32=torch.from_numpy(want32).cuda())
    _DEC[key] = d
    return d


def _neighbours_missing(cls_rows, n, shape, consecutive):
    """the meetings this launch lacks: some wave has to decode, through the same LDS region, a well-formed block right after -- and right
    before -- a block that leaves decode_rle_fast by each of its three early returns"""
    grid, per_wave, step = shape
    a = np.arange(n)
    if consecutive:
        a = a[(a + 1 < n) & ((a + 1) % per_wave != 0)]
        b = a + 1
    else:
        a = a[a + step < n]
        b = a + step
    missing = []
    for early in ("zero", "go", "ok"):
        if not ((cls_rows[a] == "well") & (cls_rows[b] == early)).any():
            missing.append(("well", early))
        if not ((cls_rows[a] == early) & (cls_rows[b] == "well")).any():
            missing.append((early, "well"))
    return missing


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_raw_decode_in_every_launch_form(lib, oracle, cus, scheme):
    """speckv_ext_codec_decompress, untrusted records: rows cycle through the blocks of make_blocks(), the malformed and ragged streams,
    all-zero-value streams under the scales for which the shortcut must and must not fire, runs of 8 / 32 / 2048, noise and records
    whose len is cut short, with a period coprime to 4, per_wave and the grid -- both quantiser modes, fp16 and fp32 out, scheme 2 with
    and without the structured hint (the FLAT kernels)."""
    torch = torch_mod()
    R = 4 * cus
    for mode in MODES[scheme]:
        L = decode_library(oracle, scheme, mode)
        for n in (R + 1, 2 * R + 5, 3 * R - 1, 5 * R + 3):
            p = period(lib, n, L["slots"], L["cls"])
            idx_h = row_index(L["slots"], p, n)
            idx = torch.from_numpy(idx_h).cuda()
            d_recs, d_len, d_scale = L["recs"][idx].contiguous(), L["d_lens"][idx].contiguous(), L["scales"][idx].contiguous()
            for hint in ((0, HINT) if scheme == 2 else (0,)):
                for f32 in (False, True):
                    want = (L["want32"] if f32 else L["want16"])[idx]
                    control = None
                    for name, wgs, consecutive in SETTINGS:
                        what = f"scheme {scheme} mode {mode} n {n} hint {hint:#x} f32 {f32} {name}"
                        out = nan_filled(n + GUARD, f32)
                        with tuned(wgs, consecutive):
                            shape = prove_rounds(lib, n, wgs, consecutive)
                            if scheme == 2 and wgs:
                                assert not _neighbours_missing(L["cls"][idx_h], n, shape, consecutive), what
                            rc = lib.speckv_ext_codec_decompress(d_recs.data_ptr(), 4096, d_len.data_ptr(), d_scale.data_ptr(), n, out.data_ptr(),
                                                                 int(f32), scheme, mode | hint, stream_ptr())
                            assert rc == 0, (what, rc)
                            torch.cuda.synchronize()
                        same_bits(out[:n], want, what)
                        untouched(out[n:], what)
                        if control is None:
                            control = out
                        else:
                            exact(out, control, what)


# ----------------------------------------------------------------------------- b. raw encode
_ENC = {}


def encode_library(oracle, scheme, mode):
    key = (scheme, mode)
    if key in _ENC:
        return _ENC[key]
    torch = torch_mod()
    rng = np.random.default_rng(9500 + 10 * scheme + mode)
    base = make_blocks()
    noise = (rng.standard_normal((6, N)) * rng.uniform(0.05, 5.0, (6, 1))).astype(np.float16)
    around = []                                                      # long stretches around the 255 run limit, at several phases
    for seg, shift in ((230, 0), (247, 3), (254, 1), (255, 0), (255, 7), (256, 8), (257, 129), (270, 500), (510, 5), (765, 2)):
        around.append(np.repeat(rng.standard_normal((N + 600) // seg + 3), seg)[shift:shift + N])
    for start, length in ((0, 255), (300, 256), (511, 520), (1790, 257)):
        x = rng.standard_normal(N); x[start:start + length] = x[start]
        around.append(x)
    around = np.stack(around).astype(np.float16)
    zeros = np.stack([np.zeros(N), -np.zeros(N), np.concatenate([np.zeros(255), [1.0], np.zeros(N - 256)])]).astype(np.float16)
    nonfinite = base[14:]
    x = np.concatenate([base[:14], noise, around, zeros, nonfinite])
    o = np.cumsum([0, 14, len(noise), len(around), len(zeros), len(nonfinite)])
    rg = lambda k: list(range(o[k], o[k + 1]))
    slots = [rg(0), rg(1), rg(2), rg(3), rg(4), rg(1)[::-1], rg(2)[5:], rg(0)[7:], rg(3)[::-1], rg(2)[::-1], rg(1)[2:], rg(4)[::-1], rg(0)[3:]]
    scales, lens, recs = oracle.compress_blocks_f16(x, scheme, mode)
    oracle_rows = np.ones(len(x), bool)
    if scheme in (3, 4):
        oracle_rows[o[4]:] = False               # INT4_G32 / FP8 parity with the oracle is stated for finite data: those rows against the control only
    d = dict(slots=slots, x=torch.from_numpy(x.view(np.int16)).cuda(), lens=torch.from_numpy(lens.view(np.int32)).cuda(),
             scales=torch.from_numpy(scales).cuda(), recs=torch.from_numpy(recs).cuda(), oracle_rows=torch.from_numpy(oracle_rows).cuda())
    _ENC[key] = d
    return d


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_raw_encode_in_every_launch_form(lib, oracle, cus, scheme):
    """speckv_ext_codec_compress: rows cycle through make_blocks(), noise, long stretches around 255, zeros and inf / NaN blocks; record
    bytes, lengths and scale bits are the oracle's, the record rooms' tails and the rows behind the last block stay as they were."""
    torch = torch_mod()
    R = 4 * cus
    room = REC_ROOM[scheme]
    stride = room + 64                                               # 64 guard bytes behind every record room
    col = torch.arange(stride, device="cuda")[None, :]
    for mode in MODES[scheme]:
        L = encode_library(oracle, scheme, mode)
        for n in (R + 1, 2 * R + 5, 3 * R - 1, 5 * R + 3):
            idx = torch.from_numpy(row_index(L["slots"], period(lib, n), n)).cuda()
            d_x = L["x"][idx].contiguous()
            w_len, w_scale, w_recs, by_oracle = L["lens"][idx], L["scales"][idx], L["recs"][idx][:, :room], L["oracle_rows"][idx]
            control = None
            for name, wgs, consecutive in SETTINGS:
                what = f"scheme {scheme} mode {mode} n {n} {name}"
                d_recs = torch.full((n + GUARD, stride), 0xA5, dtype=torch.uint8, device="cuda")
                d_len = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
                d_scale = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
                with tuned(wgs, consecutive):
                    prove_rounds(lib, n, wgs, consecutive)
                    rc = lib.speckv_ext_codec_compress(d_x.data_ptr(), n, d_recs.data_ptr(), stride, d_len.data_ptr(), d_scale.data_ptr(), scheme, mode,
                                                       stream_ptr())
                    assert rc == 0, (what, rc)
                    torch.cuda.synchronize()
                assert torch.equal(d_len[:n][by_oracle], w_len[by_oracle]), (what, "record lengths")
                assert bool((d_len[:n] >= 0).all()) and bool((d_len[:n] <= room).all()), (what, "a block without a record")
                if scheme != 0:
                    nan = torch.isnan(w_scale)
                    assert bool((torch.isnan(d_scale[:n]) == nan)[by_oracle].all()), (what, "NaN scales")
                    assert bool(((d_scale[:n].view(torch.int32) == w_scale.view(torch.int32)) | nan | ~by_oracle).all()), (what, "scale bits")
                inside = col[:, :room] < d_len[:n, None]
                bad = (d_recs[:n, :room] != w_recs) & inside & by_oracle[:, None]
                assert not bool(bad.any()), (what, "record bytes", torch.nonzero(bad)[:4].tolist())
                # behind every record room and behind the last block: the fill
                assert bool((d_recs[:n, room:] == 0xA5).all()), (what, "bytes behind a record room")
                assert bool((d_recs[n:] == 0xA5).all()) and bool((d_len[n:] == -7).all()) and bool(torch.isnan(d_scale[n:]).all()), (what, "guard rows")
                got = (d_recs, d_len, d_scale)
                if control is None:
                    control = got
                else:
                    for a, b in zip(got, control):
                        exact(a, b, what)


# ----------------------------------------------------------------------------- c. pool routes
def open_engine(**env):
    """an engine with a remote pool (SPECKV_POOL_DEVICES="0,0", as test_engine_picks_the_flat_run_decoder_by_itself sets it)"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvLib
    env = dict({"SPECKV_POOL_DEVICES": "0,0"}, **{k: str(v) for k, v in env.items()})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return SpeckvLib(pkg.library_path(), "hip:0")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_POOL = {}


def pool_data(oracle, scheme, rows, flat=False):
    """`rows` pages whose kinds cycle with period 13 (noise, runs of 32 / 8 / 2048, zeros, the blocks of make_blocks(), stretches around
    255), their records and decode by the oracle -- computed once per pool format.  flat: data the RLE scheme compresses (runs and
    zeros with one noisy kind in 13), for which the engine picks the flat-run decoder by itself."""
    key = (scheme, flat)
    if key in _POOL:
        assert len(_POOL[key]["x"]) >= rows
        return _POOL[key]
    rng = np.random.default_rng(700 + scheme + 50 * flat)
    base = make_blocks()[:14]                                       # finite: what every pool format's parity with the oracle is stated for
    runs = lambda run: (lambda: np.repeat(rng.standard_normal(N // run), run))
    if flat:
        # (the engine samples the record length of every 1024th page: kinds 0, 10, 7, 4 for the first four; the noisy kind is none of them)
        kinds = [runs(32), runs(64), lambda: rng.standard_normal(N), runs(2048), lambda: np.zeros(N), runs(32), runs(128), runs(32),
                 runs(256), runs(64), runs(32), lambda: np.full(N, 0.37), runs(16)]
    else:
        kinds = [lambda: rng.standard_normal(N) * rng.uniform(0.1, 3.0), runs(32), lambda: np.zeros(N),
                 lambda: base[int(rng.integers(0, 14))], lambda: rng.standard_normal(N), runs(8), runs(2048), lambda: rng.standard_normal(N) * 1e-3,
                 lambda: np.repeat(rng.standard_normal(N // 255 + 2), 255)[int(rng.integers(0, 255)):][:N], runs(32),
                 lambda: base[int(rng.integers(0, 14))], lambda: rng.standard_normal(N) * 2.5, runs(64)]
    x = np.stack([np.asarray(kinds[i % 13](), np.float64) for i in range(rows)]).astype(np.float16)
    scales, lens, recs = oracle.compress_blocks_f16(x, scheme, 0)
    want = oracle.decompress_blocks_f16(recs, lens, scales, scheme, 0)
    torch = torch_mod()
    _POOL[key] = dict(scheme=scheme, x=x, scales=scales, lens=lens, recs=recs, want=want, d_x=torch.from_numpy(x.view(np.int16)).cuda(),
                      d_want=torch.from_numpy(want.view(np.int16)).cuda().view(torch.float16))
    return _POOL[key]


def check_records(eng, h, pages, D, rows, what):
    """the stored records of some pages against the oracle's: bytes, length and (RLE, FP8: the formats with a block scale) scale bits;
    pages[k] holds row rows[k] of the data"""
    for pg, r in zip(pages, rows):
        info = eng.translate(h, int(pg) * PAGE)
        ln = int(D["lens"][r])
        assert info.rec_bytes == ln, (what, pg, info.rec_bytes, ln)
        if D["scheme"] in (2, 4):
            assert np.float32(info.scale).tobytes() == D["scales"][r].tobytes(), (what, pg, "scale")
        assert stored_record(info, ln).tobytes() == D["recs"][r, :ln].tobytes(), (what, pg, "record bytes")


class Controls:
    """what the control launch left, per route: the small-cap launches have to leave the same bits"""

    def __init__(self):
        self.kept = {}

    def hold(self, key, setting, out, what):
        if setting == SETTINGS[0][0]:
            self.kept[key] = out
        else:
            exact(out, self.kept[key], what)


def fetch_all_ways(eng, h, n, D, stream, controls, setting, tag, what, engines=(1, 2)):
    """fetch_range through the fused kernel (1) and through the copy engines (2: staged records), fetch_list over a permutation with
    repeated pages: page p is the oracle's decode of data row p"""
    torch = torch_mod()
    want = D["d_want"][:n]
    for engine in engines:
        out = nan_filled(n + GUARD)
        eng.fetch_range(h, 0, n, out.data_ptr(), False, stream.cuda_stream, engine=engine)
        stream.synchronize()
        same_bits(out[:n], want, f"{what} fetch_range engine {engine}")
        untouched(out[n:], f"{what} fetch_range engine {engine}")
        controls.hold((tag, n, "range", engine), setting, out, f"{what} fetch_range engine {engine}")
    rng = np.random.default_rng(n)
    pages = np.concatenate([rng.permutation(n), rng.integers(0, n, 9)]).astype(np.int32)             # every page, nine of them twice
    rng.shuffle(pages)
    d_pages = torch.from_numpy(pages).cuda()
    out = nan_filled(len(pages) + GUARD)
    eng.fetch_list(h, d_pages.data_ptr(), len(pages), out.data_ptr(), False, stream.cuda_stream)
    stream.synchronize()
    same_bits(out[:len(pages)], want[d_pages.long()], f"{what} fetch_list")
    untouched(out[len(pages):], f"{what} fetch_list")
    controls.hold((tag, n, "list"), setting, out, f"{what} fetch_list")


def written(eng):
    st = eng.stats()
    return st.written_pages, st.compressed_bytes


@pytest.mark.parametrize("scheme,flat", [(2, False), (2, True), (4, False), (3, False), (5, False)], ids=["rle", "rle-flat", "fp8", "int4", "mxfp4"])
def test_pool_writes_and_fetches_in_every_launch_form(oracle, cus, scheme, flat):
    """One engine with a remote pool; per pool format (RLE -- also with data it compresses, which the engine reads with the FLAT kernels,
    plain and staged, by itself --, FP8, INT4_G32, MXFP4) and size: write from a device source and from a host source (whose staging
    chunks are launches of their own), fetch_range by both engines, fetch_list over a permutation with repeated pages, the same fetches
    after compaction (RLE: packed records, the structured hint by packed size) and after migrating a few runs (the page-table placement:
    the fused kernel and the list; the copy engines need runs) -- every page against the oracle's records and decode."""
    torch = torch_mod()
    R = 4 * cus
    D = pool_data(oracle, scheme, 3 * R - 1, flat)
    eng = open_engine()
    try:
        assert eng.stats().n_pool_devices == 2
        eng.set_compression_scheme(scheme)
        stream = torch.cuda.Stream()
        controls = Controls()
        for n in (R + 1, 2 * R + 5, 3 * R - 1):
            sample = np.unique(np.r_[0, 1, n - 1, np.arange(3, n, 97)])
            total_len = int(D["lens"][:n].astype(np.int64).sum())
            for setting, wgs, consecutive in SETTINGS:
                what = f"scheme {scheme} n {n} {setting}"
                with tuned(wgs, consecutive):
                    prove_rounds(eng, n, wgs, consecutive)
                    before = written(eng)
                    h = eng.alloc(n * PAGE)
                    eng.write(h, 0, D["d_x"].data_ptr(), n * PAGE, True)
                    torch.cuda.synchronize()
                    after = written(eng)
                    assert (after[0] - before[0], after[1] - before[1]) == (n, total_len), (what, "device write: pages, record lengths")
                    check_records(eng, h, sample, D, sample, what + " device write")
                    flat0 = eng.stats().flat_decoder_fetches
                    fetch_all_ways(eng, h, n, D, stream, controls, setting, "dev", what + " device write")
                    if scheme == 2:
                        assert eng.stats().flat_decoder_fetches - flat0 == (2 if flat else 0), (what, "which decoder the ranges took")
                        eng.compact(h)
                        check_records(eng, h, sample[:12], D, sample[:12], what + " compacted")
                        fetch_all_ways(eng, h, n, D, stream, controls, setting, "compacted", what + " compacted")
                    eng.free(h)
                    before = written(eng)
                    h = eng.alloc(n * PAGE)
                    eng.write(h, 0, D["x"].ctypes.data, n * PAGE, False)
                    torch.cuda.synchronize()
                    after = written(eng)
                    assert (after[0] - before[0], after[1] - before[1]) == (n, total_len), (what, "host write: pages, record lengths")
                    check_records(eng, h, sample[:12], D, sample[:12], what + " host write")
                    fetch_all_ways(eng, h, n, D, stream, controls, setting, "host", what + " host write", engines=(1,))
                    for first, count, pool in ((10, 50, 1), (n // 2, 301, 0), (n - 40, 40, 1)):
                        eng.migrate(h, first, count, pool)
                    check_records(eng, h, [10, 59, n // 2 + 300, n - 1], D, [10, 59, n // 2 + 300, n - 1], what + " migrated")
                    fetch_all_ways(eng, h, n, D, stream, controls, setting, "migrated", what + " migrated", engines=(1,))
                    eng.free(h)
    finally:
        eng.finalize()


@pytest.mark.parametrize("scheme", [2, 4, 3, 5])
def test_pool_strided_and_grouped_writes_in_every_launch_form(oracle, cus, scheme):
    """k_compress's page_step and its groups (block i belongs to group i / group_n): write_strided with a page step at the three sizes;
    write_strided_batch over many allocations and write_runs over many runs of one allocation with n_groups x group_n > R, for a group_n
    that divides grid x 4 and one that does not."""
    torch = torch_mod()
    R = 4 * cus
    D = pool_data(oracle, scheme, 3 * R - 1)
    eng = open_engine()
    try:
        eng.set_compression_scheme(scheme)
        stream = torch.cuda.Stream()
        controls = Controls()
        with tuned(1, 0):
            grid4 = 4 * launch_shape(eng, R + 16)[0]
        divides = 4
        not_divides = next(g for g in (7, 9, 5, 11) if grid4 % g)
        assert grid4 % divides == 0
        for setting, wgs, consecutive in SETTINGS:
            with tuned(wgs, consecutive):
                for n in (R + 1, 2 * R + 5, 3 * R - 1):
                    what = f"scheme {scheme} write_strided n {n} {setting}"
                    prove_rounds(eng, n, wgs, consecutive)
                    step = 3
                    before = written(eng)
                    h = eng.alloc((2 + step * n) * PAGE)
                    eng.write_strided(h, 2, step, n, D["d_x"].data_ptr(), stream.cuda_stream)
                    stream.synchronize()
                    assert written(eng)[0] - before[0] == n, (what, "pages that hold a record")
                    pages = (2 + step * np.arange(n)).astype(np.int32)
                    sample = np.unique(np.r_[0, n - 1, np.arange(5, n, 131)])
                    check_records(eng, h, pages[sample], D, sample, what)
                    d_pages = torch.from_numpy(pages).cuda()
                    out = nan_filled(n + GUARD)
                    eng.fetch_list(h, d_pages.data_ptr(), n, out.data_ptr(), False, stream.cuda_stream)
                    stream.synchronize()
                    same_bits(out[:n], D["d_want"][:n], what)
                    untouched(out[n:], what)
                    controls.hold(("strided", n), setting, out, what)
                    for pg in (0, 1, 3, 4, step * n + 1):                   # pages between the written ones hold no record
                        assert eng.translate(h, pg * PAGE).rec_bytes == 0, (what, pg)
                    eng.free(h)
                for group_n in (divides, not_divides):
                    n_groups = -(-(R + 1) // group_n)
                    total = n_groups * group_n
                    what = f"scheme {scheme} groups of {group_n} x {n_groups} {setting}"
                    prove_rounds(eng, total, wgs, consecutive)
                    step = 2
                    # write_strided_batch: one allocation per group, pages 1, 3, ... of it
                    before = written(eng)
                    hs = [eng.alloc((1 + step * group_n) * PAGE) for _ in range(n_groups)]
                    srcs = [D["d_x"].data_ptr() + g * group_n * PAGE for g in range(n_groups)]
                    eng.write_strided_batch(hs, [1] * n_groups, srcs, step, group_n, stream.cuda_stream)
                    stream.synchronize()
                    after = written(eng)
                    assert (after[0] - before[0], after[1] - before[1]) == (total, int(D["lens"][:total].astype(np.int64).sum())), what
                    out = nan_filled(total + GUARD)
                    d_pages = torch.from_numpy((1 + step * np.arange(group_n)).astype(np.int32)).cuda()
                    for g, h in enumerate(hs):
                        eng.fetch_list(h, d_pages.data_ptr(), group_n, out[g * group_n:].data_ptr(), False, stream.cuda_stream)
                    stream.synchronize()
                    same_bits(out[:total], D["d_want"][:total], what + " write_strided_batch")
                    untouched(out[total:], what)
                    controls.hold(("batch", group_n), setting, out, what)
                    for g in (0, 1, n_groups // 2, n_groups - 1):
                        check_records(eng, hs[g], [1, 1 + step * (group_n - 1)], D, [g * group_n, g * group_n + group_n - 1], what + " write_strided_batch")
                        assert eng.translate(hs[g], 0).rec_bytes == 0 and eng.translate(hs[g], 2 * PAGE).rec_bytes == 0, (what, g)
                    for h in hs:
                        eng.free(h)
                    # write_runs: runs of group_n pages of one allocation, a page apart
                    h = eng.alloc(n_groups * (group_n + 1) * PAGE)
                    firsts = [g * (group_n + 1) for g in range(n_groups)]
                    before = written(eng)
                    eng.write_runs(h, firsts, srcs, group_n, stream.cuda_stream)
                    stream.synchronize()
                    after = written(eng)
                    assert (after[0] - before[0], after[1] - before[1]) == (total, int(D["lens"][:total].astype(np.int64).sum())), what
                    pages = (np.asarray(firsts)[:, None] + np.arange(group_n)[None, :]).reshape(-1).astype(np.int32)
                    d_pages = torch.from_numpy(pages).cuda()
                    out = nan_filled(total + GUARD)
                    eng.fetch_list(h, d_pages.data_ptr(), total, out.data_ptr(), False, stream.cuda_stream)
                    stream.synchronize()
                    same_bits(out[:total], D["d_want"][:total], what + " write_runs")
                    untouched(out[total:], what)
                    controls.hold(("runs", group_n), setting, out, what)
                    sample = np.unique(np.r_[0, total - 1, np.arange(2, total, 211)])
                    check_records(eng, h, pages[sample], D, sample, what + " write_runs")
                    for g in (0, n_groups // 3, n_groups - 1):
                        assert eng.translate(h, (firsts[g] + group_n) * PAGE).rec_bytes == 0, (what, g)
                    eng.free(h)
    finally:
        eng.finalize()


# ----------------------------------------------------------------------------- d. flush fetch
RING_MB = 256                                      # SPECKV_L2_MB: 65 536 ring slots


@pytest.mark.parametrize("words", ["fetch", "scatter"])
def test_flush_fetch_clipped_on_the_device_in_every_launch_form(oracle, cus, words):
    """A prefetch_batch + prefetch_flush that takes more than 2R pages, built as test_flush_of_a_256_sequence_decode_step_at_full_size
    builds its own, smaller.  The fetch launch is sized for the flush's take limit -- min(ring / 2, 32 W words per request) -- and reads
    its block count on the device (n_dev), in the form that stores the pages' host-visible words itself (host_words) and in the one
    that leaves them to the scatter kernel.  Afterwards every page is issued, each slot holds the oracle's page, the slots follow the
    first-occurrence order and the slots in front of and behind the take are as they were."""
    R = 4 * cus
    Lyr, T, H, Dh = 8, 128, 8, 128
    n_pages = 2 * T * Lyr * H * Dh * 2 // PAGE
    region = T // 2
    pos0 = 16
    order = []                                                         # first occurrence inside a sequence: layer by layer, K then V, ascending positions
    for layer in range(Lyr):
        for kind in (0, 1):
            for p in range(pos0 + 1, pos0 + 5):
                pg = (layer * 2 + kind) * region + p // 2
                if pg not in order:
                    order.append(pg)
    per_seq = len(order)
    assert per_seq == 6 * Lyr
    n_seq = (2 * R + 7) // per_seq + 1
    take = n_seq * per_seq
    assert take > 2 * R
    Dt = pool_data(oracle, 2, 3 * R - 1)
    assert take <= len(Dt["x"])
    n_req = n_seq * Lyr
    n_l2 = RING_MB * 256
    window = take + GUARD + 64                                         # ring slots looked at before and after
    kept = None
    for setting, wgs, consecutive in SETTINGS:
        what = f"flush words by {words} {setting}"
        eng = open_engine(SPECKV_FLUSH_HOST_WORDS=words, SPECKV_L2_MB=RING_MB)
        try:
            with tuned(wgs, consecutive):
                # the launch is sized for min(ring / 2, 32 W n_req) blocks with W >= 1; the shape's per_wave does not fall with n
                for m in (min(n_l2 // 2, 32 * n_req), n_l2 // 2, take):
                    prove_rounds(eng, m, wgs, consecutive)
                eng.set_compression_scheme(2)
                hs = []
                for s_ in range(n_seq):
                    h = eng.alloc(n_pages * PAGE)
                    eng.set_layout(h, T, Lyr, H, Dh, 2)
                    eng.bind_request(s_, h, 0)
                    hs.append(h)
                    x = Dt["x"][s_ * per_seq:(s_ + 1) * per_seq]
                    for i, pg in enumerate(order):
                        eng.write(h, pg * PAGE, x[i].ctypes.data, PAGE, False)
                ring0 = eng.access(hs[0], 0, 8)                            # a page no request asks for: its slot tells where the ring stands
                before = dev_to_host(ring0, window * PAGE).reshape(window, PAGE).copy()
                reqs = np.repeat(np.arange(n_seq, dtype=np.uint32), Lyr)
                layers = np.tile(np.arange(Lyr, dtype=np.uint16), n_seq)
                cur = np.full(n_req, pos0, np.uint32)
                depth = np.full(n_req, 4, np.uint32)
                eng.prefetch_batch(reqs, layers, cur, depth)
                assert eng.prefetch_flush() == take, what
                eng.sync()
                base = None
                for s_ in range(n_seq):
                    infos = [eng.translate(hs[s_], pg * PAGE) for pg in order]
                    assert all(i.flags & 2 for i in infos), (what, s_)
                    addrs = [i.cache_addr for i in infos]
                    assert all(b - a == PAGE for a, b in zip(addrs, addrs[1:])), (what, s_)      # one run of ring slots per sequence
                    if base is None:
                        base = addrs[0]
                    assert addrs[0] == base + s_ * per_seq * PAGE, (what, s_)                        # ... the sequences in request order
                    others = [pg for pg in range(1, n_pages, 37) if pg not in order]
                    assert not any(eng.translate(hs[s_], pg * PAGE).flags & 3 for pg in others), (what, s_)
                k = (base - ring0) // PAGE
                assert (base - ring0) % PAGE == 0 and 1 <= k and k + take + GUARD <= window, (what, k)
                after = dev_to_host(ring0, window * PAGE).reshape(window, PAGE)
                rows = np.array([s_ * per_seq + i for s_ in range(n_seq) for i in range(per_seq)])
                assert_same_float_bits(after[k:k + take].view(np.float16), Dt["want"][rows], what)
                assert after[:k].tobytes() == before[:k].tobytes(), (what, "ring slots in front of the take were written")
                assert after[k + take:].tobytes() == before[k + take:].tobytes(), (what, "ring slots behind the count were written")
                if kept is None:
                    kept = after[k:k + take].copy()
                else:
                    assert after[k:k + take].tobytes() == kept.tobytes(), (what, "the small-cap launch and the control differ")
                assert eng.stats().prefetch_dropped == 0
                eng.prefetch_batch(reqs, layers, cur, depth)
                assert eng.prefetch_flush() == 0, what
        finally:
            eng.finalize()


# ----------------------------------------------------------------------------- e. ring fetch
@pytest.mark.parametrize("scheme", [2, 4])
def test_access_over_more_than_a_round_of_uncached_pages(oracle, cus, scheme):
    """speckv_access over a span of more than R uncached pages: the ring form of the fetch (one load_desc_ring per iteration, the ring's
    bookkeeping done by the waves) with several blocks per wave.  The span comes back contiguous with the oracle's pages, every page
    L2-resident at its slot, pages outside the span not.  Then the same through a page list (access_batch over as many pages in a
    shuffled order): one run of ring slots in list order."""
    R = 4 * cus
    D = pool_data(oracle, scheme, 3 * R - 1)
    kept = {}                                                       # the control's bytes, per fetch
    for setting, wgs, consecutive in SETTINGS:
        eng = open_engine(SPECKV_L2_MB=RING_MB)                     # 65 536 slots: the span fits many times
        try:
            with tuned(wgs, consecutive):
                eng.set_compression_scheme(scheme)
                for n in (R + 1, 2 * R + 5):
                    what = f"scheme {scheme} access over {n} pages {setting}"
                    prove_rounds(eng, n, wgs, consecutive)
                    h = eng.alloc((n + 9) * PAGE)
                    eng.write(h, 0, D["x"].ctypes.data, (n + 9) * PAGE, False)
                    ptr = eng.access(h, 4 * PAGE + 100, n * PAGE - 100 - 7)              # pages 4 .. n + 3
                    got = dev_to_host(ptr - 100, n * PAGE).view(np.float16).reshape(n, N)
                    assert_same_float_bits(got, D["want"][4:4 + n], what)
                    assert kept.setdefault((n, "span"), got.tobytes()) == got.tobytes(), (what, "the small-cap launch and the control differ")
                    for pg in range(n + 9):
                        info = eng.translate(h, pg * PAGE)
                        if 4 <= pg < 4 + n:
                            assert info.flags & 2 and info.cache_addr == ptr - 100 + (pg - 4) * PAGE, (what, pg, info.flags)
                        else:
                            assert not info.flags & 3, (what, pg, info.flags)
                    st = eng.stats()
                    assert st.dma_completed == st.dma_submitted
                    ptr2 = eng.access(h, 4 * PAGE + 100, n * PAGE - 100 - 7)             # all hits now: the same run, nothing fetched
                    assert ptr2 == ptr and eng.stats().dma_submitted == st.dma_submitted, what
                    eng.free(h)
                    # the same fetch by a page list: access_batch over n pages of a second allocation in a shuffled order
                    h = eng.alloc((n + 9) * PAGE)
                    eng.write(h, 0, D["x"].ctypes.data, (n + 9) * PAGE, False)
                    pages = 3 + np.random.default_rng(n).permutation(n)
                    ptrs = eng.access_batch(h, [int(pg) * PAGE + 64 for pg in pages])
                    assert all(p == ptrs[0] + i * PAGE for i, p in enumerate(ptrs)), (what, "one run of ring slots in list order")
                    got = dev_to_host(ptrs[0] - 64, n * PAGE).view(np.float16).reshape(n, N)
                    assert_same_float_bits(got, D["want"][pages], what + " by list")
                    assert kept.setdefault((n, "list"), got.tobytes()) == got.tobytes(), (what, "by list: the small-cap launch and the control differ")
                    for pg in range(n + 9):
                        info = eng.translate(h, pg * PAGE)
                        assert bool(info.flags & 2) == (3 <= pg < 3 + n) and not info.flags & 1, (what, "by list", pg, info.flags)
                    where = {int(pg): i for i, pg in enumerate(pages)}
                    for pg in (3, 4, n // 2, n + 2):
                        assert eng.translate(h, pg * PAGE).cache_addr == ptrs[0] - 64 + where[pg] * PAGE, (what, "by list", pg)
                    eng.free(h)
        finally:
            eng.finalize()
