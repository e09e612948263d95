"""-m gpu: the STREAM form of speckv_ext_attend_int4 (k_attend_int4_wg8 with AttendArgs::stream: the layers x tiles of a call cut, layer-major,
into one contiguous piece per workgroup; attend_int4.hip) against float64, at 128 and 512 positions.

By itself the engine takes the form from 28k context only (attend_geometry.hpp int4_wg8_stream); the tuning key attend_stream = N cuts a call
of any size into exactly N pieces, so 5 layers x 4 or 16 tiles reach every shape of the partition: one workgroup for the whole call, pieces
over three layers, pieces of one tile, piece boundaries on and off layer boundaries, a remainder (the first rem pieces one longer), layers of
1 .. 16 partials (both merge kernels), every count of query rows, ranges off 0, a first layer off 0, a ragged last tile in every layer, and
the residue-class form of the kernel over pools striped 3 and 7 ways.

Every case (1) asserts on the host, through the decision the engine itself takes (tests/_rules.py int4_stream over tests/csrc/host_rules_test.cpp),
that the call streams with the (n_wgs, len, rem, max_slots) it names -- a failing branch assertion means the case no longer tests what it
names; (2) pre-fills out and lse with NaN; (3) checks EVERY (layer, head, query row) of out and lse against the float64 attention over the
dequantised records (tests/_gpu.py HeadChecker.check_rows: |err| <= 2e-3 sum p|v| + 1e-6, lse within 2e-3; INT4_G32 multiplies the fp16
query as it is, delta = 0).

Data: N(0, 1) x a per-page magnitude in [0.2, 3); pages of zeros (zero group scales) and pages with a wide spread inside their groups, in K
and in V; queries 1.5 x N(0, 1) in fp16.  Seeds are fixed."""
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from tests._gpu import D, H, HeadChecker, set_tuning, torch_mod
from tests._rules import int4_stream, load_rules, striped_tiles

pytestmark = pytest.mark.gpu
PAGE = 4096
L = 5
SM = 1.0 / np.sqrt(D)
INT4 = 3


@pytest.fixture(scope="module")
def rules():
    return load_rules()


def cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


def partition(n_layers, n_tiles, n_wgs):
    """(len, rem, max_slots, layers the longest-reaching piece meets) of n_layers x n_tiles tiles in n_wgs pieces, by brute force"""
    total = n_layers * n_tiles
    ln, rem = divmod(total, n_wgs)
    owner = np.repeat(np.arange(n_wgs), [ln + (w < rem) for w in range(n_wgs)])
    per_layer = [len(np.unique(owner[l * n_tiles:(l + 1) * n_tiles])) for l in range(n_layers)]
    span = max(len(np.unique(np.nonzero(owner == w)[0] // n_tiles)) for w in range(n_wgs))
    return ln, rem, max(per_layer), span


# ----------------------------------------------------------------------------- one engine at a time, its allocations and checkers built once
class Setup:
    """An engine over `pools` pools on this GPU with one INT4_G32 allocation of L layers per T, the float64 checker of every layer, and
    queries for every count of rows the cases use.  Nothing here changes after it is built."""

    def __init__(self, oracle, pools, Ts):
        torch = torch_mod()
        if pools > 1:
            os.environ["SPECKV_POOL_DEVICES"] = ",".join(["0"] * pools)
        try:
            self.kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), "hip:0")
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        self.lib = self.kv.lib
        self.lib.set_compression_scheme(INT4)
        self.handle, self.checkers = {}, {}
        for T in Ts:
            rng = np.random.default_rng(9100 + T + pools)
            n_pages = T * L                                          # a layer: T / 2 pages of K, then T / 2 of V
            x = (rng.standard_normal((n_pages, 2048)) * rng.uniform(0.2, 3.0, (n_pages, 1))).astype(np.float16)
            x[5] = 0.0                                               # layer 0, K: a page of zeros
            x[3 * T + T // 2 + 40] = 0.0                             # layer 3, V
            x[1 * T + 41, ::3] *= np.float16(40.0)                   # layer 1, K: a wide spread inside the groups
            x[2 * T + T // 2 + 9, ::3] *= np.float16(40.0)           # layer 2, V
            h = self.lib.alloc(n_pages * PAGE)
            self.lib.set_layout(h, T, L, H, D, 2)
            self.lib.write(h, 0, x.ctypes.data, x.nbytes, False)
            self.handle[T] = h
            self.checkers[T] = [HeadChecker(oracle, INT4, x[l * T:(l + 1) * T], T) for l in range(L)]
        qrng = np.random.default_rng(9200 + pools)
        self.qh = {g: (qrng.standard_normal((L, H, g, D)) * 1.5).astype(np.float16) for g in (1, 3, 8, 16)}
        self.q = {g: torch.from_numpy(q).cuda() for g, q in self.qh.items()}
        torch.cuda.synchronize()

    def close(self):
        for h in self.handle.values():
            self.lib.free(h)
        self.kv.close()


_state = {"pools": None, "setup": None}


def drop_setup():
    if _state["setup"] is not None:
        _state["setup"].close()
    _state.update(pools=None, setup=None)


def setup_for(oracle, pools):
    if _state["pools"] != pools:
        drop_setup()
        _state["setup"] = Setup(oracle, pools, (128, 512) if pools == 1 else (512,))
        _state["pools"] = pools
    return _state["setup"]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_setup()


def attend(su, T, g, layer, n_layers, pb, pe, knob, want_lse=True):
    """the call with attend_stream = knob; out [n_layers][H][g][D], lse [n_layers][H][g] (None without), both NaN before the call"""
    torch = torch_mod()
    out = torch.full((n_layers, H, g, D), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((n_layers, H, g), float("nan"), dtype=torch.float32, device="cuda") if want_lse else None
    set_tuning("attend_stream", knob)
    try:
        su.lib.attend_int4(su.handle[T], layer, n_layers, su.q[g][layer].data_ptr(), g, pb, pe, SM, out.data_ptr(), lse.data_ptr() if want_lse else None)
        torch.cuda.synchronize()
    finally:
        set_tuning("attend_stream", 0)
    return out.cpu().numpy(), lse.cpu().numpy() if want_lse else None


def check_float64(su, T, g, layer, n_layers, pb, pe, out, lse, what):
    for i in range(n_layers):
        hc = su.checkers[T][layer + i]
        for head in range(H):
            hc.check_rows(out[i, head][None], None if lse is None else lse[i, head][None], su.qh[g][layer + i, head][None], head, [pe - pb], SM,
                          (what, "layer", layer + i, "head", head), pos_begin=pb)


def stream_case(rules, su, T, pieces, g=8, layer=0, n_layers=L, pb=0, pe=None, pools=1, want_lse=True, expect=None):
    """One stream call: the host assertion of its form, then the float64 check of every row.  expect = (len, rem, max_slots) the case names."""
    pe = T if pe is None else pe
    n_pages = (pe - pb) // 2
    cls = pools > 1
    n_tiles = int(striped_tiles(n_pages, pools)) if cls else (n_pages + 15) // 16
    assert pb + (n_pages + 15) // 16 * 32 <= T                        # every tile inside the layer's region: arithmetic addresses, not the page table
    ln, rem, max_slots, _ = partition(n_layers, n_tiles, pieces)
    d = int4_stream(rules, n_layers, n_tiles, cus(), cls=cls, attend_stream=pieces)
    assert d == dict(n_wgs=pieces, len=ln, rem=rem, max_slots=max_slots, tiles=n_tiles if cls else 0), (d, pieces, ln, rem, max_slots)
    if expect is not None:
        assert (ln, rem, max_slots) == expect
    what = ("stream", "T", T, "pieces", pieces, "g", g, "layers", layer, n_layers, "range", pb, pe, "pools", pools)
    out, lse = attend(su, T, g, layer, n_layers, pb, pe, pieces, want_lse)
    check_float64(su, T, g, layer, n_layers, pb, pe, out, lse, what)
    return out, lse


# ----------------------------------------------------------------------------- partition shapes
# (T, pieces, (len, rem, max_slots)) over all 5 layers
PARTITIONS = [
    (128, 1, (20, 0, 1)),        # one workgroup streams the whole call, through four layer boundaries
    (128, 2, (10, 0, 2)),        # two pieces of three layers each, the cut inside layer 2
    (128, 3, (6, 2, 2)),         # 7 + 7 + 6 tiles: a remainder; the middle piece meets layers 1, 2 and 3
    (128, 7, (2, 6, 2)),         # six pieces of 3 tiles and one of 2
    (128, 19, (1, 1, 4)),        # one piece of 2 tiles, eighteen of one
    (128, 20, (1, 0, 4)),        # every tile a piece of its own
    (512, 5, (16, 0, 1)),        # a piece per layer: every piece boundary a layer boundary, one partial a row
    (512, 6, (13, 2, 2)),        # 14 + 14 + 13 x 4: no boundary on a layer boundary
    (512, 10, (8, 0, 2)),        # two pieces a layer: every second boundary a layer boundary
    (512, 16, (5, 0, 4)),        # pieces of 5 tiles against layers of 16
    (512, 33, (2, 14, 8)),       # fourteen pieces of 3 and nineteen of 2: layers of 6, 6, 7, 8 and 8 partials
    (512, 80, (1, 0, 16)),       # one-tile pieces, 16 partials a row: past the small merge kernel's 8 (k_attend_combine)
]


@pytest.mark.parametrize("T,pieces,expect", PARTITIONS, ids=[f"T{t}-{p}pieces" for t, p, _ in PARTITIONS])
def test_stream_partition_shapes(oracle, rules, T, pieces, expect):
    n_tiles = T // 32
    _, _, _, span = partition(L, n_tiles, pieces)
    if (T, pieces) in ((128, 1), (128, 2), (128, 3)):
        assert span >= 3                                              # a piece over three layers or more
    if (T, pieces) in ((128, 19), (128, 20), (512, 80)):
        assert expect[0] == 1                                         # pieces of one tile
    stream_case(rules, setup_for(oracle, 1), T, pieces, expect=expect)


# ----------------------------------------------------------------------------- query rows
@pytest.mark.parametrize("g,want_lse", [(1, True), (3, True), (8, True), (16, True), (8, False)], ids=["g1", "g3", "g8", "g16", "g8-no-lse"])
def test_stream_query_rows(oracle, rules, g, want_lse):
    """1, 3, 8 and 16 query rows a kv head (the lanes behind the last row are dead columns of the MFMA; at a layer boundary the workgroup
    reloads the next layer's rows), on 7 + 7 + 6 tiles -- a remainder and a piece over three layers; once without a log-sum-exp."""
    _, _, _, span = partition(L, 4, 3)
    assert span == 3
    stream_case(rules, setup_for(oracle, 1), 128, 3, g=g, want_lse=want_lse, expect=(6, 2, 2))


# ----------------------------------------------------------------------------- ranges and layers off 0, a ragged last tile
# (T, pieces, first layer, layers, pos_begin, pos_end, (len, rem, max_slots))
RANGES = [
    (128, 5, 1, 3, 0, 128, (2, 2, 2)),           # layers 1 .. 3: the rows of q / out / lse and the regions count from the call's first layer
    (512, 7, 1, 3, 0, 512, (6, 6, 3)),
    (128, 3, 0, 5, 64, 128, (3, 1, 2)),          # INT4 tiles count from pos_begin: 2 tiles a layer
    (512, 6, 0, 5, 64, 512, (11, 4, 2)),         # 14 tiles a layer
    (512, 6, 0, 5, 0, 482, (13, 2, 2)),          # pos_end = T - 30: 241 pages, the 16th tile of EVERY layer holds one page
    (512, 33, 0, 5, 0, 482, (2, 14, 8)),
    (512, 80, 0, 5, 0, 482, (1, 0, 16)),         # ... and is a piece of its own
    (512, 7, 1, 4, 64, 482, (8, 0, 3)),          # all of it: layers 1 .. 4, positions 64 .. 482 (209 pages: 14 tiles, the last of one page)
]


@pytest.mark.parametrize("T,pieces,layer,n_layers,pb,pe,expect", RANGES, ids=[f"T{c[0]}-{c[1]}pieces-layers{c[2]}+{c[3]}-pos{c[4]}-{c[5]}" for c in RANGES])
def test_stream_ranges_and_layers_off_zero(oracle, rules, T, pieces, layer, n_layers, pb, pe, expect):
    """The ragged cases STREAM: int4_wg8_stream has no condition on the range (MXFP4's decision refuses ragged ranges; this kernel masks the
    last tile of a layer by its index in the layer, wherever in a piece it falls), which stream_case asserts before it checks the rows."""
    stream_case(rules, setup_for(oracle, 1), T, pieces, layer=layer, n_layers=n_layers, pb=pb, pe=pe, expect=expect)


# ----------------------------------------------------------------------------- stream against the fixed grid
@pytest.mark.parametrize("pieces", [6, 33])
def test_stream_equals_the_fixed_grid(oracle, rules, pieces):
    """The same call with attend_stream = -1 (never: the fixed grid of splits x layers workgroups): the same arithmetic in another order of
    summation.  out: the bound tests/test_gpu_mx4.py compares its stream form with its per-layer calls under, |a - b| <= 2e-3 x the row's
    largest |b| + 1e-6; observed here on the MI355X 7.5e-4 (6 pieces) and 6.4e-4 (33 pieces) of the row's largest value.  lse: that test's
    1e-4 was measured for MXFP4; INT4_G32 showed 1.9e-6 for both partitions (two fp32 steps at an lse of 4 .. 8: only the order in which the
    fp32 sums of a row are added differs), more than ten times below it, so the bound here is 2e-5."""
    su = setup_for(oracle, 1)
    assert int4_stream(rules, L, 16, cus(), attend_stream=-1) is None
    a, alse = stream_case(rules, su, 512, pieces)
    b, blse = attend(su, 512, 8, 0, L, 0, 512, -1)
    check_float64(su, 512, 8, 0, L, 0, 512, b, blse, ("fixed grid", pieces))
    rel = float((np.abs(a - b) / np.abs(b).max(axis=-1, keepdims=True)).max())
    dl = float(np.abs(alse - blse).max())
    print(f"int4 stream vs fixed grid, {pieces} pieces: max |a - b| / row max = {rel:.3e}, max |lse a - lse b| = {dl:.3e}")
    assert np.all(np.abs(a - b) <= 2e-3 * np.abs(b).max(axis=-1, keepdims=True) + 1e-6), (pieces, rel)
    assert np.all(np.abs(alse - blse) <= 2e-5), (pieces, dl)


# ----------------------------------------------------------------------------- the residue-class form over a striped pool
# (pools, pieces, pos_end, (len, rem, max_slots)): 256 pages in 3 runs = classes of 86, 85, 85 pages in 6 tiles each, in 7 runs = 37 x 4 and 36 x 3 in 3 tiles each;
# 241 pages (pos_end = T - 30): 81, 80, 80 and 35 x 3, 34 x 4 -- classes of unequal length, ragged last tiles, rows past a class's end masked
CLASSES = [
    (3, 3, 512, (30, 0, 2)), (3, 7, 512, (12, 6, 3)), (3, 3, 482, (30, 0, 2)), (3, 7, 482, (12, 6, 3)),
    (7, 3, 512, (35, 0, 2)), (7, 7, 512, (15, 0, 3)), (7, 3, 482, (35, 0, 2)), (7, 7, 482, (15, 0, 3)),
]


@pytest.mark.parametrize("pools,pieces,pe,expect", CLASSES, ids=[f"{c[0]}pools-{c[1]}pieces-to{c[2]}" for c in CLASSES])
def test_stream_by_residue_classes_over_a_striped_pool(oracle, rules, pools, pieces, pe, expect):
    """k_attend_int4_wg8<1, true> with AttendArgs::stream.tiles: the pages of the range by residue class of the page index, the class-major
    tiles of all layers in one partition; a fresh engine over 3 / 7 runs on this GPU."""
    n_pages = pe // 2
    assert n_pages % pools != 0 and int(striped_tiles(n_pages, pools)) == pools * (-(-(-(-n_pages // pools)) // 16))
    su = setup_for(oracle, pools)
    assert su.lib.stats().n_pool_devices == pools
    stream_case(rules, su, 512, pieces, pe=pe, pools=pools, expect=expect)
    # pieces of one tile are refused in this form (attend_geometry.hpp says why): the fixed grid, and still the float64 rows
    if pieces == 7 and pe == 512:
        n_tiles = int(striped_tiles(n_pages, pools))
        assert int4_stream(rules, L, n_tiles, cus(), cls=True, attend_stream=L * n_tiles) is None
        out, lse = attend(su, 512, 8, 0, L, 0, pe, L * n_tiles)
        check_float64(su, 512, 8, 0, L, 0, pe, out, lse, ("class form, one-tile pieces refused", pools))


# ----------------------------------------------------------------------------- the key at 0 changes nothing
def test_knob_at_zero_small_calls_take_the_fixed_grid(oracle, rules):
    """Runs last: after every case above has set and restored attend_stream, an unforced call of 5 layers x 512 positions decides for the
    fixed grid (896 tiles a layer and 16 a piece are the thresholds) and gives the float64 rows."""
    su = setup_for(oracle, 1)
    assert int4_stream(rules, L, 16, cus()) is None
    out, lse = attend(su, 512, 8, 0, L, 0, 512, 0)
    check_float64(su, 512, 8, 0, L, 0, 512, out, lse, ("fixed grid by default",))
