"""-m gpu: fetch_range walked from the top (CodecArgs::descending; tuning key fetch_sweep) writes what the ascending walk writes.

A descending launch decodes block n - 1 - i where an ascending one decodes block i: the same waves, rounds and strides, page and
destination alike.  So the two outputs have to be equal bit for bit -- for every pool format, fp16 and fp32 output, ranges of one
block, fewer blocks than a workgroup has waves, several workgroups, a sub-range that does not start at page 0, launches of several
rounds in both orders, and the flat-run kernels (a sealed allocation of data that compresses).  Destinations are pre-filled with a
NaN pattern and carry 4 KiB (fp32: 8 KiB) in front of and behind them that nothing may touch.  The ascending walk itself is held
against the oracle by tests/test_gpu_codec_rounds.py and tests/test_gpu_engine.py; tests/test_fetch_sweep_cpu.py pins the rule and the
index arithmetic.  No timing here: profiles/sweep_direction.txt is the measurement."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.speckv_ctypes import SpeckvLib
from tests._gpu import N, set_tuning, torch_mod

pytestmark = pytest.mark.gpu
PAGE = 4096
ASCENDING, ALTERNATE, DESCENDING = 0, 1, 2         # tuning key fetch_sweep; ALTERNATE is the default
SIZES = [1, 2, 5, 257]
ROUNDS_N = 2500                                    # wgs_per_cu 1 on 256 CUs: 1024 blocks a round, three rounds
POOL_PAGES = ROUNDS_N + 11


@contextlib.contextmanager
def tuned(**keys):
    try:
        for k, v in keys.items():
            set_tuning(k, v)
        yield
    finally:
        for k in keys:
            set_tuning(k, ALTERNATE if k == "fetch_sweep" else 0)


def make_rows(flat):
    """POOL_PAGES blocks: N(0,1) fp16 with a few constant and all-zero blocks among them -- or, flat, the other way round: constant,
    all-zero and long-run blocks with a noisy one in 26 (data the RLE scheme compresses: the engine reads it with the flat-run kernels)"""
    rng = np.random.default_rng(77 + flat)
    x = rng.standard_normal((POOL_PAGES, N))
    if flat:
        for i in range(POOL_PAGES):
            k = i % 13
            if i % 26 == 2:
                continue
            x[i] = 0.0 if k in (4, 9) else np.full(N, x[i, 0]) if k in (0, 7) else np.repeat(x[i, :N // 64], 64)
    else:
        x[3] = 0.0
        x[5] = 0.37
        x[256] = 0.0
        x[1029] = -1.5
        x[ROUNDS_N - 1] = 0.0
    return x.astype(np.float16)


@pytest.fixture(scope="module")
def eng():
    e = SpeckvLib(pkg.library_path(), "hip:0")
    yield e
    set_tuning("fetch_sweep", ALTERNATE)
    e.finalize()


_POOLS = {}


def pool(eng, scheme, flat=False):
    """one allocation per pool format, written once and left unchanged; flat: sealed, so that the packed size picks the flat-run decoder"""
    key = (scheme, flat)
    if key not in _POOLS:
        x = make_rows(flat)
        eng.set_compression_scheme(scheme)
        h = eng.alloc(POOL_PAGES * PAGE)
        eng.write(h, 0, x.ctypes.data, x.nbytes, False)
        if flat:
            eng.compact(h)
        _POOLS[key] = h
    return _POOLS[key]


def fetch(eng, h, first, n, f32, sweep, stream):
    """fetch_range under a forced direction into a NaN-filled buffer with a guard row on either side; returns (rows, guards)"""
    torch = torch_mod()
    buf = torch.full((n + 2, N), float("nan"), dtype=torch.float32 if f32 else torch.float16, device="cuda")
    with tuned(fetch_sweep=sweep):
        eng.fetch_range(h, first, n, buf[1:].data_ptr(), f32, stream.cuda_stream)
        stream.synchronize()
    return buf


def ints(t):
    torch = torch_mod()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_pair(up, down, what):
    torch = torch_mod()
    nan = ints(torch.full((1,), float("nan"), dtype=up.dtype, device="cuda"))
    for name, buf in (("ascending", up), ("descending", down)):
        assert bool((ints(buf[0]) == nan).all()), f"{what} {name}: the 4 KiB in front of the destination were written"
        assert bool((ints(buf[-1]) == nan).all()), f"{what} {name}: the 4 KiB behind the destination were written"
    assert torch.equal(ints(up[1:-1]), ints(down[1:-1])), f"{what}: the descending launch wrote other bytes"
    return up


def both_directions(eng, h, sizes, what):
    torch = torch_mod()
    stream = torch.cuda.Stream()
    for n in sizes:
        for first in (0, 7):
            for f32 in (False, True):
                w = f"{what} n {n} first {first} f32 {f32}"
                up = fetch(eng, h, first, n, f32, ASCENDING, stream)
                down = fetch(eng, h, first, n, f32, DESCENDING, stream)
                check_pair(up, down, w)
                if n > 1:                                   # the pool's blocks differ: a walk that mixed up rows would show
                    assert not torch.equal(ints(up[1]), ints(up[n])), w


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_descending_fetch_writes_the_ascending_bytes(eng, scheme):
    both_directions(eng, pool(eng, scheme), SIZES, f"scheme {scheme}")


@pytest.mark.parametrize("consecutive", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_descending_fetch_over_three_rounds(eng, scheme, consecutive):
    h = pool(eng, scheme)
    with tuned(wgs_per_cu=1, rounds_consecutive=consecutive):
        grid, per_wave, step = eng.codec_launch_shape(ROUNDS_N)
        assert per_wave == 3 and step == (0 if consecutive else 4 * grid), (grid, per_wave, step)
        both_directions(eng, h, [ROUNDS_N], f"scheme {scheme} three rounds consecutive {consecutive}")


def test_descending_fetch_through_the_flat_run_kernels(eng):
    h = pool(eng, 2, flat=True)
    before = eng.stats().flat_decoder_fetches
    both_directions(eng, h, SIZES, "flat-run")
    with tuned(wgs_per_cu=1):
        both_directions(eng, h, [ROUNDS_N], "flat-run three rounds")
    assert eng.stats().flat_decoder_fetches - before == (len(SIZES) + 1) * 2 * 2 * 2, "the sealed allocation was not read by the flat-run kernels"


def test_the_default_rule_alternates_and_keeps_the_bytes(eng):
    """The default setting: the same range four times (ascending, descending, ascending, descending), another range (ascending), the first
    again (ascending: the range changed in between) -- every output is the forced-ascending one."""
    torch = torch_mod()
    stream = torch.cuda.Stream()
    h = pool(eng, 2)
    a, b = (0, 257), (7, 300)
    want = {r: fetch(eng, h, r[0], r[1], False, ASCENDING, stream) for r in (a, b)}
    for k, r in enumerate((a, a, a, a, b, a)):
        buf = torch.full((r[1] + 2, N), float("nan"), dtype=torch.float16, device="cuda")
        eng.fetch_range(h, r[0], r[1], buf[1:].data_ptr(), False, stream.cuda_stream)
        stream.synchronize()
        check_pair(want[r], buf, f"default rule, call {k} over {r}")
