"""-m gpu: the split pool's decode step of several layers in one launch -- speckv_ext_attend_kv_layers (k_attend_k8v4<false, false,
AttendKvLayers>: grid layer x sequence x head quad, one descriptor per sequence, the tail of an odd length folded by split 0, one merge for all
layers) and SpeckvSplitKVConnector.attend_layers on top of it.

Reference and bound: tests/test_gpu_k8v4_decode.py's (_check: numpy float64 over the oracle's FP8 / MXFP4 records, the tail scored with the fp16
query).  Geometry: the connector counts layers in pairs, so the allocations hold FOUR regions of T = 256 whose contents differ; the calls
cover layers (0..2), (1..2) and (2).  One ragged batch of prefixes of one prompt: 0, 1, 2, 31, 32, 35, 64, 99 and 256 positions -- nothing
stored, a tail alone, one page, a ragged tile plus a tail, a whole tile, a ragged second tile plus a tail, two tiles, a ragged fourth tile
plus a tail, the full region."""
import contextlib
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, graph_capture, set_tuning, torch_mod
from tests.test_gpu_k8v4_decode import PATTERN, SM, T, _check, _checker, _rows

pytestmark = pytest.mark.gpu
LA = 4                                                                            # regions of an allocation (layers of the connector)
LENGTHS = [0, 1, 2, 31, 32, 35, 64, 99, 256]
RIDS = list(range(len(LENGTHS)))
EVEN = [b for b, n in enumerate(LENGTHS) if n % 2 == 0]
RANGES = [(0, 3), (1, 2), (2, 1)]
TUNINGS = [{}, dict(attend_tiles_per_split=1), dict(attend_order_as_given=1)]
_data = {}


def _prompt():
    if "prompt" not in _data:
        rng = np.random.default_rng(4099)
        _data["prompt"] = (_rows(rng, LA, T, H, D), _rows(rng, LA, T, H, D))
    return _data["prompt"]


def _query(g, n_layers=3, batch=len(LENGTHS)):
    if (g, n_layers, batch) not in _data:
        _data[(g, n_layers, batch)] = _rows(np.random.default_rng(700 + g), n_layers, batch, H, g, D)
    return _data[(g, n_layers, batch)]


@contextlib.contextmanager
def _batch(torch, lengths=LENGTHS, tuning=None):
    """a split connector of LA layers whose request b holds the first lengths[b] positions of the prompt (tests/test_gpu_k8v4_decode.py's
    _batch for four regions), under `tuning`"""
    k, v = _prompt()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvSplitKVConnector(lib, LA, H, D, T)
        keep = []
        for rid, n in enumerate(lengths):
            conn.add_request(rid)
            if n:
                keep += conn.write_prefill(rid, torch.from_numpy(np.ascontiguousarray(k[:, :n])).cuda(), torch.from_numpy(np.ascontiguousarray(v[:, :n])).cuda())
        for key, value in (tuning or {}).items():
            set_tuning(key, value)
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
        del keep
    finally:
        for key in tuning or {}:
            set_tuning(key, 0)
        lib.finalize()


def _prepare(torch, conn, rids, q, layer_begin, tails=True, on=None, **change):
    """the arguments of speckv_ext_attend_kv_layers over what the connector holds, out and lse filled with the pattern"""
    NL, B, _, G, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    odd = [r for r in reqs if r.length & 1] if tails else []
    ranks = iter(range(len(odd)))
    hold = dict(q=torch.from_numpy(np.ascontiguousarray(q)).cuda(), out=torch.full((NL, B, H, G, D), PATTERN, dtype=torch.int32, device="cuda"),
                lse=torch.full((NL, B, H, G), PATTERN, dtype=torch.int32, device="cuda"), st=on if on is not None else torch.cuda.Stream(),
                idx=torch.tensor([next(ranks) if r.length & 1 and tails else -1 for r in reqs], dtype=torch.int32).cuda(),
                tk=torch.stack([r.tail_k for r in odd]).contiguous() if odd else None, tv=torch.stack([r.tail_v for r in odd]).contiguous() if odd else None)
    args = dict(k_handles=np.asarray([r.k_handle for r in reqs], np.uint64), v_handles=np.asarray([r.v_handle for r in reqs], np.uint64),
                layer_begin=layer_begin, n_layers=NL, d_q_f16=hold["q"].data_ptr(), g=G, pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32),
                n_tail=len(odd), d_tail_idx=hold["idx"].data_ptr() if odd else 0, d_k_tail=hold["tk"].data_ptr() if odd else 0,
                d_v_tail=hold["tv"].data_ptr() if odd else 0, tail_stride_elems=LA * H * D, sm_scale=SM, d_out=hold["out"].data_ptr(),
                d_lse=hold["lse"].data_ptr(), stream=hold["st"].cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    return args, hold


def _entry(torch, lib, conn, rids, q, layer_begin, **how):
    args, hold = _prepare(torch, conn, rids, q, layer_begin, **how)
    lib.attend_kv_layers(**args)
    hold["st"].synchronize()
    return hold["out"].cpu().numpy().view(np.float32), hold["lse"].cpu().numpy().view(np.float32)


# ----------------------------------------------------------------------------- 1. float64
@pytest.mark.parametrize("tuning", TUNINGS, ids=["default", "tps1", "as_given"])
@pytest.mark.parametrize("g", [1, 4, 16])
@pytest.mark.parametrize("layer_begin,n_layers", RANGES)
def test_the_ragged_batch_of_several_layers_against_float64(oracle, layer_begin, n_layers, g, tuning):
    """every (layer, member, head, row) of the bare entry and of attend_layers; nothing keeps the fill pattern; no state moves.  tps1: every
    tile its own piece -- the tails fold into a partial, the one merge runs across the layers"""
    torch = torch_mod()
    k, v = _prompt()
    q = _query(g)[:n_layers]
    with _batch(torch, tuning=tuning) as (lib, conn):
        tails_before = [(r.tail_k, r.tail_v) for r in conn.requests.values()]
        out, lse = _entry(torch, lib, conn, RIDS, q, layer_begin)
        assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any()
        via = conn.attend_layers(layer_begin, n_layers, RIDS, torch.from_numpy(q).cuda(), SM).cpu().numpy()
        assert via.shape == q.shape and via.dtype == np.float32
        assert [conn.length(r) for r in RIDS] == LENGTHS
        assert all(a is c and b is d for (a, b), (c, d) in zip(tails_before, [(r.tail_k, r.tail_v) for r in conn.requests.values()]))
    for i in range(n_layers):
        layer = layer_begin + i
        tails = [(k[layer, n - 1], v[layer, n - 1]) if n & 1 else None for n in LENGTHS]
        pair, npos = _checker(oracle, "layers", k, v, layer), [n & ~1 for n in LENGTHS]
        worst = _check(pair, out[i], lse[i], q[i], npos, ("entry", layer_begin, n_layers, g, tuning, layer), tails)
        cworst = _check(pair, via[i], None, q[i], npos, ("attend_layers", layer_begin, n_layers, g, tuning, layer), tails)
        print(f"attend_kv_layers {layer_begin}+{n_layers} g {g} {tuning} layer {layer}: worst err / tol {worst:.3f}, attend_layers {cworst:.3f}")


# ----------------------------------------------------------------------------- 2. bits, no tails
@pytest.mark.parametrize("tuning", TUNINGS[:2], ids=["default", "tps1"])
def test_one_layer_is_the_batch_entry_bit_for_bit(tuning):
    """the even lengths of the batch: n_layers = 1 equals speckv_ext_attend_kv_batch of that layer; under attend_tiles_per_split = 1 (the pieces
    cannot depend on the member count) layer l of a three-layer call equals the one-layer call"""
    torch = torch_mod()
    q = _query(4)[:, EVEN]
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    with _batch(torch, tuning=tuning) as (lib, conn):
        three = _entry(torch, lib, conn, EVEN, q, 0) if tuning else None
        for layer in range(3):
            one = _entry(torch, lib, conn, EVEN, q[layer:layer + 1], layer)
            args, hold = _prepare(torch, conn, EVEN, q[layer:layer + 1], layer)
            lib.attend_kv_batch(args["k_handles"], args["v_handles"], layer, args["d_q_f16"], 4, args["pos_end"], SM, args["d_out"], args["d_lse"], args["stream"])
            hold["st"].synchronize()
            assert np.array_equal(bits(hold["out"]), one[0].view(np.uint32)) and np.array_equal(bits(hold["lse"]), one[1].view(np.uint32)), layer
            if three:
                assert np.array_equal(three[0][layer].view(np.uint32), one[0][0].view(np.uint32)), layer
                assert np.array_equal(three[1][layer].view(np.uint32), one[1][0].view(np.uint32)), layer


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing():
    """every refusal of the header: SPECKV_ERR_INVAL, out and lse keep the fill pattern"""
    torch = torch_mod()
    q = _query(4)
    with _batch(torch) as (lib, conn):
        def refused(rids=RIDS, layer_begin=0, q=q, capture=False, **change):
            args, hold = _prepare(torch, conn, rids, q, layer_begin, **change)
            if capture:
                bump = torch.zeros(4, device="cuda")
                graph = torch.cuda.CUDAGraph()
                with graph_capture(graph, hold["st"]):
                    with pytest.raises(SpeckvError) as e:
                        lib.attend_kv_layers(**args)
                    bump.add_(1)
                del graph
            else:
                with pytest.raises(SpeckvError) as e:
                    lib.attend_kv_layers(**args)
            torch.cuda.synchronize()
            assert bool((hold["out"] == PATTERN).all()) and bool((hold["lse"] == PATTERN).all()), (list(change), "a refused call wrote something")
            return e.value.status
        odd_end = np.asarray([n & ~1 for n in LENGTHS], np.uint32)
        odd_end[4] = 31
        many = [8] * 8200                                                        # 8200 x 4 layers x 2 rows > 65535, equal lengths: the grid is not rows-first
        invalid = {
            "a capturing stream": dict(capture=True), "g 0": dict(g=0), "g 17": dict(g=17), "n_layers 0": dict(n_layers=0),
            "a range past the regions": dict(layer_begin=2, tails=False), "a range far past": dict(layer_begin=1000, tails=False),
            "a range past the tail rows": dict(layer_begin=2), "an odd pos_end": dict(pos_end=odd_end),
            "a misaligned q": dict(d_q_f16=0x1008), "a misaligned out": dict(d_out=0x1008), "a misaligned K tail": dict(d_k_tail=0x1008),
            "a misaligned V tail": dict(d_v_tail=0x1008), "a tail stride off 8": dict(tail_stride_elems=LA * H * D + 4),
            "tails without K rows": dict(d_k_tail=0), "tails without V rows": dict(d_v_tail=0), "tails without an index": dict(d_tail_idx=0),
            "a grid beyond the launch limits": dict(rids=many, q=np.zeros((4, len(many), H, 1, D), np.float16)),
        }
        for what, change in invalid.items():
            assert refused(**change) == -4, what                                 # SPECKV_ERR_INVAL
    # an allocation that does not lie in one run: an engine of three pools stripes every allocation
    os.environ["SPECKV_POOL_DEVICES"] = "0,0,0"
    try:
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    finally:
        os.environ.pop("SPECKV_POOL_DEVICES", None)
    try:
        conn = SpeckvSplitKVConnector(lib, LA, H, D, T)
        conn.add_request(0)
        args, hold = _prepare(torch, conn, [0], q[:, :1], 0)
        with pytest.raises(SpeckvError) as e:
            lib.attend_kv_layers(**args)
        torch.cuda.synchronize()
        assert e.value.status == -4 and bool((hold["out"] == PATTERN).all())
    finally:
        lib.finalize()
