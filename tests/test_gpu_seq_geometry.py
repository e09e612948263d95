"""-m gpu: the single-sequence attention entries (speckv_ext_attend_fp8 / _int4 / _mx4) against float64, one case per outcome of their launch
decision (attend_geometry.hpp seq_decide) at the smallest shape that reaches it: 1 or 2 layers, 8 tiles of 32 positions at most.

Every case (1) asserts on the host that it reaches the outcome it names -- through the decision the engine itself takes (tests/_rules.py decide_seq
over tests/csrc/host_rules_test.cpp), fed the device's CU count and the tuning keys the case sets; a failing regime assertion means the case no longer
tests what it says it tests; (2) pre-fills out and lse with NaN and runs the call with those keys set through speckv_ext_set_tuning (restored
afterwards); (3) checks EVERY (layer, head, query row) of out and lse against the float64 attention over the dequantised records, with the bound the
formats' own tests use (tests/_gpu.py HeadChecker.check_rows: |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, lse within 2e-3 + delta; delta = the score
error bound of the 8-bit query formats, 0 for INT4_G32).

Placements: one engine over one pool (records in one run), one over two pools on this GPU (striped over 2 runs); the page-table forms through
attend_general = 1.  Data: N(0, 1) x a per-page magnitude in [0.2, 3), a page of zeros in K and in V; queries 1.5 x N(0, 1) in fp16.  Seeds are fixed."""
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from tests._gpu import D, H, HeadChecker, set_tuning, torch_mod
from tests._rules import FP8, FP8_KERNELS, INT4, MX4, SEQ_PLACES, decide_seq, load_rules

pytestmark = pytest.mark.gpu
PAGE = 4096
L = 2
SM = 1.0 / np.sqrt(D)
NAMES = {FP8: "fp8", INT4: "int4", MX4: "mx4"}
LAYOUTS = (256, 250)                               # positions per layer: 8 whole tiles; 250 = no multiple of 32 (FP8: a layout without a scale table)


@pytest.fixture(scope="module")
def rules():
    return load_rules()


def cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- one engine at a time, its allocations and checkers built once
class Setup:
    """An engine over `pools` pools on this GPU with one allocation of L layers per (format, layout) and the float64 checker of every layer; queries
    for the row counts the cases use.  Nothing here changes after it is built."""

    def __init__(self, oracle, pools):
        torch = torch_mod()
        if pools > 1:
            os.environ["SPECKV_POOL_DEVICES"] = ",".join(["0"] * pools)
        try:
            self.kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), "hip:0")
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        self.lib = self.kv.lib
        assert self.lib.stats().n_pool_devices == pools
        self.handle, self.checkers = {}, {}
        for scheme in (FP8, INT4, MX4):
            self.lib.set_compression_scheme(scheme)
            for T in LAYOUTS if (scheme == FP8 and pools == 1) else LAYOUTS[:1]:
                rng = np.random.default_rng(9300 + 10 * scheme + T + pools)
                n_pages = T * L                                          # a layer: T / 2 pages of K, then T / 2 of V
                x = (rng.standard_normal((n_pages, 2048)) * rng.uniform(0.2, 3.0, (n_pages, 1))).astype(np.float16)
                x[5] = 0.0                                               # layer 0, K: a page of zeros
                x[T + T // 2 + 40] = 0.0                                 # layer 1, V
                h = self.lib.alloc(n_pages * PAGE)
                self.lib.set_layout(h, T, L, H, D, 2)
                self.lib.write(h, 0, x.ctypes.data, x.nbytes, False)
                self.handle[scheme, T] = h
                self.checkers[scheme, T] = [HeadChecker(oracle, scheme, x[l * T:(l + 1) * T], T) for l in range(L)]
        qrng = np.random.default_rng(9400 + pools)
        self.qh = {g: (qrng.standard_normal((L, H, g, D)) * 1.5).astype(np.float16) for g in (8, 9)}
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
        _state["setup"] = Setup(oracle, pools)
        _state["pools"] = pools
    return _state["setup"]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_setup()


def decision(rules, scheme, pools, T, n_layers, g, pb, pe, keys):
    """What the engine decides for the call: the range as Engine::attend_begin hands it on (FP8 over a scale table: from the table's tile, the pages in
    front of pos_begin masked), the placement the engine over `pools` pools gives (one run, or striped over `pools` runs)."""
    has_tab = scheme == FP8 and T % 32 == 0
    begin = pb - pb % 32 if has_tab else pb
    return decide_seq(rules, scheme, n_layers, (pe - begin) // 2, cus(), g=g, num_tokens=T, pos_begin=begin, skip_pages=(pb - begin) // 2, has_tab=has_tab,
                      one_run=pools == 1, stripe_n=pools, tuning=keys)


# (name, format, pools, layout, layers, g, pos_begin, pos_end, tuning keys, the outcome the case names: fields of the decision)
def fp8(kernel, **kw):
    return dict(fp8_kernel=FP8_KERNELS.index(kernel), **kw)


def place(name, **kw):
    return dict(place=SEQ_PLACES.index(name), **kw)


CASES = [
    # FP8
    ("dma0-one-split", FP8, 1, 256, 1, 8, 0, 64, {}, fp8("dma<0>", n_tiles=2, n_splits=1, rows_final=1, **place("linear"))),
    ("regs-linear-merge", FP8, 1, 256, 1, 8, 0, 128, dict(attend_fp8_dma=-1, attend_splits=2), fp8("linear<false>", n_tiles=4, n_splits=2, rows_final=0, **place("linear"))),
    ("dma2-by-class", FP8, 2, 256, 2, 8, 0, 256, {}, fp8("dma<2>", cls=1, n_tiles=8, **place("striped"))),
    ("dma1-striped-through-the-table", FP8, 2, 256, 2, 8, 0, 256, dict(attend_fp8_striped_table=1), fp8("dma<1>", cls=0, **place("striped"))),
    ("dma1-table", FP8, 1, 256, 2, 8, 0, 256, dict(attend_general=1), fp8("dma<1>", **place("table"))),
    ("regs-striped", FP8, 2, 256, 2, 8, 0, 256, dict(attend_fp8_table_regs=1), fp8("linear<true>", cls=0, **place("striped"))),
    ("regs-table", FP8, 1, 256, 2, 8, 0, 256, dict(attend_general=1, attend_fp8_table_regs=1), fp8("linear<false, true>", **place("table"))),
    ("regs-striped-inside-a-tile", FP8, 2, 256, 2, 8, 10, 256, {}, fp8("linear<true>", cls=0, n_tiles=8, **place("striped"))),
    ("regs-table-inside-a-tile", FP8, 1, 256, 2, 8, 42, 256, dict(attend_general=1), fp8("linear<false, true>", n_tiles=7, **place("table"))),
    ("per-wave-no-scale-table", FP8, 1, 250, 2, 8, 0, 250, {}, fp8("k_attend_fp8", quantize_q=1, rows_final=0, **place("none"))),
    ("ragged", FP8, 1, 256, 2, 8, 0, 250, {}, fp8("dma<0>", n_tiles=8, **place("linear"))),
    ("ragged-two-splits", FP8, 1, 256, 2, 8, 0, 250, dict(attend_splits=2), fp8("dma<0>", n_tiles=8, n_splits=2, tiles_per_split=4, rows_final=0, **place("linear"))),
    # INT4_G32
    ("wg8-fixed-grid", INT4, 1, 256, 1, 8, 0, 256, {}, place("linear", wg8=1, cls=0, stream=None, n_splits=1, rows_final=1)),
    ("wg8-by-class", INT4, 2, 256, 2, 8, 0, 256, {}, place("striped", wg8=1, cls=1, n_tiles=8, stream=None)),
    ("wg8-stream", INT4, 1, 256, 2, 8, 0, 128, dict(attend_stream=3), place("linear", wg8=1, stream=dict(n_wgs=3, len=2, rem=2, max_slots=2, tiles=0), slots=2, rows_final=0)),
    ("striped-4-head-kernel", INT4, 2, 256, 2, 8, 0, 256, dict(attend_int4_striped_wg=1), place("striped", wg8=0, cls=0)),
    ("table", INT4, 1, 256, 2, 8, 0, 256, dict(attend_general=1), place("table", wg8=0, zero_page=1)),
    ("ragged", INT4, 1, 256, 2, 8, 0, 250, {}, place("linear", wg8=1, n_tiles=8)),
    ("ragged-two-splits", INT4, 1, 256, 2, 8, 0, 250, dict(attend_splits=2), place("linear", wg8=1, n_splits=2, tiles_per_split=4, stream=None, rows_final=0)),
    # MXFP4
    ("linear", MX4, 1, 256, 2, 8, 0, 256, {}, place("linear", cls=0, stream=None)),
    ("striped-by-class", MX4, 2, 256, 2, 8, 0, 256, {}, place("striped", cls=1, n_tiles=8)),
    ("table", MX4, 1, 256, 2, 8, 0, 256, dict(attend_general=1), place("table", zero_page=1)),
    ("stream", MX4, 1, 256, 2, 8, 0, 128, dict(attend_stream=3), place("linear", stream=dict(n_wgs=3, len=2, rem=2, max_slots=2, tiles=0), slots=2, rows_final=0)),
    ("two-row-groups", MX4, 1, 256, 2, 9, 0, 256, {}, place("linear", stream=None)),
    ("ragged", MX4, 1, 256, 2, 8, 0, 250, {}, place("linear", n_tiles=8, stream=None)),
    ("ragged-two-splits", MX4, 1, 256, 2, 8, 0, 250, dict(attend_splits=2), place("linear", n_splits=2, tiles_per_split=4, stream=None, rows_final=0)),
    ("ragged-stream-refused", MX4, 1, 256, 2, 8, 0, 250, dict(attend_stream=3), place("linear", stream=None)),
]
CASES.sort(key=lambda c: c[2])                     # one engine at a time: the one-pool cases first


@pytest.mark.parametrize("name,scheme,pools,T,n_layers,g,pb,pe,keys,outcome", CASES, ids=[f"{NAMES[c[1]]}-{c[0]}" for c in CASES])
def test_single_sequence_attention_in_every_outcome_of_its_decision(oracle, rules, name, scheme, pools, T, n_layers, g, pb, pe, keys, outcome):
    torch = torch_mod()
    d = decision(rules, scheme, pools, T, n_layers, g, pb, pe, keys)
    assert {k: d[k] for k in outcome} == outcome, (name, d)                  # the case reaches the outcome it names
    if "ragged" in name:
        assert ((pe - pb) // 2) % 16 != 0
    su = setup_for(oracle, pools)
    layer = L - n_layers                                                     # (a single layer: the last one, so that the call's first layer is off 0)
    out = torch.full((n_layers, H, g, D), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((n_layers, H, g), float("nan"), dtype=torch.float32, device="cuda")
    call = {FP8: su.lib.attend_fp8, INT4: su.lib.attend_int4, MX4: su.lib.attend_mx4}[scheme]
    for k, v in keys.items():
        set_tuning(k, v)
    try:
        call(su.handle[scheme, T], layer, n_layers, su.q[g][layer].data_ptr(), g, pb, pe, SM, out.data_ptr(), lse.data_ptr())
        torch.cuda.synchronize()
    finally:
        for k in keys:
            set_tuning(k, 0)
    out, lse = out.cpu().numpy(), lse.cpu().numpy()
    for i in range(n_layers):
        hc = su.checkers[scheme, T][layer + i]
        for head in range(H):
            hc.check_rows(out[i, head][None], lse[i, head][None], su.qh[g][layer + i, head][None], head, [pe - pb], SM,
                          (NAMES[scheme], name, "layer", layer + i, "head", head), pos_begin=pb)
