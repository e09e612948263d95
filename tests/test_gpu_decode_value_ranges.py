"""-m gpu: the decode attention bodies over value ranges INSIDE the attended span, against float64 -- V magnitude ladders across tiles and inside a
tile, a dominant key on the smallest-V page, tile maxima that ramp by >= 8 nats a tile, all-zero K, zero V tiles, and zero / spike / tiny / fp16-extreme
query rows (tests/_value_ranges.py; tests/test_value_ranges_cpu.py proves without a GPU that every data set is what it claims and decides the bound).

Every case (1) asserts on the host that it reaches the body it names, through the decision the engine itself takes (tests/_rules.py decide_seq / decide,
fed the device's CU count and the case's tuning keys); (2) pre-fills out and lse with NaN; (3) checks EVERY (layer, head, query row) of out and lse
against the float64 attention over the dequantised records (tests/_gpu.py HeadChecker.check_rows) and requires every output finite.  The bound: the
project's, |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6 and lse within 2e-3 + delta, unchanged for a tier-1 profile; for a tier-2 profile (sink) out
gets 2 x term on top, what the kernels' declared fp16 weights cost (_value_ranges.term_rows; the FP8 term in the tile map of the body: 32 consecutive
positions, or two residue classes for k_attend_fp8_dma<2>).  The tier is decided on the CPU from the model, never here.

Single-sequence entries: both layers in one call (layer 0 ordinary, layer 1 the profile), the ranges (0, 256) and the ragged (0, 250), with one split
(attend_splits = 1) and with two (tiles_per_split = 4).  Batch entries and the split pool (attend_kv_batch): three members of 256, 250 and 64 positions
over the same content, as given (one piece each) and in pieces of 4 tiles with the merge (attend_tiles_per_split = 4).  The worst err / tol per
(profile, body) is printed."""
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from tests import _value_ranges as vr
from tests._gpu import D, H, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, FP8, FP8_KERNELS, INT4, MX4, SEQ_PLACES, decide, decide_seq, load_rules

pytestmark = pytest.mark.gpu
PAGE = 4096
G, L = vr.G, vr.L
MEMBERS = (256, 250, 64)


@pytest.fixture(scope="module")
def rules():
    return load_rules()


def cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- one engine at a time; an allocation once per (data set, format, layout)
class Setup:
    def __init__(self, pools):
        self.torch = torch_mod()
        self.pools, self.handle, self.q, self.pairs, self.keep = pools, {}, {}, {}, []
        if pools == "k8v4":                                          # the split pool: a library of its own, one connector, a request per data set
            self.kv = None
            self.lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
            self.conn = SpeckvSplitKVConnector(self.lib, L, H, D, 256)
            return
        if pools > 1:
            os.environ["SPECKV_POOL_DEVICES"] = ",".join(["0"] * pools)
        try:
            self.kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), "hip:0")
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        self.lib = self.kv.lib
        assert self.lib.stats().n_pool_devices == pools

    def alloc(self, name, scheme, T):
        key = (name, scheme, T)
        if key not in self.handle:
            x = vr.dataset(name, T)["x"]
            self.lib.set_compression_scheme(scheme)
            h = self.lib.alloc(len(x) * PAGE)
            self.lib.set_layout(h, T, L, H, D, 2)
            self.lib.write(h, 0, x.ctypes.data, x.nbytes, False)
            self.torch.cuda.synchronize()
            self.handle[key] = h
        return self.handle[key]

    def pair(self, name):
        """(K handle, V handle) of the data set in the split pool"""
        if name not in self.pairs:
            ds, t = vr.dataset(name), self.torch
            k, v = (np.stack([ds["kv16_layer0"][i], ds["kv16"][i]]) for i in (0, 1))
            self.pairs[name] = self.conn.add_request(name)
            self.keep += self.conn.write_prefill(name, t.from_numpy(k).cuda(), t.from_numpy(v).cuda())
            t.cuda.synchronize()
        return self.pairs[name]

    def query(self, name, T, members=None):
        """the data set's query on the device: [L][H][G][D], or -- members -- layer 1's rows for every member [n][H][G][D]"""
        key = (name, T, members)
        if key not in self.q:
            q = vr.dataset(name, T)["q"]
            self.q[key] = self.torch.from_numpy(np.array(q if members is None else np.repeat(q[1][None], members, axis=0))).cuda()      # (a copy: the data set is read-only)
        return self.q[key]

    def close(self):
        self.torch.cuda.synchronize()
        if self.kv is None:
            self.keep.clear()
            self.lib.finalize()
            return
        for h in self.handle.values():
            self.lib.free(h)
        self.kv.close()


_state = {"pools": None, "setup": None}


def drop_setup():
    if _state["setup"] is not None:
        _state["setup"].close()
    _state.update(pools=None, setup=None)


def setup_for(pools):
    if _state["pools"] != pools:
        drop_setup()
        _state["setup"] = Setup(pools)
        _state["pools"] = pools
    return _state["setup"]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_setup()


# ----------------------------------------------------------------------------- the float64 side, once per (data set, format, layer, head, lengths)
_want = {}


def hold_want(hc):
    """want_rows of a checker, remembered per (head, lengths): the queries of a data set never change"""
    if "want_rows" not in hc.__dict__:
        plain, memo = hc.want_rows, {}

        def want_rows(q16, head, npos, sm, tail=None, pos_begin=0):
            key = (head, tuple(int(n) for n in npos), np.asarray(q16).shape)
            if key not in memo:
                memo[key] = plain(q16, head, npos, sm, tail, pos_begin)
            return memo[key]
        hc.want_rows = want_rows
    return hc


def extra(oracle, name, T, fmt, head, npos, stripe_n):
    key = (name, T, fmt, head, tuple(npos), stripe_n)
    if key not in _want:
        _want[key] = vr.extra_tol(oracle, name, T, fmt, head, list(npos), stripe_n=stripe_n)
    return _want[key]


class Worst:
    """the worst err / tol per profile of one body, printed when the body's test ends (also when it fails)"""

    def __init__(self, body):
        self.body, self.by, self.failed = body, {}, []

    def check(self, hc, name, *args, **kw):
        """check_rows; a row outside its bound is kept for the end of the body's test, so that every data set is run and printed"""
        try:
            hc.check_rows(*args, worst=self.list_for(name), **kw)
        except AssertionError as e:
            self.failed.append(str(e))

    def list_for(self, name):
        return self.by.setdefault(vr.PROFILE_OF[name], [])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for prof, w in self.by.items():
            print(f"value-ranges {self.body} {prof}: worst err / tol {max(w):.3f}")
        assert exc[0] is not None or not self.failed, (self.body, len(self.failed), self.failed[:4])
        return False


def check_exact(name, out1, lse1):
    """layer 1's rows of a data set whose answer is exact in every format"""
    if name == "ties-v0":
        assert not out1.any(), "V is zero everywhere: out must be exactly 0"


# ----------------------------------------------------------------------------- single-sequence entries
def fp8(kernel, **kw):
    return dict(fp8_kernel=FP8_KERNELS.index(kernel), **kw)


def place(name, **kw):
    return dict(place=SEQ_PLACES.index(name), **kw)


# (name, format, pools, layout, tuning keys, the body: fields of the decision)
BODIES = [
    ("dma0", FP8, 1, 256, {}, fp8("dma<0>", **place("linear"))),
    ("regs-linear", FP8, 1, 256, dict(attend_fp8_dma=-1), fp8("linear<false>", **place("linear"))),
    ("per-wave", FP8, 1, 250, {}, fp8("k_attend_fp8", quantize_q=1, rows_final=0, **place("none"))),        # (this body always goes through the merge)
    ("dma1-table", FP8, 1, 256, dict(attend_general=1), fp8("dma<1>", **place("table"))),
    ("regs-table", FP8, 1, 256, dict(attend_general=1, attend_fp8_table_regs=1), fp8("linear<false, true>", **place("table"))),
    ("dma2-by-class", FP8, 2, 256, {}, fp8("dma<2>", cls=1, **place("striped"))),
    ("regs-striped", FP8, 2, 256, dict(attend_fp8_table_regs=1), fp8("linear<true>", cls=0, **place("striped"))),
    ("wg8", INT4, 1, 256, {}, place("linear", wg8=1, cls=0, stream=None)),
    ("table", INT4, 1, 256, dict(attend_general=1), place("table", wg8=0)),
    ("wg8-by-class", INT4, 2, 256, {}, place("striped", wg8=1, cls=1, stream=None)),
    ("striped-4-head-kernel", INT4, 2, 256, dict(attend_int4_striped_wg=1), place("striped", wg8=0, cls=0)),
    ("linear", MX4, 1, 256, {}, place("linear", cls=0, stream=None)),
    ("table", MX4, 1, 256, dict(attend_general=1), place("table")),
    ("striped-by-class", MX4, 2, 256, {}, place("striped", cls=1)),
]
SEQ_CASES = sorted(((b, s) for b in BODIES for s in (1, 2)), key=lambda c: c[0][2])          # one engine at a time: the one-pool cases first


@pytest.mark.parametrize("body,splits", SEQ_CASES, ids=[f"{vr.NAMES[b[1]]}-{b[0]}-{s}-split{'s' if s > 1 else ''}" for b, s in SEQ_CASES])
def test_single_sequence_bodies_over_value_ranges(oracle, rules, body, splits):
    torch = torch_mod()
    bname, scheme, pools, T, keys, outcome = body
    keys = dict(keys, attend_splits=splits)
    ranges = [n for n in vr.RANGES if n <= T] if T == 256 else [250]
    has_tab = scheme == FP8 and T % 32 == 0
    stripe_n = 1
    for n in ranges:                                                             # the case reaches the body it names, with the splits it names
        d = decide_seq(rules, scheme, L, n // 2, cus(), g=G, num_tokens=T, pos_begin=0, skip_pages=0, has_tab=has_tab, one_run=pools == 1,
                       stripe_n=pools, tuning=keys)
        assert {k: d[k] for k in outcome} == outcome, (bname, n, d)
        assert d["n_tiles"] == 8 and d["n_splits"] == splits and d["tiles_per_split"] == 8 // splits, (bname, n, d)
        assert d["rows_final"] == (1 if splits == 1 and "rows_final" not in outcome else 0), (bname, n, d)     # one split: final from the body itself
        stripe_n = pools if (scheme == FP8 and d["cls"]) else 1
    su = setup_for(pools)
    call = {FP8: su.lib.attend_fp8, INT4: su.lib.attend_int4, MX4: su.lib.attend_mx4}[scheme]
    with Worst(f"{vr.NAMES[scheme]} {bname} splits {splits}") as worst:
        for name in vr.DATASETS:
            ds = vr.dataset(name, T)
            h, q = su.alloc(name, scheme, T), su.query(name, T)
            for n in ranges:
                out = torch.full((L, H, G, D), float("nan"), dtype=torch.float32, device="cuda")
                lse = torch.full((L, H, G), float("nan"), dtype=torch.float32, device="cuda")
                for k, v in keys.items():
                    set_tuning(k, v)
                try:
                    call(h, 0, L, q.data_ptr(), G, 0, n, ds["sm"], out.data_ptr(), lse.data_ptr())
                    torch.cuda.synchronize()
                finally:
                    for k in keys:
                        set_tuning(k, 0)
                out, lse = out.cpu().numpy(), lse.cpu().numpy()
                assert np.isfinite(out).all() and np.isfinite(lse).all(), (bname, name, n, "an output is not finite")
                check_exact(name, out[1], lse[1])
                for layer in range(L):
                    hc = hold_want(vr.checker(oracle, name, T, scheme, layer))
                    for head in range(H):
                        xt = extra(oracle, name, T, scheme, head, (n,), stripe_n) if layer == 1 else None
                        worst.check(hc, name, out[layer, head][None], lse[layer, head][None], ds["q"][layer, head][None], head, [n], ds["sm"],
                                    (vr.NAMES[scheme], bname, splits, name, n, "layer", layer, "head", head), extra_tol=xt)


# ----------------------------------------------------------------------------- batch entries on one pool
BATCH_CASES = [(s, p) for s in (FP8, INT4, MX4) for p in (False, True)]


def batch_decision(rules, scheme, pieces):
    """three members as given: one piece each, final from the attention kernel; attend_tiles_per_split = 4: the members of 8 tiles in two pieces and
    the merge, the member of 2 tiles final in the same launch (rows first)"""
    pages = np.asarray(MEMBERS) // 2
    d = decide(rules, scheme, "batch", pages, cus(), tuning=((4,) + DEFAULT_TUNING[1:]) if pieces else DEFAULT_TUNING)
    assert d["fits"] == 1 and not d["table"] and not d["striped"], d
    if pieces:
        assert d["tps"] == 4 and d["max_splits"] == 2 and d["rows_first"] == 1 and [int(x) for x in d["pieces"][:, 1]] == [2, 2, 1], d
    else:
        assert d["max_splits"] == 1 and [int(x) for x in d["pieces"][:, 1]] == [1, 1, 1], d
    return d


@pytest.mark.parametrize("scheme,pieces", BATCH_CASES, ids=[f"{vr.NAMES[s]}-{'pieces-and-merge' if p else 'as-given'}" for s, p in BATCH_CASES])
def test_batch_entries_over_value_ranges(oracle, rules, scheme, pieces):
    torch = torch_mod()
    batch_decision(rules, scheme, pieces)
    su = setup_for(1)
    batch = {FP8: su.lib.attend_fp8_batch, INT4: su.lib.attend_int4_batch, MX4: su.lib.attend_mx4_batch}[scheme]
    n = len(MEMBERS)
    with Worst(f"{vr.NAMES[scheme]} batch {'pieces' if pieces else 'as given'}") as worst:
        for name in vr.DATASETS:
            ds = vr.dataset(name)
            h, q = su.alloc(name, scheme, 256), su.query(name, 256, n)
            out = torch.full((n, H, G, D), float("nan"), dtype=torch.float32, device="cuda")
            lse = torch.full((n, H, G), float("nan"), dtype=torch.float32, device="cuda")
            set_tuning("attend_tiles_per_split", 4 if pieces else 0)
            try:
                batch([h] * n, 1, q.data_ptr(), G, np.asarray(MEMBERS, np.uint32), ds["sm"], out.data_ptr(), lse.data_ptr())
                torch.cuda.synchronize()
            finally:
                set_tuning("attend_tiles_per_split", 0)
            out, lse = out.cpu().numpy(), lse.cpu().numpy()
            assert np.isfinite(out).all() and np.isfinite(lse).all(), (name, "an output is not finite")
            check_exact(name, out, lse)
            hc = hold_want(vr.checker(oracle, name, 256, scheme))
            for head in range(H):
                worst.check(hc, name, out[:, head], lse[:, head], np.repeat(ds["q"][1, head][None], n, axis=0), head, list(MEMBERS), ds["sm"],
                            (vr.NAMES[scheme], "batch", pieces, name, "head", head), extra_tol=extra(oracle, name, 256, scheme, head, MEMBERS, 1))


# ----------------------------------------------------------------------------- the split pool: K from the FP8 records, V from the MXFP4 records
@pytest.mark.parametrize("pieces", [False, True], ids=["final", "merged"])
def test_split_pool_over_value_ranges(oracle, rules, pieces):
    torch = torch_mod()
    batch_decision(rules, FP8, pieces)                                         # (attend_kv_batch decides as BatchShape{fp8 = true}: tests/_k8v4_cases.py)
    su = setup_for("k8v4")
    n = len(MEMBERS)
    st = torch.cuda.Stream()
    with Worst(f"k8v4 batch {'merged' if pieces else 'final'}") as worst:
        for name in vr.DATASETS:
            ds = vr.dataset(name)
            kh, vh = su.pair(name)
            q = su.query(name, 256, n)
            out = torch.full((n, H, G, D), float("nan"), dtype=torch.float32, device="cuda")
            lse = torch.full((n, H, G), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            set_tuning("attend_tiles_per_split", 4 if pieces else 0)
            try:
                su.lib.attend_kv_batch(np.asarray([kh] * n, np.uint64), np.asarray([vh] * n, np.uint64), 1, q.data_ptr(), G, np.asarray(MEMBERS, np.uint32),
                                       ds["sm"], out.data_ptr(), lse.data_ptr(), st.cuda_stream)
                st.synchronize()
            finally:
                set_tuning("attend_tiles_per_split", 0)
            out, lse = out.cpu().numpy(), lse.cpu().numpy()
            assert np.isfinite(out).all() and np.isfinite(lse).all(), (name, "an output is not finite")
            check_exact(name, out, lse)
            hc = hold_want(vr.checker(oracle, name, 256, vr.K8V4))
            for head in range(H):
                worst.check(hc, name, out[:, head], lse[:, head], np.repeat(ds["q"][1, head][None], n, axis=0), head, list(MEMBERS), ds["sm"],
                            ("k8v4", pieces, name, "head", head), extra_tol=extra(oracle, name, 256, vr.K8V4, head, MEMBERS, 1))
