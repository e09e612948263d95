"""-m gpu: the split pool's decode route under a SLIDING WINDOW -- speckv_ext_attend_kv_batch_window (k_attend_k8v4<true>: every member
walked from its window's tile in the FP8 K allocation and in the MXFP4 V allocation, the leading positions of that tile masked) and
SpeckvSplitKVConnector.attend(window=W) on top of it.

The conventions are those of tests/test_gpu_decode_window.py and tests/test_gpu_k8v4_decode.py.  A member has `length` positions, the
step's own included: stored = length & ~1 of them in the pool, an odd length its last one in the caller's tail; its query sees
[lo, length - 1], lo = max(0, length - W) (csrc/decode_window.hpp).  Every member has its OWN pair of allocations holding all 256
positions, written through write_prefill, and EVERY position below lo and at or behind stored is hostile (K x 200, V = +-1000): an odd
lo puts a hostile row into a kept position's FP8 page scale and MXFP4 block code.  Reference: numpy float64 attention over the oracle's
records of exactly [lo, stored) -- K from HeadChecker(oracle, FP8), V from HeadChecker(oracle, MXFP4), the query through q_rows (E4M3 x
a row scale) -- plus the fp16 tail for the connector route: the _check of tests/test_gpu_k8v4_decode.py with a lower bound.  Bound: the
project's, |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, lse within 2e-3 + delta, delta = 3e-5 max sum |q||k| sm per (member, head); a
member without a position is exactly 0 with lse -inf.  Every (member, head, row) is compared; the worst err / tol of a case is printed
before anything is asserted.

Layout: L = 2 (both layers hostile, both used), T = 256, H = 8, D = 128, g = 8 (one case each with g = 1 and g = 16).  Batches A = 1, 2,
33, 64, 65, 98, 131, 255 and B = 256, 255, 64, 33, 98, 131; W = 1, 2, 31, 32, 33, 64, 100, 300: lo odd and even, on and inside a tile,
lo = 0, an empty pool with and without a tail, a ragged last tile, the first and the last tile coinciding, and W = 300, which cuts
nobody and must be byte-identical to speckv_ext_attend_kv_batch."""
import contextlib
import itertools

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, decide, load_rules
from tests.test_gpu_decode_window import LENGTHS_A, LENGTHS_B, NEEDLE_LENGTHS, NEEDLE_W, WINDOWS, checker, content, needle_dirs, span
from tests.test_gpu_hostile_ranges import drop_engine
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
G, L, T = 8, 2, 256
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19
FP8, MX4 = 4, 5

_rids = itertools.count(1)


@contextlib.contextmanager
def _pool(torch):
    """an engine with one pool and a split connector over it (one engine in the process at a time)"""
    drop_engine()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        yield lib, SpeckvSplitKVConnector(lib, L, H, D, T)
        torch.cuda.synchronize()
    finally:
        lib.finalize()


def _cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


def member_check(pair, out, lse, q, lo, stored, what, tail=None):
    """ONE member: out [H][G][D], lse [H][G] (None: a call that returns the rows alone), q [H][G][D] fp16, over the content of pair = (FP8
    HeadChecker, MXFP4 HeadChecker), attending its stored positions [lo, stored) (and its fp16 tail (k [H][D], v [H][D]), scored with the
    fp16 query) against float64 -> (worst err / tol, the first row that missed or None)"""
    k8, v4 = pair
    worst, first = 0.0, None
    for head in range(H):
        K, V = k8.kv(head)[0][lo:stored], v4.kv(head)[1][lo:stored]
        if len(K) == 0 and tail is None:
            if out[head].any() or (lse is not None and not np.all(lse[head] == -np.inf)):
                worst, first = np.inf, first or (what, head, "an empty member is exactly 0 with lse -inf")
            continue
        qe = k8.q_rows(q[head])                                                 # [G][D]
        s = (qe @ K.T) * SM
        delta = 3e-5 * float((np.abs(qe) @ np.abs(K).T).max(initial=0.0)) * SM
        vals = V
        if tail is not None:
            st = (q[head].astype(np.float64) @ tail[0][head].astype(np.float64)) * SM
            s = np.concatenate([s, st[:, None]], axis=1)
            vals = np.concatenate([V, tail[1][head].astype(np.float64)[None]])
        mx = s.max(axis=1)
        p = np.exp(s - mx[:, None])
        l = p.sum(axis=1)
        want, mag, wlse = (p @ vals) / l[:, None], (p @ np.abs(vals)) / l[:, None], mx + np.log(l)
        err, tol = np.abs(out[head].astype(np.float64) - want), (2e-3 + 2 * delta) * mag + 1e-6
        lerr, ltol = (np.zeros(len(qe)) if lse is None else np.abs(lse[head].astype(np.float64) - wlse)), 2e-3 + delta
        with np.errstate(invalid="ignore"):
            worst = max(worst, float(np.nan_to_num(err / tol, nan=np.inf).max()), float(np.nan_to_num(lerr / ltol, nan=np.inf).max()))
        if not np.all(err <= tol):
            first = first or (what, head, "out", float(np.nan_to_num(err / tol, nan=np.inf).max()))
        if not np.all(lerr <= ltol):
            first = first or (what, head, "lse", float(np.nanmax(lerr)), ltol)
    return worst, first


class Members:
    """a batch under one window: per member its own request (a pair of allocations) with its hostile content, queries and references"""

    def __init__(self, conn, lengths, window, seed, needle=False, g=G):
        torch = torch_mod()
        self.conn, self.window, self.needle, self.g = conn, window, needle, g
        self.lengths = np.asarray(lengths, np.int64)
        self.n = len(lengths)
        self.spans = [span(int(n), window) for n in lengths]
        self.pos_end = (self.lengths & ~1).astype(np.uint32)
        self.q_pos = (np.maximum(self.lengths, 1) - 1).astype(np.uint32)
        self.rids, self.failures, keep = [], [], []
        for lo, stored in self.spans:
            rows = content(lo, stored, needle).reshape(L, 2, T, H, D)              # [layer][kind][position][head][dim]
            rid = next(_rids)
            conn.add_request(rid)
            keep += conn.write_prefill(rid, torch.from_numpy(np.ascontiguousarray(rows[:, 0])).cuda(), torch.from_numpy(np.ascontiguousarray(rows[:, 1])).cuda())
            self.rids.append(rid)
        reqs = [conn.requests[r] for r in self.rids]
        self.kh = np.asarray([r.k_handle for r in reqs], np.uint64)
        self.vh = np.asarray([r.v_handle for r in reqs], np.uint64)
        rng = np.random.default_rng(seed)
        self.qh = (rng.standard_normal((L, self.n, H, g, D)) * 1.5).astype(np.float16)
        if needle:
            self.qh = (needle_dirs()[:, None, :, None, :] + 0.3 * rng.standard_normal((L, self.n, H, g, D))).astype(np.float16)
        self.q = torch.from_numpy(self.qh).cuda()
        torch.cuda.synchronize()
        del keep

    def args(self, layer, out, lse, stream, **change):
        a = dict(k_handles=self.kh, v_handles=self.vh, layer=layer, d_q_f16=self.q[min(layer, L - 1)].data_ptr(), g=self.g, pos_end=self.pos_end, q_pos=self.q_pos,
                 window=self.window, sm_scale=SM, d_out=out.data_ptr(), d_lse=lse.data_ptr(), stream=stream.cuda_stream)
        a.update(change)
        return a

    def fresh(self):
        torch = torch_mod()
        out = torch.full((self.n, H, self.g, D), PATTERN, dtype=torch.int32, device="cuda")
        lse = torch.full((self.n, H, self.g), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return out, lse

    def entry(self, layer, **change):
        """speckv_ext_attend_kv_batch_window itself: (out [n][H][g][D], lse [n][H][g]) as fp32 numpy"""
        torch = torch_mod()
        out, lse = self.fresh()
        st = torch.cuda.Stream()
        self.conn.lib.attend_kv_batch_window(**self.args(layer, out, lse, st, **change))
        st.synchronize()
        return out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)

    def plain(self, layer):
        """speckv_ext_attend_kv_batch over the same handles, query and pos_end"""
        torch = torch_mod()
        out, lse = self.fresh()
        st = torch.cuda.Stream()
        a = self.args(layer, out, lse, st)
        del a["q_pos"], a["window"]
        self.conn.lib.attend_kv_batch(**a)
        st.synchronize()
        return out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)

    def check(self, oracle, out, lse, layer, what):
        """every (member, head, row) of one layer; failures are collected, the worst err / tol returned"""
        worst = 0.0
        if (out.view(np.uint32) == PATTERN).any() or (lse.view(np.uint32) == PATTERN).any():
            self.failures.append((what, layer, "rows keep the fill pattern"))
        if not np.isfinite(out).all() or np.isnan(lse).any() or (lse == np.inf).any():
            self.failures.append((what, layer, "out / lse not finite"))
        for i, (lo, stored) in enumerate(self.spans):
            pair = (checker(oracle, FP8, layer, lo, stored, self.needle), checker(oracle, MX4, layer, lo, stored, self.needle))
            w, first = member_check(pair, out[i], lse[i], self.qh[layer, i], min(lo, stored), stored, what + (layer, int(self.lengths[i])))
            worst = max(worst, w)
            if first is not None:
                self.failures.append(first)
        return worst

    def free(self):
        for rid in self.rids:
            self.conn.free_request(rid)
        self.rids = []


# ----------------------------------------------------------------------------- 1. the entry over A and B under every window
@pytest.mark.parametrize("window", WINDOWS)
def test_lengths_under_windows(oracle, window):
    """batches A and B, both layers, hostile rows outside every member's window; W = 300 cuts nobody: the bits of speckv_ext_attend_kv_batch"""
    torch = torch_mod()
    overall, failures = 0.0, []
    with _pool(torch) as (lib, conn):
        for name, lengths in (("A", LENGTHS_A), ("B", LENGTHS_B)):
            m = Members(conn, lengths, window, 9600 + FP8)
            try:
                for layer in range(L):
                    out, lse = m.entry(layer)
                    overall = max(overall, m.check(oracle, out, lse, layer, (window, name)))
                    if window == 300:
                        po, pl = m.plain(layer)
                        assert np.array_equal(po.view(np.uint32), out.view(np.uint32)) and np.array_equal(pl.view(np.uint32), lse.view(np.uint32)), (name, layer)
            finally:
                m.free()
            failures += m.failures
    print(f"k8v4 decode window W = {window}: worst err / tol {overall:.3f}, {len(failures)} checks failed")
    assert not failures, failures[:6]


@pytest.mark.parametrize("g", [1, 16])
def test_one_and_sixteen_query_rows(oracle, g):
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS_B, 33, 9610 + g, g=g)
        try:
            worst = max(m.check(oracle, *m.entry(layer), layer, (33, "B", g)) for layer in range(L))
        finally:
            m.free()
    print(f"k8v4 decode window g = {g}: worst err / tol {worst:.3f}, {len(m.failures)} checks failed")
    assert not m.failures, m.failures[:6]


# ----------------------------------------------------------------------------- 2. a needle at the bound
def test_needle_at_the_window_bound(oracle):
    """position lo takes nearly all the weight and lo - 1 is hostile: a mask one position off in either direction is of the order of the
    output (lo = 65, 98, 32, 222, 31, 223 under W = 33; the scheme of tests/test_gpu_decode_window.py)"""
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        m = Members(conn, NEEDLE_LENGTHS, NEEDLE_W, 9650 + FP8, needle=True)
        try:
            worst = max(m.check(oracle, *m.entry(layer), layer, (NEEDLE_W, "needle")) for layer in range(L))
        finally:
            m.free()
    print(f"k8v4 decode window needle: worst err / tol {worst:.3f}, {len(m.failures)} checks failed")
    assert not m.failures, m.failures[:6]


# ----------------------------------------------------------------------------- 3. pieces and the merge under a window
@pytest.mark.parametrize("as_given", [0, 1])
def test_pieces_and_the_merge_under_a_window(oracle, as_given):
    """attend_tiles_per_split = 1: a windowed member of 2 .. 5 tiles is cut into as many pieces (partials and the merge; tile 0's mask lies in
    piece 0 only, guarded by the absolute tile index), dispatched by length rows-first and in the order given.  The engine's own rules
    (tests/_rules.py decide over the WINDOWED page counts) say so first."""
    torch = torch_mod()
    lengths = LENGTHS_B + LENGTHS_A
    overall, failures = 0.0, []
    with _pool(torch) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", 1)
            set_tuning("attend_order_as_given", as_given)
            for window in (33, 100):
                pages = np.asarray([SpeckvKVConnector.decode_window_range(int(n), window)[2] for n in lengths])
                tiles = (pages + 15) // 16
                d = decide(load_rules(), FP8, "batch", pages, _cus(), tuning=(1, as_given) + DEFAULT_TUNING[2:])
                assert d["fits"] == 1 and d["tps"] == 1 and d["max_splits"] == int(tiles.max()) >= 2 and not d["table"] and not d["striped"], d
                assert [int(x) for x in d["pieces"][:, 1]] == [int(t) for t in tiles]
                assert d["by_length"] == (0 if as_given else 1)
                m = Members(conn, lengths, window, 9620 + window)
                try:
                    for layer in range(L):
                        overall = max(overall, m.check(oracle, *m.entry(layer), layer, (window, "pieces", as_given)))
                finally:
                    m.free()
                failures += m.failures
        finally:
            set_tuning("attend_tiles_per_split", 0)
            set_tuning("attend_order_as_given", 0)
    print(f"k8v4 decode window pieces of one tile, order as given {as_given}: worst err / tol {overall:.3f}, {len(failures)} checks failed")
    assert not failures, failures[:6]


# ----------------------------------------------------------------------------- 4. no window: the launches of the entry without one
def test_window_0_and_a_window_that_cuts_nobody_are_the_plain_entry_bit_for_bit():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS_B + LENGTHS_A, 300, 9630)
        try:
            for layer in range(L):
                po, pl = m.plain(layer)
                assert not (po.view(np.uint32) == PATTERN).any()
                for how in (dict(window=0), dict(window=0, q_pos=None), dict(window=300), dict(window=256), dict(window=4096)):
                    out, lse = m.entry(layer, **how)
                    assert np.array_equal(out.view(np.uint32), po.view(np.uint32)) and np.array_equal(lse.view(np.uint32), pl.view(np.uint32)), (layer, how)
            # ... and a window that cuts one member changes that member's rows and no other member's bits
            out, lse = m.entry(0, window=255)
            po, pl = m.plain(0)
            assert np.array_equal(out[1:].view(np.uint32), po[1:].view(np.uint32)) and np.array_equal(lse[1:].view(np.uint32), pl[1:].view(np.uint32))
            assert not np.array_equal(lse[0], pl[0]) and np.all(lse[0] <= pl[0])
        finally:
            m.free()


# ----------------------------------------------------------------------------- 5. the connector route
def test_a_walk_through_the_connector_on_a_local_and_a_global_layer(oracle):
    """two requests, write_prefill(61) and (7), then eight rounds of (attend at the local layer 0 under W = 33 and at the global layer 1,
    commit of one position): lengths 61 .. 68 and 7 .. 14, odd (one batch call and one fold of the fp16 tails) and even in turn; lo of the
    first request walks 28 .. 35 across the tile bound at 32, its stored count across the tile bound at 64; every attend against float64
    over a shadow of the committed rows"""
    torch = torch_mod()
    rng = np.random.default_rng(6160)
    rows = lambda *shape: rng.standard_normal(shape).astype(np.float16)
    g, W, rids = 4, 33, [7, 9]
    shadow = [[rows(L, n, H, D), rows(L, n, H, D)] for n in (61, 7)]
    worst, failures = 0.0, []
    with _pool(torch) as (lib, conn):
        keep = []
        for rid, (k, v) in zip(rids, shadow):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
        counts = {"attend_kv_batch": 0, "attend_kv_batch_window": 0, "attend_fold_tail": 0}
        for name in counts:
            real = getattr(lib, name)
            setattr(lib, name, (lambda real, name: lambda *a, **k: (counts.__setitem__(name, counts[name] + 1), real(*a, **k))[1])(real, name))
        for step in range(8):
            lengths = [s[0].shape[1] for s in shadow]
            assert [conn.length(r) for r in rids] == lengths == [61 + step, 7 + step]
            q = rows(L, 2, H, g, D)
            before = dict(counts)
            outs = [conn.attend(layer, rids, torch.from_numpy(q[layer]).cuda(), SM, window=W if layer == 0 else None) for layer in range(L)]
            torch.cuda.synchronize()
            assert counts["attend_kv_batch_window"] == before["attend_kv_batch_window"] + 1 and counts["attend_kv_batch"] == before["attend_kv_batch"] + 1
            assert counts["attend_fold_tail"] == before["attend_fold_tail"] + (L if lengths[0] & 1 else 0)      # (both lengths have one parity)
            for layer in range(L):
                got = outs[layer].cpu().numpy()
                assert got.shape == (2, H, g, D) and got.dtype == np.float32
                for b, (sk, sv) in enumerate(shadow):
                    length = lengths[b]
                    even = length & ~1
                    lo = max(0, length - W) if layer == 0 else 0
                    region = _region(sk[layer, :even], sv[layer, :even], T)
                    pair = (HeadChecker(oracle, FP8, region, T), HeadChecker(oracle, MX4, region, T))
                    tail = (sk[layer, -1], sv[layer, -1]) if length & 1 else None
                    w, first = member_check(pair, got[b], None, q[layer, b], min(lo, even), even, ("walk", step, layer, length), tail)
                    worst = max(worst, w)
                    if first is not None:
                        failures.append(first)
            kn, vn = rows(2, 1, L, H, D), rows(2, 1, L, H, D)
            keep += conn.commit(rids, torch.from_numpy(kn).cuda(), torch.from_numpy(vn).cuda(), [1, 1])
            for b in range(2):
                shadow[b][0] = np.concatenate([shadow[b][0], kn[b].transpose(1, 0, 2, 3)], axis=1)
                shadow[b][1] = np.concatenate([shadow[b][1], vn[b].transpose(1, 0, 2, 3)], axis=1)
        torch.cuda.synchronize()
        del keep
    print(f"k8v4 decode window connector walk: worst err / tol {worst:.3f}, {len(failures)} checks failed")
    assert not failures, failures[:6]


def test_the_connector_with_tails_and_a_request_of_length_0(oracle):
    """SpeckvSplitKVConnector.attend(window=W) over hostile content with odd lengths (the tails folded) and a request without a position:
    batch A's odd members under W = 33 and W = 1 (the pool part empty, the tail alone), layer 0 local and layer 1 global in one step"""
    torch = torch_mod()
    rng = np.random.default_rng(6170)
    lengths = [33, 65, 131, 255, 0, 98, 1]
    failures, worst = [], 0.0
    with _pool(torch) as (lib, conn):
        for W in (33, 1):
            keep, rids, data = [], [], []
            for n in lengths:
                lo, stored = span(n, W)
                rws = content(lo, stored).reshape(L, 2, T, H, D)[:, :, :n]
                k, v = np.ascontiguousarray(rws[:, 0]), np.ascontiguousarray(rws[:, 1])
                if n & 1:                                                      # the tail is an ordinary row (it is always inside the window)
                    k[:, -1], v[:, -1] = rng.standard_normal((L, H, D)).astype(np.float16), rng.standard_normal((L, H, D)).astype(np.float16)
                rid = next(_rids)
                conn.add_request(rid)
                if n:
                    keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
                rids.append(rid)
                data.append((k, v))
            q = (rng.standard_normal((L, len(lengths), H, G, D)) * 1.5).astype(np.float16)
            outs = [conn.attend(layer, rids, torch.from_numpy(q[layer]).cuda(), SM, window=W if layer == 0 else None).cpu().numpy() for layer in range(L)]
            torch.cuda.synchronize()
            for layer in range(L):
                for b, n in enumerate(lengths):
                    lo, stored = span(n, W if layer == 0 else 0)
                    k, v = data[b]
                    if layer == 0:
                        pair = (checker(oracle, FP8, 0, *span(n, W)), checker(oracle, MX4, 0, *span(n, W)))
                    else:                                                      # the global layer sees the hostile rows below the local layer's lo: its own reference
                        region = _region(k[1, :stored], v[1, :stored], T)
                        pair = (HeadChecker(oracle, FP8, region, T), HeadChecker(oracle, MX4, region, T))
                    tail = (k[layer, -1], v[layer, -1]) if n & 1 else None
                    w, first = member_check(pair, outs[layer][b], None, q[layer, b], min(lo, stored), stored, ("tails", W, layer, n), tail)
                    worst = max(worst, w)
                    if first is not None:
                        failures.append(first)
            for rid in rids:
                conn.free_request(rid)
            del keep
    print(f"k8v4 decode window connector with tails: worst err / tol {worst:.3f}, {len(failures)} checks failed")
    assert not failures, failures[:6]


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS_B, 33, 9640)
        try:
            with_at = lambda a, b, x: np.concatenate([a[:b], np.asarray([x], a.dtype), a[b + 1:]])

            def refused(**change):
                """the status of the refused call; out and lse keep the fill pattern"""
                out, lse = m.fresh()
                st = torch.cuda.Stream()
                with pytest.raises(SpeckvError) as e:
                    lib.attend_kv_batch_window(**m.args(change.pop("layer", 1), out, lse, st, **change))
                st.synchronize(); torch.cuda.synchronize()
                assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all()), (list(change), "a refused call wrote something")
                return e.value.status
            invalid = {
                "q_pos two below pos_end": dict(q_pos=with_at(m.q_pos, 0, 254)), "q_pos beyond pos_end": dict(q_pos=with_at(m.q_pos, 2, 65)),
                "q_pos 1 with pos_end 0": dict(pos_end=with_at(m.pos_end, 3, 0), q_pos=with_at(m.q_pos, 3, 1)),
                "NULL q_pos with a window": dict(q_pos=None),
                "swapped handle arrays": dict(k_handles=m.vh, v_handles=m.kh),
                "a K allocation of MXFP4": dict(k_handles=with_at(m.kh, 2, m.vh[3])), "a V allocation of FP8": dict(v_handles=with_at(m.vh, 2, m.kh[3])),
                "an odd pos_end": dict(pos_end=with_at(m.pos_end, 4, 97), q_pos=with_at(m.q_pos, 4, 97)),
                "pos_end beyond the layout": dict(pos_end=with_at(m.pos_end, 0, T + 2), q_pos=with_at(m.q_pos, 0, T + 1)),
                "g 0": dict(g=0), "g 17": dict(g=17),
                "NULL k_handles": dict(k_handles=None), "NULL v_handles": dict(v_handles=None), "NULL pos_end": dict(pos_end=None),
                "NULL q": dict(d_q_f16=0), "NULL out": dict(d_out=0), "a misaligned q": dict(d_q_f16=0x1008),
                "a layer beyond the regions": dict(layer=L), "a layer far beyond": dict(layer=1000),
            }
            for what, change in invalid.items():
                assert refused(**change) == -4, what                             # SPECKV_ERR_INVAL
            for change in (dict(k_handles=with_at(m.kh, 1, 0xDEAD)), dict(v_handles=with_at(m.vh, 1, 0xDEAD))):
                assert refused(**change) == -1                                   # SPECKV_ERR_GENERAL: an unknown handle
            # a capturing stream: refused, nothing written; the same arguments are taken once the stream captures no more
            st = torch.cuda.Stream()
            out, lse = m.fresh()
            args = m.args(1, out, lse, st)
            bump = torch.zeros(4, device="cuda")
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, st):
                with pytest.raises(SpeckvError) as e:
                    lib.attend_kv_batch_window(**args)
                assert e.value.status == -4
                bump.add_(1)
            del g
            torch.cuda.synchronize()
            assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all())
            lib.attend_kv_batch_window(**args)
            st.synchronize()
            assert not bool((out == PATTERN).any()) and not bool((lse == PATTERN).any())
            # nothing to do: no sequence, nothing written
            none = np.zeros(0, np.uint32)
            lib.attend_kv_batch_window(np.zeros(0, np.uint64), np.zeros(0, np.uint64), 1, m.q[1].data_ptr(), G, none, none, 33, SM, out.data_ptr(), lse.data_ptr(),
                                       st.cuda_stream)
            st.synchronize()
        finally:
            m.free()


# ----------------------------------------------------------------------------- 7. the example
def test_the_example_runs():
    """examples/k8v4_window_decode_example.py in this process, short: a local and a global layer, requests of odd and even lengths, every
    attend checked inside the example against torch over the dequantised window"""
    import importlib.util
    import os
    torch_mod()
    drop_engine()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "k8v4_window_decode_example.py")
    spec = importlib.util.spec_from_file_location("k8v4_window_decode_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(steps=3, verbose=False) == 3
