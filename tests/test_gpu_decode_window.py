"""-m gpu: decode attention under a SLIDING WINDOW -- speckv_ext_attend_batch_window, speckv_ext_attend_batch_plan_window and the planned
entries over its plans, SpeckvKVConnector.attend(window=...).

A member has `length` positions, the step's own included: stored = length & ~1 of them in the pool, an odd length its last one in the
caller's tail; its query sees [lo, length - 1], lo = max(0, length - W) (csrc/decode_window.hpp).  EVERY position of a member's
allocation below lo and at or behind stored is hostile, position by position (K x 200, V = +-1000: the magnitudes of
tests/test_gpu_hostile_ranges.py) -- an odd lo cuts a page, whose kept position then shares its FP8 page scale with a hostile row -- and
every (layer, head, query row) of out and lse is held to float64 attention over the oracle's dequantised records of exactly the
positions [lo, stored) (+ the tail where the entry takes one): tests/_gpu.py HeadChecker.want_rows(pos_begin=lo, tail=...), |err| <=
(2e-3 + 2 delta) sum p|v| + 1e-6, lse within 2e-3 + delta, a member without a position exactly 0 / -inf.  The reference runs per member
(lo differs), once per (format, content), shared by every entry and placement.  All seeds are fixed; the worst err / tol of every
case is printed before anything is asserted.

Layout: 8 kv heads x 128, G = 8, L = 2 layers (both hostile), allocations of T = 256 positions.  Two batches cover the lengths 1, 2,
33, 64, 65, 98, 131, 255, 256: A = 1, 2, 33, 64, 65, 98, 131, 255 (empty members: a length of 1, and every odd length under W = 1)
and B = 256, 255, 64, 33, 98, 131 (no empty member under W >= 2: the MXFP4 launch over layers x members with its in-kernel tail
fold).  W = 1, 2, 31, 32, 33, 64, 100, 300: lo odd and even, on and inside a tile, lo = 0, an empty pool with and without a tail, a
ragged last tile, the first and the last tile coinciding.  Entries: the batch entry (no tail), _planned (no tail), _planned_tail and
_planned_layers with both layers (the tails of the odd lengths).

Kernel body -> the case that runs it (batch = attend_batch_window where the window cuts a member, planned = the planned entries over a
windowed plan, always)

(FP8: the window has instances of its own, k_attend_fp8_linear<STRIPED, TABLE, CLS, WINDOW = true>; a launch that brings a skip array
 runs them, the instances without WINDOW run the window-less launches as before.  INT4_G32 / MXFP4: the existing instances.)
  k_attend_fp8_linear<false, false, false, true>   one pool, FP8: batch and planned (asserted: decide gives table = striped = 0)
  k_attend_fp8_linear<false, true, false, true>    striped3 and migrated, FP8: batch and planned (a windowed launch over a striped or
                                      migrated member reads the page tables; the register-staged table kernel: k_attend_fp8_dma<1> has no
                                      leading mask)
  k_attend_fp8_linear<true, false, false, true>    striped3, FP8, attend_fp8_table_regs = 1 (test_striped_bodies_on_request)
  k_attend_fp8_linear<false> (no WINDOW)           one pool, FP8: the batch entry under a window that cuts no member (W = 300; test_dispatch)
  k_attend_int4_wg8<2>                one pool, INT4_G32: batch and planned (asserted: wg8 = 1, the 16-wave form, for <= CUs members)
  k_attend_int4_wg8<1>                one pool, INT4_G32, more members than CUs (asserted: wg8 = 2): test_int4_one_run_workgroups
  k_attend_int4_wg<false, true>       striped3 and migrated, INT4_G32: batch and planned
  k_attend_int4_wg<true>              striped3, INT4_G32, attend_int4_striped_wg = 1 (test_striped_bodies_on_request)
  k_attend_mx4<0>                     one pool, MXFP4: the batch entry (a batch with an empty member: partials and the merge)
  k_attend_mx4<0, 2>                  one pool, MXFP4: planned (a room of one split); _planned_layers of batch B under W >= 2: the grid
                                      over layers x members with the tail folded in by the kernel
  k_attend_mx4<2>                     striped3 and migrated, MXFP4: batch and planned
  the class forms, k_attend_fp8_dma   never under a window: they have no mask for the head of a tile
No (format, placement) is skipped or refused."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests._gpu import D, H, HeadChecker, assert_same_float_bits, graph_capture, torch_mod
from tests._rules import decide, load_rules
from tests.test_gpu_hostile_ranges import FP8, INT4, MX4, NAMES, K_HOSTILE, V_HOSTILE, allocation, base, cus, drop_engine, engine, fresh, tuned

pytestmark = pytest.mark.gpu
G, L, T = 8, 2, 256
SM = 1.0 / np.sqrt(D)
LENGTHS_A = [1, 2, 33, 64, 65, 98, 131, 255]
LENGTHS_B = [256, 255, 64, 33, 98, 131]
WINDOWS = [1, 2, 31, 32, 33, 64, 100, 300]
NEEDLE_LENGTHS, NEEDLE_W = [98, 131, 65, 255, 64, 256], 33      # lo = 65, 98, 32, 222, 31, 223: odd and even, first and last of a tile
PLACEMENTS = ("one", "striped3", "migrated")

_checkers, _dirs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_engine()
    _checkers.clear()
    _contents.clear()


def span(length, window):
    """(lo, stored) of a member"""
    return (length - window if window and length > window else 0), length & ~1


def needle_dirs():
    """per (layer, head) a direction of +-1: position lo holds 1.2 x it as K, the queries of the needle case lie along it"""
    if "u" not in _dirs:
        _dirs["u"] = np.sign(np.random.default_rng(9700).standard_normal((L, H, D))).astype(np.float32)
    return _dirs["u"]


_contents = {}


def content(lo, stored, needle=False):
    """base(256) with every POSITION below lo and at or behind stored hostile in both layers; needle: position lo's K = 1.2 x the needle
    direction (its score 13.6 against scores of order 1: nearly all the weight), position lo - 1 hostile like the rest"""
    if (lo, stored, needle) not in _contents:
        if len(_contents) >= 64:
            _contents.clear()
        _contents[(lo, stored, needle)] = _content(lo, stored, needle)
    return _contents[(lo, stored, needle)]


def _content(lo, stored, needle):
    x = base(T).copy()
    rows = x.reshape(L, 2, T, H * D)                        # [layer][kind][position][head x dim]: a page holds two positions
    out = np.ones(T, bool)
    out[lo:stored] = False
    rows[:, 0, out] = (rows[:, 0, out].astype(np.float32) * K_HOSTILE).astype(np.float16)
    rows[:, 1, out] = (np.sign(rows[:, 1, out].astype(np.float32)) * V_HOSTILE).astype(np.float16)
    if needle and lo < stored:
        rows[:, 0, lo] = (1.2 * needle_dirs()).reshape(L, H * D).astype(np.float16)
    assert np.isfinite(x.astype(np.float32)).all()
    return x


def checker(oracle, scheme, layer, lo, stored, needle=False):
    """float64 attention over a member's own content (a page cut by lo is quantised together with its hostile row)"""
    key = (scheme, layer, lo, stored, needle)
    if key not in _checkers:
        _checkers[key] = HeadChecker(oracle, scheme, content(lo, stored, needle)[layer * T:(layer + 1) * T], T)
    return _checkers[key]


class Members:
    """a batch under one window: allocations with their hostile content, queries, the tails of the odd lengths, and the references"""

    def __init__(self, lib, scheme, lengths, window, seed, migrate_member=None, needle=False):
        torch = torch_mod()
        self.lib, self.scheme, self.window, self.needle = lib, scheme, window, needle
        self.lengths = np.asarray(lengths, np.int64)
        self.n = len(lengths)
        self.spans = [span(int(n), window) for n in lengths]
        self.pos_end = (self.lengths & ~1).astype(np.uint32)
        self.q_pos = np.maximum(self.lengths, 1).astype(np.uint32) - 1
        self.handles, self.failures, self.refs = [], [], {}
        for i, (lo, stored) in enumerate(self.spans):
            self.handles.append(allocation(lib, scheme, T, content(lo, stored, needle), migrate=i == migrate_member))
        rng = np.random.default_rng(seed)
        self.qh = (rng.standard_normal((L, self.n, H, G, D)) * 1.5).astype(np.float16)
        if needle:
            self.qh = (needle_dirs()[:, None, :, None, :] + 0.3 * rng.standard_normal((L, self.n, H, G, D))).astype(np.float16)
        self.q = torch.from_numpy(self.qh).cuda()
        self.odd = [i for i, n in enumerate(lengths) if n & 1]
        inv = np.full(self.n, -1, np.int32)
        inv[self.odd] = np.arange(len(self.odd))
        self.kt = (rng.standard_normal((len(self.odd), L, H, D)) * 1.5).astype(np.float16)
        self.vt = rng.standard_normal((len(self.odd), L, H, D)).astype(np.float16)
        self.d_kt, self.d_vt = torch.from_numpy(self.kt).cuda(), torch.from_numpy(self.vt).cuda()
        self.d_rows, self.d_idx = torch.from_numpy(np.asarray(self.odd, np.int32)).cuda(), torch.from_numpy(inv).cuda()
        self.inv = inv
        torch.cuda.synchronize()

    def tail_args(self):
        return dict(n_tail=len(self.odd), d_tail_rows=self.d_rows.data_ptr(), d_tail_idx=self.d_idx.data_ptr(), d_k_tail=self.d_kt.data_ptr(),
                    d_v_tail=self.d_vt.data_ptr(), tail_stride_elems=L * H * D)

    def check(self, oracle, out, lse, layer, what, tails, members=None):
        """rows [n][H][G][D] / [n][H][G] of one layer against the per-member reference; tails: the entry folded the odd members' tails in"""
        worst, first = [], None
        for i in (range(self.n) if members is None else members):
            lo, stored = self.spans[i]
            hc = checker(oracle, self.scheme, layer, lo, stored, self.needle)
            has_tail = tails and self.inv[i] >= 0
            for head in range(H):
                tl = (self.kt[self.inv[i], layer, head][None], self.vt[self.inv[i], layer, head][None]) if has_tail else None
                try:
                    hc.check_rows(out[i, head][None], lse[i, head][None], self.qh[layer, i, head][None], head, [max(0, stored - lo)], SM,
                                  what + (layer, int(self.lengths[i]), head), tl, pos_begin=lo, worst=worst)
                except AssertionError as ex:
                    first = first or ex.args[0]
            if stored <= lo and not has_tail and not np.all(lse[i] == -np.inf):
                first = first or (what, layer, int(self.lengths[i]), "a member without a position: lse is not -inf")
        if not np.isfinite(out).all() or np.isnan(lse).any() or (lse == np.inf).any():
            first = first or (what, layer, "out / lse not finite")
        if first is not None:
            self.failures.append((first, f"worst err/tol {max(worst):.3f}"))
        return max(worst)

    def free(self):
        for h in self.handles:
            self.lib.free(h)
        self.handles = []


def run_entries(oracle, m, what):
    """the batch entry, _planned, _planned_tail and _planned_layers over the members `m`, every row checked; the worst err / tol"""
    torch = torch_mod()
    lib, scheme, n, W = m.lib, m.scheme, m.n, m.window
    overall = 0.0
    for layer in range(L):
        out, lse = fresh((n, H), torch)
        lib.attend_batch_window(scheme, m.handles, layer, m.q[layer].data_ptr(), G, m.pos_end, m.q_pos, W, SM, out.data_ptr(), lse.data_ptr())
        torch.cuda.synchronize()
        overall = max(overall, m.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), layer, what + ("batch",), tails=False))
    st = torch.cuda.Stream()
    plan_bytes = lib.attend_plan_window_bytes(n)
    plan = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib.attend_batch_plan_window(m.handles, m.pos_end, m.q_pos, W, T, plan.data_ptr(), plan_bytes, st.cuda_stream)
    for layer in range(L):
        out, lse = fresh((n, H), torch)
        torch.cuda.synchronize()
        lib.attend_planned(scheme, plan.data_ptr(), n, layer, m.q[layer].data_ptr(), G, T, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
        st.synchronize()
        overall = max(overall, m.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), layer, what + ("planned",), tails=False))
        if m.odd:
            out, lse = fresh((n, H), torch)
            torch.cuda.synchronize()
            t = m.tail_args()
            lib.attend_planned_tail(scheme, plan.data_ptr(), n, layer, m.q[layer].data_ptr(), G, T, SM, out.data_ptr(), lse.data_ptr(), t["n_tail"],
                                    t["d_tail_rows"], t["d_tail_idx"], t["d_k_tail"], t["d_v_tail"], t["tail_stride_elems"], st.cuda_stream)
            st.synchronize()
            overall = max(overall, m.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), layer, what + ("planned_tail",), tails=True))
    out, lse = fresh((L, n, H), torch)
    torch.cuda.synchronize()
    lib.attend_planned_layers(scheme, plan.data_ptr(), n, 0, L, m.q.data_ptr(), G, T, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream, **m.tail_args())
    st.synchronize()
    o, l = out.cpu().numpy(), lse.cpu().numpy()
    for layer in range(L):
        overall = max(overall, m.check(oracle, o[layer], l[layer], layer, what + ("planned_layers",), tails=True))
    return overall


def assert_one_pool_form(scheme, lengths, window):
    """where tests/_rules.py decide can tell: pools in single runs keep the linear bodies under a window (the module's table)"""
    pages = np.asarray([SpeckvKVConnector.decode_window_range(int(n), window)[2] for n in lengths])
    d = decide(load_rules(), scheme, "plan", pages, cus(), max_pos_end=T)
    assert (d["table"], d["striped"], d["by_class"]) == (0, 0, 0) and d["fits"] == 1, d
    assert d["wg8"] == (1 if scheme == INT4 else 0), d


CASES = [(p, s, w) for p in PLACEMENTS for s in (FP8, INT4, MX4) for w in WINDOWS]


@pytest.mark.parametrize("placement,scheme,window", CASES, ids=[f"{p}-{NAMES[s]}-W{w}" for p, s, w in CASES])
def test_lengths_under_windows(oracle, placement, scheme, window):
    """batches A and B under one window through the batch entry and the three planned entries, hostile rows outside every member's window"""
    lib = engine(placement)
    overall, failures = 0.0, []
    for name, lengths in (("A", LENGTHS_A), ("B", LENGTHS_B)):
        if placement == "one":
            assert_one_pool_form(scheme, lengths, window)
        m = Members(lib, scheme, lengths, window, 9600 + scheme, migrate_member=lengths.index(64) if placement == "migrated" else None)      # (its page 17: positions 34, 35)
        try:
            overall = max(overall, run_entries(oracle, m, (placement, NAMES[scheme], window, name)))
        finally:
            m.free()
        failures += m.failures
    print(f"decode window {placement}-{NAMES[scheme]} W = {window}: worst err/tol {overall:.3f}, {len(failures)} rows' checks failed")
    assert not failures, failures[:6]


NEEDLES = [(p, s) for s in (FP8, INT4, MX4) for p in PLACEMENTS]


@pytest.mark.parametrize("placement,scheme", NEEDLES, ids=[f"{p}-{NAMES[s]}" for p, s in NEEDLES])
def test_needle_at_the_window_bound(oracle, placement, scheme):
    """position lo takes nearly all the weight and lo - 1 is hostile: a mask one position off in either direction is of the order of
    the output (lo = 65, 98, 32, 222, 31, 223 under W = 33)"""
    lib = engine(placement)
    m = Members(lib, scheme, NEEDLE_LENGTHS, NEEDLE_W, 9650 + scheme, migrate_member=NEEDLE_LENGTHS.index(64) if placement == "migrated" else None, needle=True)
    try:
        worst = run_entries(oracle, m, (placement, NAMES[scheme], NEEDLE_W, "needle"))
    finally:
        m.free()
    print(f"decode window needle {placement}-{NAMES[scheme]}: worst err/tol {worst:.3f}, {len(m.failures)} rows' checks failed")
    assert not m.failures, m.failures[:6]


STRIPED_ON_REQUEST = [(FP8, (("attend_fp8_table_regs", 1),), (0, 0, 1, 0, 0)), (INT4, (("attend_int4_striped_wg", 1),), (0, 0, 0, 0, 1))]


@pytest.mark.parametrize("scheme,tuning,rule_tuning", STRIPED_ON_REQUEST, ids=["fp8-table_regs", "int4-striped_wg"])
def test_striped_bodies_on_request(oracle, scheme, tuning, rule_tuning):
    """k_attend_fp8_linear<true> and k_attend_int4_wg<true>: the striped bodies a tuning key selects keep their form under a window"""
    lib = engine("striped3")
    pages = np.asarray([SpeckvKVConnector.decode_window_range(int(n), 33)[2] for n in LENGTHS_B])
    d = decide(load_rules(), scheme, "plan", pages, cus(), stripe_n=3, tuning=rule_tuning, max_pos_end=T)
    assert (d["table"], d["striped"], d["by_class"]) == (0, 1, 0), d
    with tuned(tuning):
        m = Members(lib, scheme, LENGTHS_B, 33, 9660 + scheme)
        try:
            worst = run_entries(oracle, m, ("striped3", NAMES[scheme], 33, tuning[0][0]))
        finally:
            m.free()
    print(f"decode window striped on request {NAMES[scheme]}: worst err/tol {worst:.3f}")
    assert not m.failures, m.failures[:6]


def test_int4_one_run_workgroups(oracle):
    """k_attend_int4_wg8<1>: more members than CUs take the one-run (8-wave) workgroups.  CUs + 4 members of the lengths of batch B under
    W = 33, hostile outside every window; layer 0 through the batch entry and the planned entry."""
    torch = torch_mod()
    lib = engine("one")
    n = cus() + 4
    lengths = [LENGTHS_B[i % len(LENGTHS_B)] for i in range(n)]
    pages = np.asarray([SpeckvKVConnector.decode_window_range(x, 33)[2] for x in lengths])
    for entry in ("batch", "plan"):
        d = decide(load_rules(), INT4, entry, pages, cus(), max_pos_end=T)
        assert (d["table"], d["striped"], d["wg8"], d["fits"]) == (0, 0, 2, 1), (entry, d)
    m = Members(lib, INT4, lengths, 33, 9670)
    try:
        out, lse = fresh((n, H), torch)
        lib.attend_batch_window(INT4, m.handles, 0, m.q[0].data_ptr(), G, m.pos_end, m.q_pos, 33, SM, out.data_ptr(), lse.data_ptr())
        torch.cuda.synchronize()
        worst = m.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), 0, ("one", "int4", 33, "wg8 = 2", "batch"), tails=False)
        st = torch.cuda.Stream()
        nbytes = lib.attend_plan_window_bytes(n)
        plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        out, lse = fresh((n, H), torch)
        torch.cuda.synchronize()
        lib.attend_batch_plan_window(m.handles, m.pos_end, m.q_pos, 33, T, plan.data_ptr(), nbytes, st.cuda_stream)
        lib.attend_planned(INT4, plan.data_ptr(), n, 0, m.q[0].data_ptr(), G, T, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
        st.synchronize()
        worst = max(worst, m.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), 0, ("one", "int4", 33, "wg8 = 2", "planned"), tails=False))
    finally:
        m.free()
    print(f"decode window int4 one-run workgroups, {n} members: worst err/tol {worst:.3f}, {len(m.failures)} rows' checks failed")
    assert not m.failures, m.failures[:6]


# ----------------------------------------------------------------------------- dispatch
def plain_members(lib, scheme, lengths, seed):
    """members over ordinary content (nothing hostile): what the window cuts is an ordinary row, the results with and without it compare"""
    m = Members.__new__(Members)
    torch = torch_mod()
    m.lib, m.scheme, m.n = lib, scheme, len(lengths)
    m.lengths = np.asarray(lengths, np.int64)
    m.pos_end = (m.lengths & ~1).astype(np.uint32)
    m.q_pos = np.maximum(m.lengths, 1).astype(np.uint32) - 1
    m.handles = [allocation(lib, scheme, T, base(T)) for _ in lengths]
    m.qh = (np.random.default_rng(seed).standard_normal((L, m.n, H, G, D)) * 1.5).astype(np.float16)
    m.q = torch.from_numpy(m.qh).cuda()
    torch.cuda.synchronize()
    return m


def planned(lib, scheme, m, window, st, lengths=None):
    """both layers through attend_planned over a fresh plan (window 0: attend_batch_plan): out, lse as numpy"""
    torch = torch_mod()
    n = m.n
    pos_end, q_pos = (m.pos_end, m.q_pos) if lengths is None else ((np.asarray(lengths) & ~1).astype(np.uint32), (np.asarray(lengths) - 1).astype(np.uint32))
    nbytes = lib.attend_plan_window_bytes(n)
    plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out, lse = fresh((L, n, H), torch)
    torch.cuda.synchronize()
    if window:
        lib.attend_batch_plan_window(m.handles, pos_end, q_pos, window, T, plan.data_ptr(), nbytes, st.cuda_stream)
    else:
        lib.attend_batch_plan(m.handles, pos_end, T, plan.data_ptr(), lib.attend_plan_bytes(n), st.cuda_stream)
    for layer in range(L):
        lib.attend_planned(scheme, plan.data_ptr(), n, layer, m.q[layer].data_ptr(), G, T, SM, out[layer].data_ptr(), lse[layer].data_ptr(), st.cuda_stream)
    st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


@pytest.mark.parametrize("scheme", [FP8, INT4, MX4], ids=[NAMES[s] for s in (FP8, INT4, MX4)])
def test_dispatch(scheme):
    """A window >= every length: the bits of the unwindowed planned call (and of the unwindowed batch entry).  A window one less than
    the longest member's length: that member's rows change, no other member's bits do."""
    torch = torch_mod()
    lib = engine("one")
    lengths = [256, 200, 130, 64, 98, 34]
    m = plain_members(lib, scheme, lengths, 9800 + scheme)
    entry = {FP8: lib.attend_fp8_batch, INT4: lib.attend_int4_batch, MX4: lib.attend_mx4_batch}[scheme]
    try:
        st = torch.cuda.Stream()
        o0, l0 = planned(lib, scheme, m, 0, st)
        for w in (256, 300, 4096):
            o1, l1 = planned(lib, scheme, m, w, st)
            assert_same_float_bits(o1, o0, f"planned, W = {w} >= every length")
            assert_same_float_bits(l1, l0, f"planned lse, W = {w}")
        ob, lb = fresh((m.n, H), torch)
        entry(m.handles, 0, m.q[0].data_ptr(), G, m.pos_end, SM, ob.data_ptr(), lb.data_ptr())
        torch.cuda.synchronize()
        for w, q_pos in ((256, m.q_pos), (0, None)):
            ow, lw = fresh((m.n, H), torch)
            lib.attend_batch_window(scheme, m.handles, 0, m.q[0].data_ptr(), G, m.pos_end, q_pos, w, SM, ow.data_ptr(), lw.data_ptr())
            torch.cuda.synchronize()
            assert_same_float_bits(ow.cpu().numpy(), ob.cpu().numpy(), f"batch entry, W = {w}")
            assert_same_float_bits(lw.cpu().numpy(), lb.cpu().numpy(), f"batch entry lse, W = {w}")
        o2, l2 = planned(lib, scheme, m, 255, st)
        assert_same_float_bits(o2[:, 1:], o0[:, 1:], "planned, W = 255: the members it does not cut")
        assert_same_float_bits(l2[:, 1:], l0[:, 1:], "planned lse, W = 255: the members it does not cut")
        for layer in range(L):
            assert not np.array_equal(l2[layer, 0], l0[layer, 0]) and not np.array_equal(o2[layer, 0], o0[layer, 0]), "W = 255 left the longest member as it was"
            # (a position less never raises a row's log-sum-exp; where its weight is below the sum's last bit the row keeps its bits)
            assert np.all(l2[layer, 0] <= l0[layer, 0]) and np.mean(l2[layer, 0] < l0[layer, 0]) > 0.5, "a position less must lower the log-sum-exp"
    finally:
        m.free()


def test_refusals():
    """a q_pos outside {pos_end - 1, pos_end}, a short buffer, a missing q_pos: SPECKV_ERR_INVAL, nothing written"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    torch = torch_mod()
    lib = engine("one")
    m = plain_members(lib, FP8, [64, 33], 9850)
    try:
        st = torch.cuda.Stream()
        nbytes = lib.attend_plan_window_bytes(2)
        plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for pos_end, q_pos, nb in (([64, 32], [62, 32], nbytes), ([64, 32], [63, 34], nbytes), ([64, 32], [63, 32], lib.attend_plan_bytes(2))):
            with pytest.raises(SpeckvError) as e:
                lib.attend_batch_plan_window(m.handles, pos_end, q_pos, 16, T, plan.data_ptr(), nb, st.cuda_stream)
            assert e.value.status == -4
        assert not plan.any()
        # a capturing stream in the plan call: the plan is what changes between replays, it stays outside the graph
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            with pytest.raises(SpeckvError) as e:
                lib.attend_batch_plan_window(m.handles, [64, 32], [63, 32], 16, T, plan.data_ptr(), nbytes, st.cuda_stream)
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert not plan.any()
        del g
        out, lse = fresh((2, H), torch)
        for q_pos in ([62, 32], None):
            with pytest.raises(SpeckvError) as e:
                lib.attend_batch_window(FP8, m.handles, 0, m.q[0].data_ptr(), G, [64, 32], q_pos, 16, SM, out.data_ptr(), lse.data_ptr())
            assert e.value.status == -4
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    finally:
        m.free()


# ----------------------------------------------------------------------------- graph
@pytest.mark.parametrize("scheme", [FP8, INT4, MX4], ids=[NAMES[s] for s in (FP8, INT4, MX4)])
def test_captured_windowed_launches_replay_over_new_plans(scheme):
    """the planned layer calls over a windowed plan, captured once, replayed after speckv_ext_attend_batch_plan_window with every length
    advanced by 1 and then by 2 more (a parity and a tile boundary of lo and of stored crossed inside the bucket): each replay equals the
    eager call over the same plan bit for bit"""
    torch = torch_mod()
    lib = engine("one")
    W = 40
    lengths = np.array([63, 71, 95, 130, 200, 31, 253])          # lo = 23, 31, 55, 90, 160, 0, 213; 71: lo crosses 32; 63: stored crosses 64
    m = plain_members(lib, scheme, lengths, 9900 + scheme)
    n = m.n
    try:
        st = torch.cuda.Stream()
        nbytes = lib.attend_plan_window_bytes(n)
        plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

        def do_plan(lens):
            lib.attend_batch_plan_window(m.handles, (lens & ~1).astype(np.uint32), (lens - 1).astype(np.uint32), W, T, plan.data_ptr(), nbytes, st.cuda_stream)

        def launches(out, lse):
            for layer in range(L):
                lib.attend_planned(scheme, plan.data_ptr(), n, layer, m.q[layer].data_ptr(), G, T, SM, out[layer].data_ptr(), lse[layer].data_ptr(), st.cuda_stream)

        g_out, g_lse = fresh((L, n, H), torch)
        torch.cuda.synchronize()
        do_plan(lengths)
        launches(g_out, g_lse)                                   # warm: the scratch grows outside the capture
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with graph_capture(graph, st):
            launches(g_out, g_lse)
        for step in (0, 1, 3):
            lens = lengths + step
            do_plan(lens)
            g_out.fill_(float("nan")); g_lse.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                graph.replay()
            st.synchronize()
            e_out, e_lse = fresh((L, n, H), torch)
            torch.cuda.synchronize()
            launches(e_out, e_lse)
            st.synchronize()
            assert_same_float_bits(g_out.cpu().numpy(), e_out.cpu().numpy(), f"replay at lengths + {step}")
            assert_same_float_bits(g_lse.cpu().numpy(), e_lse.cpu().numpy(), f"replay lse at lengths + {step}")
            assert bool(torch.isfinite(g_out).all())
        del graph
    finally:
        m.free()


# ----------------------------------------------------------------------------- connector
def connector_reference(hq, scheme, q16, k, v, lo, length, sm):
    """float64 attention of one (request, layer, head): q16 [G][D] fp16 as the connector hands it to the kernel, k / v [length][D] float64
    as the pool and the tail hold them; stored positions [lo, length & ~1) meet the quantised query, an odd length's last position the
    fp16 one (HeadChecker.want_rows restated over kv_rows).  out, lse, mag, delta"""
    stored = length & ~1
    qe = hq.q_rows(q16)
    s = (qe @ k[lo:stored].T) * sm
    delta = 3e-5 * float((np.abs(qe) @ np.abs(k[lo:stored]).T).max(initial=0.0)) * sm if scheme != INT4 else 0.0
    vv = v[lo:stored]
    if length & 1:
        s = np.concatenate([s, (q16.astype(np.float64) @ k[length - 1])[:, None] * sm], axis=1)
        vv = np.concatenate([vv, v[length - 1][None]])
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return (p @ vv) / l[:, None], mx + np.log(l), (p @ np.abs(vv)) / l[:, None], delta


@pytest.mark.parametrize("kscale_on", [False, True], ids=["plain", "k-prescale"])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_connector_decode_over_local_and_global_layers(oracle, scheme, kscale_on):
    """six decode steps of four requests over layers local (W = 40), global, local, global: every step's rows against float64 over
    kv_rows, and the global layers' bits equal to those of a connector that was never given a window"""
    import cxl_speckv_amd as pkg
    torch = torch_mod()
    drop_engine()                                             # one engine in the process at a time
    NL, W, prompts, rids = 4, 40, [37, 64, 90, 5], [0, 1, 2, 3]
    code = {"fp8": FP8, "int4": INT4, "mxfp4": MX4}[scheme]
    hq = HeadChecker(oracle, code, np.zeros((32, 2048), np.float16), 32)          # (its q_rows: the query as the format's kernel takes it)
    rng = np.random.default_rng(9950)
    rows = lambda *shape: (rng.standard_normal(shape) * rng.uniform(0.2, 3.0, shape[:-1] + (1,))).astype(np.float16)
    pk, pv = [rows(NL, n, H, D) for n in prompts], [rows(NL, n, H, D) for n in prompts]
    steps = [(rows(4, NL, H, D), rows(4, NL, H, D), (rng.standard_normal((NL, 4, H, G, D)) * 1.5).astype(np.float16)) for _ in range(6)]
    kscale = np.exp2(rng.integers(-2, 3, (NL, H, D))).astype(np.float32) if kscale_on else None
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    worst = 0.0
    try:
        conns = [SpeckvKVConnector(lib, NL, H, D, T, scheme) for _ in range(2)]     # [0]: local + global layers, [1]: never given a window
        keep = []
        for c, conn in enumerate(conns):
            if kscale is not None:
                conn.set_k_channel_scale(torch.from_numpy(kscale).cuda())
            for rid, k, v in zip(rids, pk, pv):
                conn.add_request(rid + 10 * c)
                keep += conn.write_prefill(rid + 10 * c, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
        ids = [[r + 10 * c for r in rids] for c in range(2)]
        for step, (k_new, v_new, q) in enumerate(steps):
            dq = torch.from_numpy(q).cuda()
            for c, conn in enumerate(conns):
                keep.append(conn.append(ids[c], torch.from_numpy(k_new).cuda(), torch.from_numpy(v_new).cuda()))
            outs = [conns[0].attend(layer, ids[0], dq[layer], SM, window=W if layer % 2 == 0 else None).cpu().numpy() for layer in range(NL)]
            plain = [conns[1].attend(layer, ids[1], dq[layer], SM).cpu().numpy() for layer in (1, 3)]
            torch.cuda.synchronize()
            assert_same_float_bits(outs[1], plain[0], f"step {step}: global layer 1 beside local layers")
            assert_same_float_bits(outs[3], plain[1], f"step {step}: global layer 3 beside local layers")
            for layer in range(NL):
                for b, rid in enumerate(ids[0]):
                    length = conns[0].length(rid)
                    lo = max(0, length - W) if layer % 2 == 0 else 0
                    k = conns[0].kv_rows(rid, layer, 0).double().cpu().numpy()
                    v = conns[0].kv_rows(rid, layer, 1).double().cpu().numpy()
                    for head in range(H):
                        q16, kk = q[layer, b, head], k[:, head]
                        if kscale is not None:                    # the pool holds K / scale, the kernel meets it with q x scale (powers of two: exact)
                            q16, kk = (q16.astype(np.float32) * kscale[layer, head]).astype(np.float16), kk / kscale[layer, head]
                        want, _, mag, delta = connector_reference(hq, code, q16, kk, v[:, head], lo, length, SM)
                        err = np.abs(outs[layer][b, head] - want)
                        tol = (2e-3 + 2 * delta) * mag + 1e-6
                        worst = max(worst, float((err / tol).max()))
                        assert np.all(err <= tol), (scheme, kscale_on, step, layer, rid, head, float((err / tol).max()))
        torch.cuda.synchronize()
        del keep
    finally:
        lib.finalize()
    print(f"decode window connector {scheme}{' k-prescale' if kscale_on else ''}: worst err/tol {worst:.3f}")


def test_the_sliding_window_decode_example_agrees_with_its_torch_reference():
    """examples/sliding_window_decode_example.py in this process, short: local and global layers alternating, four requests, odd and
    even lengths, every step against torch over kv_rows"""
    import importlib.util
    import os
    drop_engine()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sliding_window_decode_example.py")
    spec = importlib.util.spec_from_file_location("sliding_window_decode_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for scheme in ("fp8", "int4", "mxfp4"):
        assert mod.run(scheme, window=40, prompts=(70, 33, 48), steps=3, verbose=False) == 3
