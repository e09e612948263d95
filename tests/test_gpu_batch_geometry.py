"""-m gpu: batched decode-step attention against float64 in every launch geometry of the batch entry
(speckv_ext_attend_{fp8,int4,mx4}_batch) and the planned entry (speckv_ext_attend_batch_plan + *_planned).

Each case names the geometry regime it is built to reach and proves that on the host first, through the rules the engine decides
with (attend_geometry.hpp and ring_rule.hpp, wrapped by tests/csrc/host_rules_test.cpp and asked through tests/_rules.py); a failing branch assertion means the case no longer tests its
regime.  Then EVERY (member, head, query row) of out and lse is checked against the float64 attention over the dequantised records
(tests/_gpu.py HeadChecker.check_rows: |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, lse within 2e-3 + delta, empty members 0).
Members share a few KV contents (each dequantised once) and have their own queries; all seeds are fixed.

Also here: a captured planned launch keeps the room of its shape however many other shapes are planned meanwhile
(engine_attend.cpp attend_batch_plan: plan_rooms_), and attend_planned_layers refuses a tail stride that does not cover its layers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests._rules import ORDER_AS_GIVEN, decide, load_rules

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 4096
G = 8                                            # query rows per kv head
SM = 1.0 / np.sqrt(D)
FP8, INT4, MX4 = 4, 3, 5
NAMES = {FP8: "fp8", INT4: "int4", MX4: "mx4"}
N_CONTENTS = 3


def cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def rules():
    lib = load_rules()
    P = C.POINTER(C.c_uint32)
    for name, args in (("rules_fp8_batch_tiles_per_split", [P] + [C.c_uint32] * 4), ("rules_balanced_tiles_per_piece", [P] + [C.c_uint32] * 5),
                       ("rules_ragged_tiles_per_piece", [P] + [C.c_uint32] * 3)):
        getattr(lib, name).restype = C.c_uint32
        getattr(lib, name).argtypes = args
    lib.rules_dispatch_order.restype = C.c_int
    lib.rules_dispatch_order.argtypes = [P, C.c_uint32, C.c_uint32, P]
    lib.rules_int4_unequal.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, P]
    return lib


def u32(a):
    a = np.ascontiguousarray(a, np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def tiles_of(lens):
    return (np.asarray(lens, np.int64) // 2 + 15) // 16          # tiles of 32 positions (the linear form of a single pool)


# ----------------------------------------------------------------------------- the regimes
def regime(name, n_cus):
    """(member lengths, formats) of a regime; lengths are fixed by a seed of their own"""
    rng = np.random.default_rng({"R1": 1, "R2a": 2, "R2b": 3, "R3": 4, "R4": 5, "R5": 6, "R6": 7}[name] + 7000)
    if name == "R1":                              # equal lengths, one round of workgroups
        return np.full(24, 2048), (FP8, INT4, MX4)
    if name == "R2a":                             # between half a machine and a whole one, 4k each
        return np.full(n_cus // 2 + 2, 4096), (FP8, INT4, MX4)
    if name == "R2b":                             # more members than CUs, 4k each
        return np.full(n_cus + 4, 4096), (FP8, INT4, MX4)
    if name == "R3":                              # heavy tail: most 1k..2k, one in 16 at 16k, an empty member and a two-position one
        lens = rng.integers(512, 1025, 64) * 2
        lens[7::16] = 16384
        lens[3], lens[5] = 0, 2
        return lens, (FP8, INT4, MX4)
    if name == "R4":                              # more members than a dispatch round, lengths 0.5k..2k
        return rng.integers(256, 1025, n_cus + 44) * 2, (FP8, INT4)
    if name == "R5":                              # INT4 page-table form, 400 workgroup columns, the longest member 256 tiles
        lens = rng.integers(256, 1025, 200) * 2
        lens[0], lens[50], lens[120] = 8192, 6144, 7000
        return lens, (INT4,)
    if name == "R6":                              # FP8, 200 workgroup columns of 128 tiles: split pricing below the machine
        return np.full(100, 4096), (FP8,)
    raise KeyError(name)


def assert_branch(rules, name, scheme, entry, lens, n_cus):
    """The case reaches its regime: the engine's own decision (attend_geometry.hpp batch_form / batch_geometry / batch_dispatch_order, as
    Engine::attend_batch and attend_batch_plan + attend_planned call them; tests/_rules.py decide) gives the geometry the regime names.
    FP8 split lengths are priced for 256 CUs by the engine (batch_tiles_per_split)."""
    n = len(lens)
    t = tiles_of(lens)
    tmax = int(t.max())
    cols = 2 if scheme == FP8 else 1                              # workgroup columns per member (8 kv heads: FP8 two, the others one)
    model = {FP8: 1, MX4: 0, INT4: 3}[scheme]                     # rules_ragged_tiles_per_piece: FP8 / one column, one slot
    tarr, tp = u32(t)
    ragged = rules.rules_ragged_tiles_per_piece(tp, n, n_cus, model)
    pages = np.asarray(lens) // 2
    # R5: the first member has a migrated page (no regular placement), the others lie in single runs
    d = decide(rules, scheme, "batch" if entry == "batch" else "plan", pages, n_cus, any_table=name == "R5")
    equal = decide(rules, scheme, "batch" if entry == "batch" else "plan", pages, n_cus, any_table=name == "R5", tuning=ORDER_AS_GIVEN)      # the rule for equal lengths
    order_round, by_length, order, tps = d["round"], d["by_length"], d["order"], d["tps"]
    assert d["fits"] == 1 and order_round == (0 if scheme == MX4 else (n_cus // 2 if scheme == FP8 else n_cus))
    if name == "R1":
        assert n * cols <= n_cus and ragged == 0 and by_length == 0            # one round, no pieces on account of the lengths, the order as given
        assert d["rows_first"] == 0 and d["piece_tps"] == tps
    elif name in ("R2a", "R2b"):
        assert ragged == 0 and by_length == 0 and d["rows_first"] == 0
        if scheme == FP8:                                          # more columns than CUs, 128 tiles: the balanced pieces
            assert n * cols > 256 and tmax >= 128
            assert tps == rules.rules_fp8_batch_tiles_per_split(None, n, tmax, cols, 256)
            assert tps < tmax and tps == rules.rules_balanced_tiles_per_piece(None, n, tmax, cols, 256, 1)
        elif scheme == INT4:                                       # int4_wg8_batch_tps: one-run workgroups past the CU count (form 2), 16-wave ones below (form 1)
            wg8_form = d["wg8"]
            assert wg8_form == (1 if name == "R2a" else 2)
            assert tps == rules.rules_balanced_tiles_per_piece(None, n, tmax, 1, n_cus, 2 if wg8_form == 2 else 3)
            assert 2 * n > n_cus and tmax >= 64 and tps < tmax
        elif name == "R2b":                                        # mx4_batch_tps: past the CU count, the balanced pieces
            assert n > n_cus and tps == rules.rules_balanced_tiles_per_piece(None, n, tmax, 1, n_cus, 0) and tps < tmax
        else:                                                      # MXFP4 below the CU count at 4k: whole members, the 8-wave halves form
            assert n <= n_cus and not (2 * n > n_cus and tmax >= 256) and tps == tmax and d["max_splits"] == 1
        assert d["max_splits"] == -(-tmax // tps)
    elif name == "R3":                                             # pieces on account of the lengths, rows first, by length
        assert by_length == 1 and ragged != 0 and ragged < tmax
        assert d["rows_first"] == 1 and d["max_splits"] > 1 and ragged <= d["piece_tps"] < equal["tps"]
        if entry == "batch":
            assert tps == ragged
        if scheme == FP8:
            assert ragged < rules.rules_fp8_batch_tiles_per_split(tp, n, 0, cols, 256)
        else:                                                      # mx4_batch_tps / int4_wg8_batch_tps below the CU count: one round of splits
            assert n <= n_cus // 2 and ragged < equal["tps"] and equal["piece_tps"] == equal["tps"]
    elif name == "R4":                                             # the serpentine: more members than a round, one round reversed at least
        assert by_length == 1 and order_round and n > order_round
        got = np.asarray(lens)[order] // 2
        assert np.all(np.diff(got[:order_round]) <= 0) and np.all(np.diff(got[order_round:2 * order_round]) >= 0)
    elif name == "R5":                                             # the batch entry off the whole-record kernel: unequal halves
        out = (C.c_uint32 * 3)()
        rules.rules_int4_unequal(2 * n, tmax, tmax, out)
        assert 384 <= 2 * n <= 672 and tmax >= 192 and out[0] == 1 and out[2] == 2 and tmax // 2 <= out[1] < tmax
        assert d["table"] == 1 and d["wg8"] == 0
        if entry == "batch":
            assert d["unequal"] == 1 and d["max_splits"] == 2 and d["rows_first"] == 1 and int(d["pieces"][0, 0]) == out[1]
        else:
            # (the planned entry keeps the whole-record geometry for 8 kv heads whatever the placement -- batch_geometry says why -- and runs the
            #  page-table form with it: what its case proves is that form, by the migration below)
            assert d["unequal"] == 0
    elif name == "R6":                                             # FP8 below the machine: the split rule prices pieces
        assert n * cols <= 256
        assert tps == rules.rules_fp8_batch_tiles_per_split(None, n, tmax, cols, 256)
        assert tps < tmax and n * cols * -(-tmax // tps) > 256 and d["max_splits"] == -(-tmax // tps)


# ----------------------------------------------------------------------------- building a case
class Case:
    """The members of a regime in one format: N_CONTENTS KV contents of the longest length, member i holding the first
    positions of content i % N_CONTENTS in an allocation of its own, one layer, its own queries."""

    def __init__(self, kv, oracle, scheme, lens, seed, layers=1, migrate_first=False):
        torch = torch_mod()
        self.kv, self.lib, self.scheme = kv, kv.lib, scheme
        self.lens = np.asarray(lens, np.int64)
        n = len(lens)
        self.T = [max(32, -(-int(v) // 32) * 32) for v in self.lens]
        tmax = max(self.T)
        self.lib.set_compression_scheme(scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
        contents = []
        for c in range(N_CONTENTS):                               # K region, then V region: tmax / 2 pages each
            x = torch.randn((tmax, 2048), generator=gen, device="cuda")
            x = (x * (torch.rand((tmax, 1), generator=gen, device="cuda") * 2.8 + 0.2)).to(torch.float16)
            contents.append(x)
        self.handles = []
        for i in range(n):
            x, T = contents[i % N_CONTENTS], self.T[i]
            h = self.lib.alloc(T * layers * 2 * 2048 * 2)
            self.lib.set_layout(h, T, layers, H, D, 2)
            for layer in range(layers):
                base = layer * T * PAGE                            # pages of a layer: T / 2 of K, T / 2 of V
                self.lib.write(h, base, x.data_ptr(), T // 2 * PAGE, True)
                self.lib.write(h, base + T // 2 * PAGE, x[tmax // 2:].data_ptr(), T // 2 * PAGE, True)
            self.handles.append(h)
        if migrate_first:
            self.lib.migrate(self.handles[0], 5, 1, 1)             # one page to pool 1: no regular placement, the page-table form
        torch.cuda.synchronize()
        self.checkers = [HeadChecker(oracle, scheme, x.cpu().numpy(), tmax) for x in contents]
        del contents
        rng = np.random.default_rng(seed)
        self.qh = (rng.standard_normal((layers, n, H, G, D)) * 1.5).astype(np.float16)
        self.q = torch.from_numpy(self.qh).cuda()
        self.max_pos_end = int(self.lens.max())

    def check(self, out, lse, lens, what, layer=0, tail=None):
        lens = np.asarray(lens)
        for c, hc in enumerate(self.checkers):
            idx = np.arange(c, len(lens), N_CONTENTS)
            for head in range(H):
                tl = None if tail is None else (tail[0][idx, layer, head], tail[1][idx, layer, head])
                hc.check_rows(out[idx, head], lse[idx, head], self.qh[layer][idx, head], head, lens[idx], SM, (what, "content", c, "head", head), tl)

    def free(self):
        for h in self.handles:
            self.lib.free(h)
        self.handles = []


def fresh(n, torch):
    return (torch.full((n, H, G, D), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((n, H, G), float("nan"), dtype=torch.float32, device="cuda"))


def run_entry(case, entry):
    torch = torch_mod()
    lib, n = case.lib, len(case.lens)
    out, lse = fresh(n, torch)
    lens = case.lens.astype(np.uint32)
    if entry == "batch":
        batch = {FP8: lib.attend_fp8_batch, INT4: lib.attend_int4_batch, MX4: lib.attend_mx4_batch}[case.scheme]
        batch(case.handles, 0, case.q[0].data_ptr(), G, lens, SM, out.data_ptr(), lse.data_ptr())
        torch.cuda.synchronize()
    else:
        st = torch.cuda.Stream()
        plan_bytes = lib.attend_plan_bytes(n)
        plan = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lib.attend_batch_plan(case.handles, lens, case.max_pos_end, plan.data_ptr(), plan_bytes, st.cuda_stream)
        lib.attend_planned(case.scheme, plan.data_ptr(), n, 0, case.q[0].data_ptr(), G, case.max_pos_end, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
        st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


# One engine at a time in the process (speckv_init); cases of a regime and format are kept for both entries, and dropped with their engine.
_state = {"kv": None, "pools": None, "key": None, "case": None}


def drop_engine():
    if _state["case"] is not None:
        _state["case"].free()
    if _state["kv"] is not None:
        _state["kv"].close()
    _state.update(kv=None, pools=None, key=None, case=None)


def engine(pools=1, fresh=False):
    """the module's engine over `pools` pools on this GPU (a second one to migrate pages to); fresh: a new engine, no state of earlier tests"""
    if fresh or _state["pools"] != pools:
        drop_engine()
        if pools > 1:
            os.environ["SPECKV_POOL_DEVICES"] = ",".join(["0"] * pools)
        try:
            _state["kv"] = pkg.CxlSpeckvKVAllocator(pkg.library_path(), "hip:0")
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        _state["pools"] = pools
    return _state["kv"]


def cached_case(key, pools, make):
    kv = engine(pools)
    if _state["key"] != key:
        if _state["case"] is not None:
            _state["case"].free()
        _state.update(key=None, case=None)
        _state["case"] = make(kv)
        _state["key"] = key
    return _state["case"]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_engine()


CASES = [(r, s, e) for r in ("R1", "R2a", "R2b", "R3", "R4", "R5", "R6") for s in regime(r, 256)[1] for e in ("batch", "planned")]


@pytest.mark.parametrize("name,scheme,entry", CASES, ids=[f"{r}-{NAMES[s]}-{e}" for r, s, e in CASES])
def test_batch_geometry_against_float64(oracle, rules, name, scheme, entry):
    n_cus = cus()
    lens, schemes = regime(name, n_cus)
    assert scheme in schemes
    assert_branch(rules, name, scheme, entry, lens, n_cus)
    seed = 7100 + 10 * ["R1", "R2a", "R2b", "R3", "R4", "R5", "R6"].index(name) + scheme
    # R5: two pools on this GPU, the first member's page 5 migrated to the second (the page-table form)
    case = cached_case((name, scheme), 2 if name == "R5" else 1, lambda kv: Case(kv, oracle, scheme, lens, seed, migrate_first=name == "R5"))
    out, lse = run_entry(case, entry)
    case.check(out, lse, case.lens, (name, NAMES[scheme], entry))


# ----------------------------------------------------------------------------- a captured plan keeps its room
@pytest.mark.parametrize("first", ["equal", "ragged"])
@pytest.mark.parametrize("scheme", [FP8, INT4, MX4], ids=["fp8", "int4", "mx4"])
def test_captured_plan_keeps_its_room_past_4096_shapes(oracle, rules, scheme, first):
    """Plan buffer B1 for CUs members under a bound of 4096 positions (the rule for that shape: one split per member, no merge launch),
    first with equal lengths or with a heavy tail (room for pieces and the merge launch), capture the planned launch over B1; then
    more than 4096 other shapes planned through a second buffer B2; then B1 re-planned with the other lengths of the same shape and
    the graph replayed.  The replay must still match float64 on every row: the room B1's graph was captured with stays B1's room
    (engine_attend.cpp attend_batch_plan: rooms are dropped only for buffers that hold no plan any more)."""
    torch = torch_mod()
    n_cus = cus()
    n = n_cus
    ragged = np.full(n, 256); ragged[::16] = 4096
    equal = np.full(n, 256)
    t_r, tp_r = u32(tiles_of(ragged)); t_e, tp_e = u32(tiles_of(equal))
    model = {FP8: 1, MX4: 0, INT4: 3}[scheme]
    # the shape's rule: one split per member (FP8: whole rounds of columns; INT4: the 16-wave form at CUs members; MXFP4: one round)
    if scheme == FP8:
        assert rules.rules_fp8_batch_tiles_per_split(None, n, 128, 2, 256) == 128
    elif scheme == INT4:
        assert rules.rules_balanced_tiles_per_piece(None, n, 128, 1, n_cus, 3) == 128
    assert rules.rules_ragged_tiles_per_piece(tp_r, n, n_cus, model) != 0 and rules.rules_ragged_tiles_per_piece(tp_e, n, n_cus, model) == 0
    kv = engine(fresh=True)                                         # a new engine: no room of an earlier test at a reused address
    case = None
    try:
        lens = ragged.copy()                                        # allocations long enough for either set of lengths
        case = Case(kv, oracle, scheme, lens, 7300 + scheme)
        lib = case.lib
        first_lens, second_lens = (equal, ragged) if first == "equal" else (ragged, equal)
        st = torch.cuda.Stream()
        plan_bytes = lib.attend_plan_bytes(n)
        b1 = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
        b2 = torch.zeros(lib.attend_plan_bytes(1), dtype=torch.uint8, device="cuda")
        out, lse = fresh(n, torch)
        torch.cuda.synchronize()
        lib.attend_batch_plan(case.handles, first_lens.astype(np.uint32), 4096, b1.data_ptr(), plan_bytes, st.cuda_stream)
        call = lambda: lib.attend_planned(scheme, b1.data_ptr(), n, 0, case.q[0].data_ptr(), G, 4096, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
        call(); st.synchronize()                                    # warm: the scratch is sized outside the capture
        case.check(out.cpu().numpy(), lse.cpu().numpy(), first_lens, (NAMES[scheme], first, "first plan"))
        graph = torch.cuda.CUDAGraph()
        with graph_capture(graph, st):
            call()
        long_member = [case.handles[0]]                             # 4096 positions of room
        for k in range(1, 4200):                                    # 4199 shapes of one member: (1, max_pos_end = 2k)
            lib.attend_batch_plan(long_member, np.array([2], np.uint32), 2 * k, b2.data_ptr(), b2.numel(), st.cuda_stream)
        st.synchronize()
        lib.attend_batch_plan(case.handles, second_lens.astype(np.uint32), 4096, b1.data_ptr(), plan_bytes, st.cuda_stream)
        st.synchronize()
        out.fill_(float("nan")); lse.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        case.check(out.cpu().numpy(), lse.cpu().numpy(), second_lens, (NAMES[scheme], first, "replay after 4199 shapes"))
        del graph
    finally:
        if case is not None:
            case.free()
        drop_engine()


# ----------------------------------------------------------------------------- the tail stride of several planned layers
def test_planned_layers_tail_stride_must_cover_every_layer(oracle):
    """attend_planned_layers over MXFP4, a one-split plan and two layers folds each member's tail position into both layers inside
    the kernel (rows layer_begin .. layer_begin + n_layers - 1 of the tail): a stride that covers one layer is refused before anything
    runs; with the right stride both layers match float64 attention over the pool's positions and the folded one."""
    torch = torch_mod()
    lens = np.array([256, 200, 130, 2, 64, 256, 98, 34])            # no empty member (the in-kernel fold needs every member's split 0)
    n, L = len(lens), 2
    # one split per member: mx4_batch_tps with 8 tiles at most is 8 tiles (attend_geometry.hpp), and no pieces on account of the lengths
    assert decide(load_rules(), MX4, "plan", lens // 2, cus())["max_splits"] == 1 and int(tiles_of(lens).max()) == 8
    case = Case(engine(fresh=True), oracle, MX4, lens, 7400, layers=L)
    try:
        lib = case.lib
        rng = np.random.default_rng(7401)
        kt = (rng.standard_normal((n, L, H, D)) * 1.5).astype(np.float16)
        vt = rng.standard_normal((n, L, H, D)).astype(np.float16)
        d_kt, d_vt = torch.from_numpy(kt).cuda(), torch.from_numpy(vt).cuda()
        st = torch.cuda.Stream()
        plan_bytes = lib.attend_plan_bytes(n)
        plan = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
        out = torch.full((L, n, H, G, D), float("nan"), dtype=torch.float32, device="cuda")
        lse = torch.full((L, n, H, G), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lib.attend_batch_plan(case.handles, lens.astype(np.uint32), 256, plan.data_ptr(), plan_bytes, st.cuda_stream)
        st.synchronize()
        with pytest.raises(SpeckvError):
            lib.attend_planned_layers(MX4, plan.data_ptr(), n, 0, L, case.q.data_ptr(), G, 256, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream,
                                      n_tail=n, d_k_tail=d_kt.data_ptr(), d_v_tail=d_vt.data_ptr(), tail_stride_elems=H * D)
        st.synchronize()
        assert torch.isnan(out).all() and torch.isnan(lse).all()    # nothing launched
        lib.attend_planned_layers(MX4, plan.data_ptr(), n, 0, L, case.q.data_ptr(), G, 256, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream,
                                  n_tail=n, d_k_tail=d_kt.data_ptr(), d_v_tail=d_vt.data_ptr(), tail_stride_elems=L * H * D)
        st.synchronize()
        o, l = out.cpu().numpy(), lse.cpu().numpy()
        for layer in range(L):
            case.check(o[layer], l[layer], lens, ("planned layers with tails", layer), layer=layer, tail=(kt, vt))
    finally:
        case.free()
        drop_engine()
