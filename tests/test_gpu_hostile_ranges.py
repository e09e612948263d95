"""-m gpu: decode attention with HOSTILE rows outside the attended range, in every kernel body the small layouts reach.

truncate clears nothing: whatever lies at or behind pos_end -- and in front of pos_begin where a range starts inside a tile -- is still in
the pool, and every attention kernel masks it by itself.  Here every page of the K region outside the range holds K x 200 and every page
of the V region sign(v) x 1000 (the magnitudes of tests/test_gpu_rollback.py::test_stale_records_behind_the_cut_are_never_seen); the
kept pages hold ordinary rows (randn x U(0.2, 3) per page).  EVERY (layer, head, query row) of out and lse is held to float64 attention
over the oracle's dequantised records of exactly the kept positions (tests/_gpu.py HeadChecker.check_rows: |err| <= (2e-3 + 2 delta)
sum p|v| + 1e-6, lse within 2e-3 + delta, an empty member exactly 0), and out / lse must be finite.  A mask applied behind the running
maximum, a mask one page off or a scored trailing class tile lets a row of 200 x the magnitude into the softmax: the error is then of
the order of the output itself.  All seeds are fixed; the worst err / tol of every case is printed.

Layout: 8 kv heads x 128, G = 8 query rows per kv head, L = 2 layers (layer 0 hostile, layer 1 ordinary in the single-sequence cases;
both hostile behind a member's end in the batch cases), T = 256 positions (FP8: with a scale table) and T = 200 (FP8: none).  Ranges are
even on both sides: a page is wholly kept or wholly hostile.  Placements: one pool; pools striped over 3 and over 7 (residue classes;
7 pages over 7 classes, 2 pages over 3: unequal and empty classes); a striped pool with one K and one V page migrated (no regular
placement: the page tables); attend_general = 1 on one pool.

Kernel body -> the case that runs it (single = test_single_sequence_entries, batch = test_batch_and_planned_entries; "inside" = a range
that begins inside a 32-position tile, "aligned" = one that begins on a tile; FP8 only aligns its range down to the tile, INT4 / MXFP4
count their tiles from pos_begin)

  k_attend_fp8                               single, any placement, T = 200 (no scale table), (34, 100) and (0, 70)
  k_attend_fp8_dma<0>                        single, one pool, T = 256, every range (inside ones too: skip_pages)
  k_attend_fp8_linear<false>                 single, one pool, attend_fp8_dma = -1, every range; batch + planned, one pool
  k_attend_fp8_dma<2>                        single, striped 3 / 7, aligned ranges (32, 64) (0, 70) (0, 14)
  k_attend_fp8_linear<true>                  single, striped 3 / 7, inside ranges; attend_fp8_table_regs = 1: every range;
                                             batch + planned, striped 3, attend_fp8_table_regs = 1
  k_attend_fp8_dma<1>                        single, striped, attend_fp8_striped_table = 1, aligned ranges; single, migrated and
                                             attend_general, aligned ranges; batch + planned, striped 3 (default) and migrated
  k_attend_fp8_linear<false, true>           single, migrated / attend_general, inside ranges; attend_fp8_table_regs = 1: every range;
                                             batch + planned, migrated, attend_fp8_table_regs = 1
  k_attend_fp8_linear<false, false, true>    batch + planned, striped 3, attend_fp8_striped_table = -1.  NOT reached from the single
                                             entry: launch_attend_fp8 takes it with n_splits > 1 and 128 workgroup columns = 64 layers
  k_attend_int4_wg8<2>                       single, one pool, ranges whose tiles stay inside the region; batch + planned, one pool
  k_attend_int4_wg8<2, true>                 single, striped 3 / 7, the same ranges; batch + planned, striped 3
  k_attend_int4_wg<true>                     single, striped, attend_int4_striped_wg = 1, the same ranges; batch + planned likewise
  k_attend_int4_wg<false, true>              single, any placement, ranges whose last tile would leave the region ((6, 256), (254, 256));
                                             migrated and attend_general: every range; batch + planned, migrated
  k_attend_int4_wg8<1>, <1, true>            NOT reached: the one-run workgroups take batches of more members than CUs (wg8 == 2) and
                                             the stream form (896 tiles a layer); same body as <2>, tests/test_gpu_batch_geometry.py R2b
  k_attend_int4_wg<false>                    NOT reached by any entry: with 8 kv heads (the only layout the entries take: heads x 128 =
                                             1024) records in one run always take the whole-record kernel
  k_attend_mx4<0>                            single, one pool, ranges whose tiles stay inside the region; batch, one pool (an empty
                                             member: partials and the merge); batch + planned with attend_mx4_one_half
  k_attend_mx4<0, 2>                         planned, one pool; batch, one pool, the five members that are not empty; planned_layers
  k_attend_mx4<1>                            single, striped 3 / 7, every range; batch + planned, striped 3
  k_attend_mx4<2>                            single, one pool, (6, 256) and (254, 256); migrated and attend_general: every range;
                                             batch + planned, migrated
  k_attend_mx4<3> and the INT4 stream form   NOT reached: several layers of 896 tiles or more (or attend_stream), tile-aligned ranges
                                             only -- tests/test_gpu_int4_stream.py, tests/test_gpu_mx4.py

No entry refuses any of the ranges below (REFUSED is empty); a refusal that is not listed there fails the case, a listed one must have
written nothing."""
import contextlib
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, decide, load_rules

pytestmark = pytest.mark.gpu
PAGE = 4096
G = 8                                            # query rows per kv head
L = 2
SM = 1.0 / np.sqrt(D)
FP8, INT4, MX4 = 4, 3, 5
NAMES = {FP8: "fp8", INT4: "int4", MX4: "mx4"}
K_HOSTILE, V_HOSTILE = 200.0, 1000.0
RANGES = {256: [(6, 256), (34, 100), (62, 66), (30, 32), (32, 64), (0, 70), (0, 14), (254, 256)], 200: [(34, 100), (0, 70)]}
POS_END = np.array([0, 2, 70, 96, 254, 256])     # the batch: six members in allocations of 256 positions
TAIL_LENS = np.array([256, 200, 130, 2, 64, 256, 98, 34])      # tests/test_gpu_batch_geometry.py::test_planned_layers_tail_stride_must_cover_every_layer
POOLS = {"one": 1, "general": 1, "striped3": 3, "striped7": 7, "migrated": 3}
MIGRATED_PAGE = 17                               # positions 34, 35 of layer 0: its K page and its V page go to pool 1
REFUSED = set()                                  # (format, T, pos_begin, pos_end) an entry refuses: none


def cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- content and reference, built once
_base, _checkers = {}, {}


def base(T):
    """ordinary rows: the pages of L layers (T / 2 of K, T / 2 of V each), randn x U(0.2, 3) per page"""
    if T not in _base:
        rng = np.random.default_rng(9100 + T)
        _base[T] = (rng.standard_normal((L * T, 2048)) * rng.uniform(0.2, 3.0, (L * T, 1))).astype(np.float16)
    return _base[T]


def hostile(T, keep, layers, v_mag=V_HOSTILE):
    """base(T) with every K / V page of `layers` outside the positions keep = [begin, end) made hostile"""
    x = base(T).copy()
    out = np.ones(T // 2, bool)
    out[keep[0] // 2:keep[1] // 2] = False
    for layer in layers:
        k = layer * T + np.nonzero(out)[0]
        v = k + T // 2
        x[k] = (x[k].astype(np.float32) * K_HOSTILE).astype(np.float16)
        x[v] = (np.sign(x[v].astype(np.float32)) * v_mag).astype(np.float16)
    assert np.isfinite(x.astype(np.float32)).all()
    return x


def checker(oracle, scheme, T, layer):
    """float64 attention over the ORDINARY content of a layer: the kept pages of every case are its pages (the formats quantise page by page)"""
    key = (scheme, T, layer)
    if key not in _checkers:
        _checkers[key] = HeadChecker(oracle, scheme, base(T)[layer * T:(layer + 1) * T], T)
    return _checkers[key]


# ----------------------------------------------------------------------------- one engine per placement, reused across cases
_state = {"kv": None, "pools": None}


def drop_engine():
    if _state["kv"] is not None:
        _state["kv"].close()
    _state.update(kv=None, pools=None)


def engine(placement):
    pools = POOLS[placement]
    if _state["pools"] != pools:
        drop_engine()
        if pools > 1:
            os.environ["SPECKV_POOL_DEVICES"] = ",".join(["0"] * pools)
        try:
            _state["kv"] = pkg.CxlSpeckvKVAllocator(pkg.library_path(), "hip:0")
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        _state["pools"] = pools
    return _state["kv"].lib


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_engine()
    _checkers.clear()
    _base.clear()


@contextlib.contextmanager
def tuned(keys):
    try:
        for k, v in keys:
            set_tuning(k, v)
        yield
    finally:
        for k, _ in keys:
            set_tuning(k, 0)


def allocation(lib, scheme, T, x, migrate=False):
    lib.set_compression_scheme(scheme)
    h = lib.alloc(L * T * PAGE)
    lib.set_layout(h, T, L, H, D, 2)
    lib.write(h, 0, x.ctypes.data, x.nbytes, False)
    if migrate:                                  # no regular placement any more: the entries read addresses from the page table
        lib.migrate(h, MIGRATED_PAGE, 1, 1)
        lib.migrate(h, T // 2 + MIGRATED_PAGE, 1, 1)
    return h


def fresh(shape, torch):
    return (torch.full(shape + (G, D), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full(shape + (G,), float("nan"), dtype=torch.float32, device="cuda"))


# ----------------------------------------------------------------------------- single-sequence entries
def single_tunings(placement, scheme):
    first = (("attend_general", 1),) if placement == "general" else ()
    tunings = [first]
    if scheme == FP8:
        if placement == "one":
            tunings.append((("attend_fp8_dma", -1),))
        elif placement in ("striped3", "striped7"):
            tunings += [(("attend_fp8_striped_table", 1),), (("attend_fp8_table_regs", 1),)]
        else:
            tunings.append(first + (("attend_fp8_table_regs", 1),))
    if scheme == INT4 and placement in ("striped3", "striped7"):
        tunings.append((("attend_int4_striped_wg", 1),))
    return tunings


def check_single(oracle, scheme, T, out, lse, qh, b, e, what, failures):
    """every (layer, head, row) of one call over [b, e) against float64; the figure is printed first, a case that misses goes to `failures`
    (the test asserts on them when all of its cases have run)"""
    worst, first = [], None
    for layer in range(out.shape[0]):
        hc = checker(oracle, scheme, T, layer)
        for head in range(H):
            try:
                hc.check_rows(out[layer, head][None], lse[layer, head][None], qh[layer, head][None], head, [e - b], SM, what + (layer, head),
                              pos_begin=b, worst=worst)
            except AssertionError as ex:
                first = first or ex.args[0]
    print(f"hostile single {what}: worst err/tol {max(worst):.3f}")
    if not (np.isfinite(out).all() and np.isfinite(lse).all()):
        first = first or (what, "out / lse not finite")
    if first is not None:
        failures.append((first, f"worst err/tol {max(worst):.3f}"))
    return max(worst)


SINGLE = [(p, s) for p in ("one", "general", "striped3", "striped7", "migrated") for s in (FP8, INT4, MX4)]


@pytest.mark.parametrize("placement,scheme", SINGLE, ids=[f"{p}-{NAMES[s]}" for p, s in SINGLE])
def test_single_sequence_entries(oracle, placement, scheme):
    """attend_fp8 / attend_int4 / attend_mx4 over [pos_begin, pos_end) of layer 0 alone and of both layers in one call, everything
    outside the range in layer 0 hostile; every tuning switch that selects another body for the placement (the module's table)."""
    torch = torch_mod()
    lib = engine(placement)
    fused = {FP8: lib.attend_fp8, INT4: lib.attend_int4, MX4: lib.attend_mx4}[scheme]
    rng = np.random.default_rng(9200 + scheme)
    overall, failures = 0.0, []
    for T in (256, 200):
        qh = (rng.standard_normal((L, H, G, D)) * 1.5).astype(np.float16)
        q = torch.from_numpy(qh).cuda()
        h = allocation(lib, scheme, T, base(T), migrate=placement == "migrated")
        try:
            for b, e in RANGES[T]:
                x = hostile(T, (b, e), (0,))
                lib.write(h, 0, x.ctypes.data, x.nbytes, False)
                for tuning in single_tunings(placement, scheme):
                    for n_layers in (1, 2):
                        what = (placement, NAMES[scheme], T, tuning, (b, e), n_layers)
                        out, lse = fresh((n_layers, H), torch)
                        refused = False
                        with tuned(tuning):
                            try:
                                fused(h, 0, n_layers, q.data_ptr(), G, b, e, SM, out.data_ptr(), lse.data_ptr())
                            except SpeckvError:
                                refused = True
                            torch.cuda.synchronize()
                        assert refused == ((scheme, T, b, e) in REFUSED), (what, "refused" if refused else "not refused")
                        if refused:
                            assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all()), (what, "a refused call wrote")
                            continue
                        o, l = out.cpu().numpy(), lse.cpu().numpy()
                        overall = max(overall, check_single(oracle, scheme, T, o, l, qh, b, e, what, failures))
        finally:
            lib.free(h)
    print(f"hostile single {placement}-{NAMES[scheme]}: worst err/tol over all cases {overall:.3f}, {len(failures)} cases failed")
    assert not failures, failures[:6]


# ----------------------------------------------------------------------------- batch and planned entries
# (format, placement, variant) -> the tuning keys, the same as tests/_rules.py decide() takes them, and the form the engine must decide
BATCH_VARIANTS = {
    "default": ((), DEFAULT_TUNING),
    "by_class": ((("attend_fp8_striped_table", -1),), (0, 0, 0, -1, 0)),
    "table_regs": ((("attend_fp8_table_regs", 1),), (0, 0, 1, 0, 0)),
    "striped_wg": ((("attend_int4_striped_wg", 1),), (0, 0, 0, 0, 1)),
    "one_half": ((("attend_mx4_one_half", 1),), DEFAULT_TUNING),
}
FORM = ("table", "striped", "fp8_cls", "int4_cls", "by_class", "wg8")
BATCH = {   # the kernel body, and (table, striped, fp8_cls, int4_cls, by_class, wg8) of batch_form
    (FP8, "one", "default"): ("k_attend_fp8_linear<false>", (0, 0, 0, 0, 0, 0)),
    (FP8, "striped3", "default"): ("k_attend_fp8_dma<1>", (1, 0, 0, 0, 0, 0)),
    (FP8, "striped3", "by_class"): ("k_attend_fp8_linear<false, false, true>", (0, 1, 1, 0, 1, 0)),
    (FP8, "striped3", "table_regs"): ("k_attend_fp8_linear<true>", (0, 1, 0, 0, 0, 0)),
    (FP8, "migrated", "default"): ("k_attend_fp8_dma<1>", (1, 0, 0, 0, 0, 0)),
    (FP8, "migrated", "table_regs"): ("k_attend_fp8_linear<false, true>", (1, 0, 0, 0, 0, 0)),
    (INT4, "one", "default"): ("k_attend_int4_wg8<2>", (0, 0, 0, 0, 0, 1)),
    (INT4, "striped3", "default"): ("k_attend_int4_wg8<2, true>", (0, 1, 0, 1, 1, 1)),
    (INT4, "striped3", "striped_wg"): ("k_attend_int4_wg<true>", (0, 1, 0, 0, 0, 0)),
    (INT4, "migrated", "default"): ("k_attend_int4_wg<false, true>", (1, 0, 0, 0, 0, 0)),
    (MX4, "one", "default"): ("k_attend_mx4<0, 2> (no empty member, or planned) / k_attend_mx4<0>", (0, 0, 0, 0, 0, 0)),
    (MX4, "one", "one_half"): ("k_attend_mx4<0>", (0, 0, 0, 0, 0, 0)),
    (MX4, "striped3", "default"): ("k_attend_mx4<1>", (0, 1, 0, 0, 1, 0)),
    (MX4, "migrated", "default"): ("k_attend_mx4<2>", (1, 0, 0, 0, 0, 0)),
}
BATCH_CASES = sorted(BATCH, key=lambda c: (["one", "striped3", "migrated"].index(c[1]), c[0], c[2]))


def assert_form(rules, scheme, placement, variant, entry, pos_end, max_pos_end=None):
    """the engine's own decision for these members (tests/_rules.py decide) is the form the case is built for"""
    d = decide(rules, scheme, entry, np.asarray(pos_end) // 2, cus(), stripe_n=1 if placement == "one" else 3, any_table=placement == "migrated",
               tuning=BATCH_VARIANTS[variant][1], max_pos_end=max_pos_end)
    want = BATCH[(scheme, placement, variant)][1]
    assert tuple(d[k] for k in FORM) == want and d["fits"] == 1, (NAMES[scheme], placement, variant, entry, {k: d[k] for k in FORM})
    if scheme == MX4 and placement == "one":
        # the 8-wave halves form takes launches of one split each in single runs, a CU to each member: Engine::attend_batch wants every member
        # to HAVE its one split (no empty member), Engine::attend_planned the plan's room to be one split; attend_mx4_one_half keeps form 0
        assert d["max_splits"] == 1 and len(pos_end) <= cus()
    return d


class Batch:
    """members over base(256), member i hostile behind pos_end[i] in BOTH layers, queries of their own"""

    def __init__(self, lib, scheme, pos_end, seed, migrate_member=None):
        torch = torch_mod()
        self.lib, self.scheme, self.pos_end = lib, scheme, np.asarray(pos_end, np.int64)
        self.n = len(pos_end)
        self.handles, self.failures = [], []
        for i, e in enumerate(self.pos_end):
            self.handles.append(allocation(lib, scheme, 256, hostile(256, (0, int(e)), range(L)), migrate=i == migrate_member))
        self.qh = (np.random.default_rng(seed).standard_normal((L, self.n, H, G, D)) * 1.5).astype(np.float16)
        self.q = torch.from_numpy(self.qh).cuda()
        torch.cuda.synchronize()

    def check(self, oracle, out, lse, layer, what, members=None, tail=None):
        members = np.arange(self.n) if members is None else np.asarray(members)
        pos_end = self.pos_end[members]
        empty = (pos_end == 0) if tail is None else np.zeros(len(members), bool)
        worst, first = [], None
        hc = checker(oracle, self.scheme, 256, layer)
        for head in range(H):
            tl = None if tail is None else (tail[0][members, layer, head], tail[1][members, layer, head])
            try:
                hc.check_rows(out[:, head], lse[:, head], self.qh[layer][members, head], head, pos_end, SM, what + (layer, head), tl, worst=worst)
            except AssertionError as ex:
                first = first or ex.args[0]
        print(f"hostile batch {what} layer {layer}: worst err/tol {max(worst):.3f}")
        if not (np.isfinite(out).all() and np.isfinite(lse[~empty]).all() and np.all(lse[empty] == -np.inf)):
            first = first or (what, layer, "out / lse not finite (an empty member: lse -inf)")
        if first is not None:
            self.failures.append((first, f"worst err/tol {max(worst):.3f}"))
        return max(worst)

    def free(self):
        for h in self.handles:
            self.lib.free(h)
        self.handles = []


@pytest.mark.parametrize("scheme,placement,variant", BATCH_CASES, ids=[f"{p}-{NAMES[s]}-{v}" for s, p, v in BATCH_CASES])
def test_batch_and_planned_entries(oracle, scheme, placement, variant):
    """attend_*_batch and attend_batch_plan + attend_planned over six members of pos_end 0, 2, 70, 96, 254, 256 in allocations of 256
    positions, everything at or behind a member's end hostile (whole stale tiles included), both layers; the form asserted on the host first."""
    torch = torch_mod()
    rules = load_rules()
    lib = engine(placement)
    n = len(POS_END)
    batch = Batch(lib, scheme, POS_END, 9300 + scheme, migrate_member=3 if placement == "migrated" else None)
    entry = {FP8: lib.attend_fp8_batch, INT4: lib.attend_int4_batch, MX4: lib.attend_mx4_batch}[scheme]
    lens = POS_END.astype(np.uint32)
    body = BATCH[(scheme, placement, variant)][0]
    overall = 0.0
    try:
        with tuned(BATCH_VARIANTS[variant][0]):
            assert_form(rules, scheme, placement, variant, "batch", POS_END)
            for layer in range(L):
                out, lse = fresh((n, H), torch)
                entry(batch.handles, layer, batch.q[layer].data_ptr(), G, lens, SM, out.data_ptr(), lse.data_ptr())
                torch.cuda.synchronize()
                overall = max(overall, batch.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), layer, (body, placement, variant, "batch")))
            if (scheme, placement, variant) == (MX4, "one", "default"):     # the batch entry on the halves form: the members that are not empty
                live = np.nonzero(POS_END)[0]
                assert_form(rules, scheme, placement, variant, "batch", POS_END[live])
                q = batch.q[0][torch.from_numpy(live).cuda()].contiguous()
                out, lse = fresh((len(live), H), torch)
                entry([batch.handles[i] for i in live], 0, q.data_ptr(), G, lens[live], SM, out.data_ptr(), lse.data_ptr())
                torch.cuda.synchronize()
                overall = max(overall, batch.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), 0, (body, placement, variant, "batch, no empty member"), members=live))
            assert_form(rules, scheme, placement, variant, "plan", POS_END, max_pos_end=256)
            st = torch.cuda.Stream()
            plan_bytes = lib.attend_plan_bytes(n)
            plan = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            lib.attend_batch_plan(batch.handles, lens, 256, plan.data_ptr(), plan_bytes, st.cuda_stream)
            for layer in range(L):
                out, lse = fresh((n, H), torch)
                torch.cuda.synchronize()
                lib.attend_planned(scheme, plan.data_ptr(), n, layer, batch.q[layer].data_ptr(), G, 256, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
                st.synchronize()
                overall = max(overall, batch.check(oracle, out.cpu().numpy(), lse.cpu().numpy(), layer, (body, placement, variant, "planned")))
    finally:
        batch.free()
    print(f"hostile batch {placement}-{NAMES[scheme]}-{variant}: worst err/tol over all cases {overall:.3f}, {len(batch.failures)} cases failed")
    assert not batch.failures, batch.failures[:6]


def test_planned_layers_with_tails_over_hostile_rows(oracle):
    """attend_planned_layers over MXFP4, both layers in one launch, a tail row per member folded in by the kernel (no empty member), every
    member hostile behind its end in both layers: the halves form k_attend_mx4<0, 2> with its in-kernel fold."""
    torch = torch_mod()
    rules = load_rules()
    lib = engine("one")
    n = len(TAIL_LENS)
    d = decide(rules, MX4, "plan", TAIL_LENS // 2, cus(), max_pos_end=256)
    assert (d["table"], d["striped"], d["max_splits"]) == (0, 0, 1) and n <= cus()      # one launch over layers x members, the halves form
    batch = Batch(lib, MX4, TAIL_LENS, 9400)
    try:
        rng = np.random.default_rng(9401)
        kt = (rng.standard_normal((n, L, H, D)) * 1.5).astype(np.float16)
        vt = rng.standard_normal((n, L, H, D)).astype(np.float16)
        d_kt, d_vt = torch.from_numpy(kt).cuda(), torch.from_numpy(vt).cuda()
        st = torch.cuda.Stream()
        plan_bytes = lib.attend_plan_bytes(n)
        plan = torch.zeros(plan_bytes, dtype=torch.uint8, device="cuda")
        out, lse = fresh((L, n, H), torch)
        torch.cuda.synchronize()
        lib.attend_batch_plan(batch.handles, TAIL_LENS.astype(np.uint32), 256, plan.data_ptr(), plan_bytes, st.cuda_stream)
        lib.attend_planned_layers(MX4, plan.data_ptr(), n, 0, L, batch.q.data_ptr(), G, 256, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream,
                                  n_tail=n, d_k_tail=d_kt.data_ptr(), d_v_tail=d_vt.data_ptr(), tail_stride_elems=L * H * D)
        st.synchronize()
        o, l = out.cpu().numpy(), lse.cpu().numpy()
        for layer in range(L):
            batch.check(oracle, o[layer], l[layer], layer, ("k_attend_mx4<0, 2>", "one", "planned layers with tails"), tail=(kt, vt))
    finally:
        batch.free()
    assert not batch.failures, batch.failures[:6]


# ----------------------------------------------------------------------------- FP8: stale V of any finite magnitude
@pytest.mark.parametrize("v_mag", [8000.0, 60000.0])
def test_fp8_stale_v_scale_stays_out_of_the_tile_reference(oracle, v_mag):
    """The FP8 tile kernels round their weights to fp16 in units of the tile's largest V page scale.  A stale page in a ragged first or last
    tile must not set that unit: with V = 60000 behind the cut (the largest fp16 magnitude a page can hold, a page scale of 134 against
    0.002 .. 0.03 of the kept pages) the kept positions' weights would sink into the fp16 subnormals, 2^-24 x 134 x |v code| <= 3.6e-3 absolute
    per position.  Same bound as everywhere in this file; one pool, both linear bodies, a range with stale pages behind and one with stale
    pages on both sides."""
    torch = torch_mod()
    lib = engine("one")
    T = 256
    rng = np.random.default_rng(9500)
    qh = (rng.standard_normal((L, H, G, D)) * 1.5).astype(np.float16)
    q = torch.from_numpy(qh).cuda()
    h = allocation(lib, FP8, T, base(T))
    failures = []
    try:
        for b, e in ((0, 70), (34, 100)):
            x = hostile(T, (b, e), (0,), v_mag=v_mag)
            lib.write(h, 0, x.ctypes.data, x.nbytes, False)
            for tuning in single_tunings("one", FP8):
                out, lse = fresh((1, H), torch)
                with tuned(tuning):
                    lib.attend_fp8(h, 0, 1, q.data_ptr(), G, b, e, SM, out.data_ptr(), lse.data_ptr())
                    torch.cuda.synchronize()
                check_single(oracle, FP8, T, out.cpu().numpy(), lse.cpu().numpy(), qh, b, e, ("one", "fp8", T, tuning, (b, e), f"stale V {v_mag:g}"), failures)
    finally:
        lib.free(h)
    assert not failures, failures[:6]
