"""-m gpu: the split pool's multi-position step ON A SLIDING-WINDOW LAYER -- speckv_ext_attend_kv_spec_window (k_attend_k8v4<true, true>: every
member walked from the tile of depth 0's window bound, the stored positions masked PER QUERY ROW by its node's depth, the rows held outside
the pool folded in by split 0) and SpeckvSplitKVConnector.attend_spec(window=W) on top of it.

Conventions: a member has `length` committed positions, stored = length & ~1 of them in the pool, an odd length its last one as held
position 0; a draft node of depth d sits at length + d and sees [lo(d), length + d], lo(d) = max(0, length + d + 1 - W)
(csrc/spec_window.hpp).  Every member has its OWN pair of allocations, written through write_prefill, and every position in front of
lo(0) -- in front of every row's window -- is hostile (K x 200, V = +-1000; tests/test_gpu_decode_window.py content): an odd lo(0) puts a
hostile row into a kept position's FP8 page scale and MXFP4 block code.

Reference: numpy float64 attention over the VISIBLE positions only -- per row the oracle's records of [lo(depth), stored) (K from
HeadChecker(oracle, FP8) with the query through q_rows, E4M3 x a row scale; V from HeadChecker(oracle, MXFP4)) and the held positions its
mask word shows (fp16 query, fp16 rows).  Bound: tests/test_gpu_k8v4_spec.py's _want bound, the project's for 8-bit-query kernels
(tests/_gpu.py check_rows), over the visible set: |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta = 3e-5 max
sum |q||k| sm over the visible stored and held positions of the rows of a (member, head).  Every (member, head, row) is compared; a row
that sees nothing is exactly 0 with lse -inf.  Geometry: L = 2, T = 256, H = 8, D = 128.  The worst err / tol of a case is printed before
anything is asserted."""
import contextlib
import itertools
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, decide, load_rules
from tests.test_gpu_decode_window import checker, content
from tests.test_gpu_hostile_ranges import drop_engine
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
L, T = 2, 256
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19
FP8, MX4 = 4, 5
LENGTHS = [0, 1, 2, 31, 32, 33, 64, 97, 254, 60, 61]       # 60, 61 under W = 33: lo(0) = 28, 29 -- with 16 depths a skip of 43, 44, inside tile 1
WINDOWS = [1, 2, 3, 17, 33, 40, 300]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_rids = itertools.count(1)
_steps = {}


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    drop_engine()
    _steps.clear()


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


def lo_of(length, depth, window):
    return max(0, length + depth + 1 - window) if window else 0


def _step(B, S, R, seed=0):
    """the step's query [B][S][H][R][D] and new rows [B][S][L][H][D] (K, V), once per shape"""
    key = (B, S, R, seed)
    if key not in _steps:
        rng = np.random.default_rng(5200 + 1000 * B + 100 * S + R + 7 * seed)
        rows = lambda *shape: rng.standard_normal(shape).astype(np.float16)
        _steps[key] = (rows(B, S, H, R, D), rows(B, S, L, H, D), rows(B, S, L, H, D))
    return _steps[key]


def _rows_of(q5):
    """[B][S][H][R][D] -> the entry's [B][H][S * R][D]"""
    Bq, S, _, R, _ = q5.shape
    return np.ascontiguousarray(q5.transpose(0, 2, 1, 3, 4).reshape(Bq, H, S * R, D))


class Members:
    """a batch under one window: per member its own request with its hostile content (or the rows given), the tails of the odd lengths"""

    def __init__(self, conn, lengths, window, seed, rows=None):
        torch = torch_mod()
        self.conn, self.window, self.lengths = conn, window, [int(n) for n in lengths]
        self.n = len(lengths)
        self.stored = [n & ~1 for n in self.lengths]
        self.spans = [(min(lo_of(n, 0, window), n & ~1), n & ~1) for n in self.lengths]
        rng = np.random.default_rng(seed)
        self.rids, self.tails, self.own, keep = [], [], rows, []
        for i, (n, (lo, stored)) in enumerate(zip(self.lengths, self.spans)):
            x = (content(lo, stored) if rows is None else rows[i]).reshape(L, 2, T, H, D)[:, :, :n]
            k, v = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])
            tail = None
            if n & 1:                                                          # the tail is an ordinary row: every depth below W - 1 sees it
                tail = (rng.standard_normal((L, H, D)).astype(np.float16), rng.standard_normal((L, H, D)).astype(np.float16))
                k[:, -1], v[:, -1] = tail
            rid = next(_rids)
            conn.add_request(rid)
            if n:
                keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
            self.rids.append(rid)
            self.tails.append(tail)
        torch.cuda.synchronize()
        del keep
        reqs = [conn.requests[r] for r in self.rids]
        assert [r.length for r in reqs] == self.lengths
        self.kh = np.asarray([r.k_handle for r in reqs], np.uint64)
        self.vh = np.asarray([r.v_handle for r in reqs], np.uint64)

    def pair(self, oracle, layer, i):
        if self.own is not None:
            key = ("own", id(self.own), layer, i)
            if key not in _steps:
                _steps[key] = (HeadChecker(oracle, FP8, self.own[i][layer * T:(layer + 1) * T], T), HeadChecker(oracle, MX4, self.own[i][layer * T:(layer + 1) * T], T))
            return _steps[key]
        lo, stored = self.spans[i]
        return checker(oracle, FP8, layer, lo, stored), checker(oracle, MX4, layer, lo, stored)

    def held(self, layer, k_new, v_new):
        """[B][1 + S][H][D] fp16 per kind -- the odd last position first where there is one, then the new positions; the slots behind them
        are NaN (nothing may read them) -- and base [B]"""
        S = k_new.shape[1]
        kh, vh = np.full((self.n, 1 + S, H, D), np.nan, np.float16), np.full((self.n, 1 + S, H, D), np.nan, np.float16)
        base = [n & 1 for n in self.lengths]
        for b, tail in enumerate(self.tails):
            if tail is not None:
                kh[b, 0], vh[b, 0] = tail[0][layer], tail[1][layer]
            kh[b, base[b]:base[b] + S], vh[b, base[b]:base[b] + S] = k_new[b, :, layer], v_new[b, :, layer]
        return kh, vh, base

    def want(self, oracle, layer, qg, R, kh, vh, words, depths, shift=0, window=None):
        """float64: out [B][H][G][D], lse [B][H][G], tol, ltol of qg [B][H][G][D]: row r over the stored positions [lo(depth) + shift, stored)
        and the held positions its word shows (shift: the needle test's mask one position off, on the stored part)"""
        W = self.window if window is None else window
        G = qg.shape[2]
        out, lse = np.zeros((self.n, H, G, D)), np.full((self.n, H, G), -np.inf)
        tol, ltol = np.full((self.n, H, G, D), 1e-6), np.full((self.n, H, G), 2e-3)
        for m in range(self.n):
            k8, v4 = self.pair(oracle, layer, m)
            n = self.stored[m]
            for head in range(H):
                K, V = k8.kv(head)[0], v4.kv(head)[1]
                qe = k8.q_rows(qg[m:m + 1, head]).reshape(G, D)
                qf = qg[m, head].astype(np.float64)
                top = max((int(w).bit_length() for w in words[m]), default=0)
                kf, vf = kh[m, :top, head].astype(np.float64), vh[m, :top, head].astype(np.float64)
                rows, peak = [], 0.0
                for r in range(G):
                    first = min(max(0, lo_of(self.lengths[m], min(int(depths[m][r // R]), 15), W) + shift), n)
                    seen = [t for t in range(top) if (int(words[m][r // R]) >> t) & 1]
                    rows.append((first, seen))
                    peak = max(peak, float((np.abs(qe[r]) @ np.abs(K[first:n]).T).max(initial=0.0)), float((np.abs(qf[r]) @ np.abs(kf[seen]).T).max(initial=0.0)))
                delta = 3e-5 * peak * SM
                for r, (first, seen) in enumerate(rows):
                    s = np.concatenate([(K[first:n] @ qe[r]) * SM, (kf[seen] @ qf[r]) * SM])
                    if len(s) == 0:
                        continue
                    vals = np.concatenate([V[first:n], vf[seen]])
                    mx = s.max()
                    p = np.exp(s - mx)
                    out[m, head, r], lse[m, head, r] = (p @ vals) / p.sum(), mx + np.log(p.sum())
                    tol[m, head, r] = (2e-3 + 2 * delta) * ((p @ np.abs(vals)) / p.sum()) + 1e-6
                    ltol[m, head, r] = 2e-3 + delta
        return out, lse, tol, ltol

    def entry(self, layer, qg, R, kh, vh, words, depths, with_lse=True, on=None, plain=False, **change):
        """speckv_ext_attend_kv_spec_window itself (plain: speckv_ext_attend_kv_spec over the same arguments) -> (out, lse) as fp32 numpy and
        the raw lse words; both start as the fill pattern"""
        torch = torch_mod()
        Bq, _, G, _ = qg.shape
        st = on if on is not None else torch.cuda.Stream()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dk, dv = dev(qg), dev(kh), dev(vh)
        dm, dd = dev(np.asarray(words, np.uint32).view(np.int32)), dev(np.asarray(depths, np.uint32).view(np.int32))
        out = torch.full((Bq, H, G, D), PATTERN, dtype=torch.int32, device="cuda")
        lse = torch.full((Bq, H, G), PATTERN, dtype=torch.int32, device="cuda")
        args = dict(k_handles=self.kh, v_handles=self.vh, layer=layer, d_q_f16=dq.data_ptr(), g=G, rows_per_pos=R, pos_end=np.asarray(self.stored, np.uint32),
                    length=np.asarray(self.lengths, np.uint32), d_depth=dd.data_ptr(), window=self.window, d_k_held=dk.data_ptr(), d_v_held=dv.data_ptr(),
                    seq_stride_elems=kh.shape[1] * H * D, pos_stride_elems=H * D, d_mask=dm.data_ptr(), mask_stride=dm.shape[1], sm_scale=SM,
                    d_out=out.data_ptr(), d_lse=lse.data_ptr() if with_lse else 0, stream=st.cuda_stream)
        args.update(change)
        if plain:
            for name in ("length", "d_depth", "window"):
                del args[name]
        torch.cuda.synchronize()
        try:
            (self.conn.lib.attend_kv_spec if plain else self.conn.lib.attend_kv_spec_window)(**args)
        finally:
            torch.cuda.synchronize()
        return out.cpu().numpy().view(np.float32), (lse.cpu().numpy().view(np.float32) if with_lse else None)

    def free(self):
        for rid in self.rids:
            self.conn.free_request(rid)
        self.rids = []


def _compare(want, out, lse, what):
    """-> worst err / tol over every (member, head, row); rows that see nothing are exactly 0 / -inf; nothing is NaN"""
    w_out, w_lse, tol, ltol = want
    nothing = np.isneginf(w_lse)
    assert not np.isnan(out).any() and (lse is None or not np.isnan(lse).any()), (what, "NaN")
    assert not (out.view(np.uint32) == PATTERN).any(), (what, "rows keep the fill pattern")
    assert not out[nothing].any(), (what, "a row that sees nothing is exactly 0")
    err = np.abs(out.astype(np.float64) - w_out)
    worst = float(np.nan_to_num(err / tol, nan=np.inf).max())
    if lse is not None:
        assert np.all(np.isneginf(lse[nothing])), (what, "a row that sees nothing has lse -inf")
        with np.errstate(invalid="ignore"):
            lerr = np.where(nothing, 0.0, np.abs(lse.astype(np.float64) - w_lse))
        worst = max(worst, float(np.nan_to_num(lerr / ltol, nan=np.inf).max()))
    print(f"{what}: worst err / tol {worst:.3f}")
    assert worst <= 1.0, (what, worst, np.argwhere(np.nan_to_num(err / tol, nan=np.inf) > 1.0)[:4])
    return worst


def _chain(S):
    return list(range(-1, S - 1))


def _tables(parents, base, n, window, n_new=None):
    """(mask words, depths) [n][S] of the step as the connector derives them"""
    return SpeckvKVConnector.tree_masks(parents, base, n_new, window=window or None), SpeckvKVConnector.chunk_tree_depths(parents, n)


# ----------------------------------------------------------------------------- 1. chains through the connector, every window
SHAPES = [(1, 1), (4, 4), (2, 8), (16, 1), (5, 4), (3, 8)]


@pytest.mark.parametrize("window", WINDOWS)
def test_chains_under_windows(oracle, window):
    """attend_spec(window=W) of a causal chain over the eleven lengths, every (S, R): (1, 1), (4, 4), (2, 8), (16, 1) are one group, (5, 4)
    and (3, 8) two -- the second group starts at the same tile as the first and carries deeper rows only.  (4, 4) on both layers, the others
    on one.  W = 2 on an even length is a cut page; W = 300 cuts nobody: the bits of attend_spec without a window."""
    torch = torch_mod()
    B = len(LENGTHS)
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS, window, 7100 + window)
        worst = 0.0
        for i, (S, R) in enumerate(SHAPES):
            q5, k_new, v_new = _step(B, S, R)
            dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
            for layer in (range(L) if (S, R) == (4, 4) else [i % L]):
                got = conn.attend_spec(layer, m.rids, dq, dk, dv, SM, window=window)
                torch.cuda.synchronize()
                assert tuple(got.shape) == (B, S, H, R, D) and got.dtype == torch.float32
                kh, vh, base = m.held(layer, k_new, v_new)
                words, depths = _tables(_chain(S), base, B, window)
                want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths)
                worst = max(worst, _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec(window={window}) chain S {S} R {R} layer {layer}"))
                if window == 300:
                    plain = conn.attend_spec(layer, m.rids, dq, dk, dv, SM)
                    torch.cuda.synchronize()
                    assert np.array_equal(plain.cpu().numpy().view(np.uint32), got.cpu().numpy().view(np.uint32)), (S, R, layer)
        assert [conn.length(r) for r in m.rids] == LENGTHS                         # no state moved
    print(f"k8v4 spec window W = {window}: worst err / tol {worst:.3f}")


def test_a_window_that_cuts_nobody_is_the_plain_entry_bit_for_bit():
    """window = 0 (length and d_depth NULL as well), W = 300 and W = 270 = the longest length + 16: the rows and the lse of
    speckv_ext_attend_kv_spec bit for bit; W = 256 cuts the longest member alone (depths 2 and 3 lose positions 0 and 0..1) and leaves every
    other member's bits"""
    torch = torch_mod()
    S, R, B = 4, 4, len(LENGTHS)
    q5, k_new, v_new = _step(B, S, R)
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS, 300, 7190)
        kh, vh, base = m.held(1, k_new, v_new)
        words, depths = _tables(_chain(S), base, B, None)
        po, pl = m.entry(1, _rows_of(q5), R, kh, vh, words, depths, plain=True)
        assert not (po.view(np.uint32) == PATTERN).any()
        for how in (dict(window=0), dict(window=0, length=None, d_depth=0), dict(window=300), dict(window=270), dict(window=2 ** 32 - 1)):
            out, lse = m.entry(1, _rows_of(q5), R, kh, vh, words, depths, **how)
            assert np.array_equal(out.view(np.uint32), po.view(np.uint32)) and np.array_equal(lse.view(np.uint32), pl.view(np.uint32)), how
        out, lse = m.entry(1, _rows_of(q5), R, kh, vh, words, depths, window=256)
        i = LENGTHS.index(254)
        others = [b for b in range(B) if b != i]
        assert np.array_equal(out[others].view(np.uint32), po[others].view(np.uint32)) and np.array_equal(lse[others].view(np.uint32), pl[others].view(np.uint32))
        assert np.array_equal(lse[i, :, :2 * R].view(np.uint32), pl[i, :, :2 * R].view(np.uint32))       # depths 0 and 1 still see position 0
        assert np.all(lse[i, :, 2 * R:] < pl[i, :, 2 * R:])


# ----------------------------------------------------------------------------- 2. rel < 0: shallow rows see everything, deep rows are cut
def test_a_window_that_has_not_left_position_0(oracle):
    """length 20, W = 28, S = 16: rel = -7 -- depths 0..7 see every stored position, depth 8 + j loses the first j + 1"""
    torch = torch_mod()
    S, R = 16, 1
    lengths = [20, 21, 0, 12]
    q5, k_new, v_new = _step(len(lengths), S, R)
    assert SpeckvKVConnector.spec_window_range(20, 28) == (0, -7, 10)
    with _pool(torch) as (lib, conn):
        m = Members(conn, lengths, 28, 7200)
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(_chain(S), base, len(lengths), 28)
            out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths)
            _compare(m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths), out, lse, f"attend_kv_spec_window rel < 0 layer {layer}")


# ----------------------------------------------------------------------------- 3. trees
TREE = [-1, 0, 1, 2, 0, 4, 5]                # node 0, then two branches of three


@pytest.mark.parametrize("window", [33, 3])
def test_a_tree_of_two_branches(oracle, window):
    """7 nodes, rows_per_pos 4: two groups (nodes 0..3, nodes 4..6).  Node 4 has depth 1, not 4: its stored bound is depth 1's.  W = 3 cuts
    ancestors in the words (node 3 of depth 3 no longer sees node 0, nobody deeper than 1 sees the tail).  A reference that took the
    node INDEX for the depth is further than the tolerance from the tree's under W = 33."""
    torch = torch_mod()
    S, R, B = len(TREE), 4, len(LENGTHS)
    q5, k_new, v_new = _step(B, S, R)
    v_new = v_new.copy()
    v_new[:, 4:] += np.float16(6.0)                                                  # the second branch's values stand apart
    with _pool(torch) as (lib, conn):
        m = Members(conn, LENGTHS, window, 7300 + window)
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(TREE, base, B, window)
            assert depths[0] == [0, 1, 2, 3, 1, 2, 3]
            if window == 3:
                assert words[1] == [0b11, 0b111, 0b1110, 0b11100, 0b100011, 0b1100010, 0b11100000]       # base 1
            want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths)
            if window == 33:
                by_index = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, [list(range(S))] * B)
                i = LENGTHS.index(97)                                                # lo(0) = 65: hostile rows right in front of the window
                assert (np.abs(by_index[0] - want[0])[i, :, 4 * R:] / want[2][i, :, 4 * R:]).max() > 10.0
            got = conn.attend_spec(layer, m.rids, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, parents=TREE, window=window)
            torch.cuda.synchronize()
            _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec(window={window}) tree layer {layer}")


# ----------------------------------------------------------------------------- 4. a ragged step
def test_a_ragged_step_and_its_dead_rows(oracle):
    """n_new 0..S mixed over the members, a chain and the tree: a dead node's rows are the stored positions its depth's window shows,
    finite; the member with nothing stored and the members no row of which sees the pool (W = 3 on length 1, 2) give exactly 0 / -inf"""
    torch = torch_mod()
    B = len(LENGTHS)
    with _pool(torch) as (lib, conn):
        for window in (33, 3):
            m = Members(conn, LENGTHS, window, 7400 + window)
            for parents, R, n_new in ((_chain(4), 4, [0, 2, 4, 0, 1, 3, 4, 0, 2, 0, 3]), (TREE, 2, [7, 0, 5, 2, 7, 1, 6, 4, 3, 0, 7])):
                S = len(parents)
                q5, k_new, v_new = _step(B, S, R)
                for layer in range(L):
                    kh, vh, base = m.held(layer, k_new, v_new)
                    words, depths = _tables(parents, base, B, window, n_new)
                    assert n_new.count(0) >= 2 and all(words[b] == [0] * S for b in range(B) if n_new[b] == 0)
                    want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths)
                    got = conn.attend_spec(layer, m.rids, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, n_new=n_new, parents=parents, window=window)
                    torch.cuda.synchronize()
                    assert np.isfinite(got.cpu().numpy()).all()
                    _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec(window={window}) ragged S {S} layer {layer}")
                    if S * R <= 16:
                        out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths)
                        _compare(want, out, lse, f"attend_kv_spec_window ragged S {S} layer {layer}")
                        if n_new[0] == 0:
                            assert not out[0].any() and np.all(np.isneginf(lse[0]))     # nothing stored, nothing seen
                        assert not (lse.view(np.uint32) == PATTERN).any()
            m.free()


# ----------------------------------------------------------------------------- 5. pieces and the merge: rows that see nothing of a piece
MERGE_W = 15
MERGE_LENGTHS = [66, 98, 100, 0, 33, 254, 67]


@pytest.mark.parametrize("as_given", [0, 1])
def test_rows_masked_throughout_a_piece_survive_the_merge(oracle, as_given):
    """attend_tiles_per_split = 1, both dispatch orders, S = 16 under W = 15.  Length 66: begin 32, rel 20, 17 pages -- the second tile holds
    a single page (positions 64, 65) and the rows of depth >= 14 (skip >= 34) see nothing of it: their partial of piece 1 is (-inf, 0),
    and depth 15 sees nothing stored at all.  Length 100: begin 64, rel 22, 18 pages -- the rows of depth >= 10 are masked throughout piece
    0 and see positions of piece 1.  tests/_rules.py confirms first that the engine cuts the members into these pieces."""
    torch = torch_mod()
    S, R, B = 16, 1, len(MERGE_LENGTHS)
    ranges = [SpeckvKVConnector.spec_window_range(n, MERGE_W) for n in MERGE_LENGTHS]
    assert ranges[0] == (32, 20, 17) and ranges[1] == (64, 20, 17) and ranges[2] == (64, 22, 18) and ranges[3][2] == 0 and ranges[6] == (32, 21, 17)
    assert SpeckvKVConnector.spec_window_skip(20, 14) == 34 and SpeckvKVConnector.spec_window_skip(22, 10) == 32
    pages = np.asarray([r[2] for r in ranges])
    tiles = (pages + 15) // 16
    d = decide(load_rules(), FP8, "batch", pages, _cus(), tuning=(1, as_given) + DEFAULT_TUNING[2:])
    assert d["fits"] == 1 and d["tps"] == 1 and d["max_splits"] == int(tiles.max()) == 2 and not d["table"] and not d["striped"], d
    assert [int(x) for x in d["pieces"][:, 1]] == [int(t) for t in tiles] and d["by_length"] == (0 if as_given else 1)
    q5, k_new, v_new = _step(B, S, R)
    with _pool(torch) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", 1)
            set_tuning("attend_order_as_given", as_given)
            m = Members(conn, MERGE_LENGTHS, MERGE_W, 7500)
            for layer in range(L):
                kh, vh, base = m.held(layer, k_new, v_new)
                words, depths = _tables(_chain(S), base, B, MERGE_W)
                want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths)
                out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths)
                _compare(want, out, lse, f"attend_kv_spec_window pieces of one tile, as given {as_given}, layer {layer}")
                # ... and with the held positions away (words 0): the rows of depth 15 of length 66 see nothing at all
                none = [[0] * S] * B
                out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, none, depths)
                want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, none, depths)
                assert np.all(np.isneginf(want[1][0, :, 15])) and np.all(np.isfinite(want[1][0, :, 13]))
                _compare(want, out, lse, f"attend_kv_spec_window pieces, nothing held, as given {as_given}, layer {layer}")
        finally:
            set_tuning("attend_tiles_per_split", 0)
            set_tuning("attend_order_as_given", 0)


# ----------------------------------------------------------------------------- 6. needles at every depth's bound
def _hadamard(n):
    h = np.ones((1, 1))
    while len(h) < n:
        h = np.block([[h, h], [h, -h]])
    return h


NEEDLE_LENGTHS, NEEDLE_W = [97, 60, 61, 254], 33           # lo(0) = 65, 28, 29, 222


def _needle_rows(length):
    """the member's content: position lo(d) = lo(0) + d holds K = u_d + 1.6 u_(d+1) for orthogonal +-1 directions u -- row d, whose query
    lies along u_d, scores 11.3 there (nearly all its weight) and would score 18.1 at lo(d) - 1, which row d - 1 sees and row d must not;
    the V rows of these positions stand apart (+-4 patterns)."""
    lo0, stored = lo_of(length, 0, NEEDLE_W), length & ~1
    x = content(lo0, stored).copy().reshape(L, 2, T, H, D)
    u = _hadamard(D)[1:19]                                                          # u_(-1) .. u_16
    for j in range(-1, 16):
        x[:, 0, lo0 + j] = (u[j + 1] + 1.6 * u[j + 2]).astype(np.float16)
        x[:, 1, lo0 + j] = (4.0 * _hadamard(D)[40 + j]).astype(np.float16)
    return x.reshape(L * T, 2 * H * D), u[1:17]


def test_needles_at_the_bound_of_every_depth(oracle):
    """a 16-chain: a mask one position off in either direction at ANY depth is more than 10 x the tolerance away (asserted on the CPU
    before the launch); lo(0) = 65 and 222 (tile 0 of the walk only), 28 and 29 (skips 28 .. 44: the mask reaches into tile 1)"""
    torch = torch_mod()
    S, R, B = 16, 1, len(NEEDLE_LENGTHS)
    made = [_needle_rows(n) for n in NEEDLE_LENGTHS]
    rng = np.random.default_rng(7600)
    q5 = np.stack([(dirs[:, None, None, :] + 0.3 * rng.standard_normal((S, H, R, D))).astype(np.float16) for _, dirs in made])
    _, k_new, v_new = _step(B, S, R)
    with _pool(torch) as (lib, conn):
        m = Members(conn, NEEDLE_LENGTHS, NEEDLE_W, 7610, rows=[rows for rows, _ in made])
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(_chain(S), base, B, NEEDLE_W)
            want = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths)
            for shift in (-1, 1):
                off = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths, shift=shift)
                apart = (np.abs(off[0] - want[0]) / want[2]).max(axis=3)             # [B][H][G]
                assert apart.min() > 10.0, (shift, float(apart.min()), np.argwhere(apart <= 10.0)[:4])
            out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths)
            _compare(want, out, lse, f"attend_kv_spec_window needles layer {layer}")


# ----------------------------------------------------------------------------- 7. refusals, streams
def test_refusals_launch_nothing():
    """every refusal of the entry on the GPU engine is SPECKV_ERR_INVAL, a capturing stream included, and d_out keeps its fill pattern"""
    torch = torch_mod()
    S, R = 2, 4
    lengths = [64, 33, 0, 97]
    q5, k_new, v_new = _step(len(lengths), S, R)
    with _pool(torch) as (lib, conn):
        m = Members(conn, lengths, 33, 7700)
        kh, vh, base = m.held(0, k_new, v_new)
        kh, vh = np.nan_to_num(kh), np.nan_to_num(vh)
        words, depths = _tables(_chain(S), base, len(lengths), 33)
        with_at = lambda a, b, x: np.concatenate([a[:b], np.asarray([x], a.dtype), a[b + 1:]])
        ln, pe = np.asarray(lengths, np.uint32), np.asarray(m.stored, np.uint32)
        bad = [dict(length=None), dict(d_depth=0), dict(length=with_at(ln, 0, 66)), dict(length=with_at(ln, 1, 31)), dict(length=with_at(ln, 2, 2)),
               dict(pos_end=with_at(pe, 3, 98), length=with_at(ln, 3, 97)),
               dict(rows_per_pos=0), dict(rows_per_pos=3), dict(g=17, rows_per_pos=1, mask_stride=17), dict(d_k_held=0), dict(d_v_held=0), dict(d_mask=0),
               dict(mask_stride=1), dict(seq_stride_elems=3 * H * D + 4), dict(pos_stride_elems=H * D - 8), dict(g=0), dict(g=20), dict(layer=L),
               dict(pos_end=with_at(pe, 1, 33), length=with_at(ln, 1, 33))]
        for change in bad:
            with pytest.raises(SpeckvError) as e:
                m.entry(change.pop("layer", 0), _rows_of(q5), R, kh, vh, words, depths, **change)
            assert e.value.status == -4, change
        # nothing was written: the same call shape with a watched output
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dk, dv = dev(_rows_of(q5)), dev(kh), dev(vh)
        dm, dd = dev(np.asarray(words, np.uint32).view(np.int32)), dev(np.asarray(depths, np.uint32).view(np.int32))
        out = torch.full((len(lengths), H, S * R, D), PATTERN, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        good = dict(k_handles=m.kh, v_handles=m.vh, layer=0, d_q_f16=dq.data_ptr(), g=S * R, rows_per_pos=R, pos_end=pe, length=ln, d_depth=dd.data_ptr(), window=33,
                    d_k_held=dk.data_ptr(), d_v_held=dv.data_ptr(), seq_stride_elems=(1 + S) * H * D, pos_stride_elems=H * D, d_mask=dm.data_ptr(), mask_stride=S,
                    sm_scale=SM, d_out=out.data_ptr(), d_lse=0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for change in (dict(length=None), dict(d_depth=0), dict(length=with_at(ln, 0, 66)), dict(d_mask=0), dict(g=20)):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec_window(**dict(good, **change))
            assert e.value.status == -4, change
        capturing = torch.cuda.Stream()
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with graph_capture(graph, capturing):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec_window(**dict(good, stream=capturing.cuda_stream))
            assert e.value.status == -4
            bump.add_(1)
        del graph
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == PATTERN).all()
        lib.attend_kv_spec_window(**good)                                             # and the good set goes through
        torch.cuda.synchronize()
        assert not (out.cpu().numpy().view(np.uint32) == PATTERN).any()


def test_two_calls_on_two_streams(oracle):
    torch = torch_mod()
    S, R = 4, 4
    lengths = [254, 97, 60, 0, 33]
    B = len(lengths)
    q5, k_new, v_new = _step(B, S, R)
    q5b = _step(B, S, R, seed=1)[0]
    with _pool(torch) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", 1)                                  # both calls leave partials in the one scratch buffer
            m = Members(conn, lengths, 40, 7800)
            kh, vh, base = m.held(1, k_new, v_new)
            words, depths = _tables(_chain(S), base, B, 40)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            dk, dv = dev(kh), dev(vh)
            dm, dd = dev(np.asarray(words, np.uint32).view(np.int32)), dev(np.asarray(depths, np.uint32).view(np.int32))
            streams, qs, outs = [torch.cuda.Stream(), torch.cuda.Stream()], [dev(_rows_of(q5)), dev(_rows_of(q5b))], []
            torch.cuda.synchronize()
            for st, dq in zip(streams, qs):
                out = torch.full((B, H, S * R, D), PATTERN, dtype=torch.int32, device="cuda")
                lse = torch.full((B, H, S * R), PATTERN, dtype=torch.int32, device="cuda")
                outs.append((out, lse))
                lib.attend_kv_spec_window(m.kh, m.vh, 1, dq.data_ptr(), S * R, R, np.asarray(m.stored, np.uint32), np.asarray(lengths, np.uint32), dd.data_ptr(), 40,
                                          dk.data_ptr(), dv.data_ptr(), (1 + S) * H * D, H * D, dm.data_ptr(), S, SM, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            for q, (out, lse), name in zip((q5, q5b), outs, "ab"):
                want = m.want(oracle, 1, _rows_of(q), R, kh, vh, words, depths)
                _compare(want, out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32), f"attend_kv_spec_window two streams, call {name}")
        finally:
            set_tuning("attend_tiles_per_split", 0)


# ----------------------------------------------------------------------------- 8. the example, and a walk through the connector
def test_the_example_runs():
    """examples/k8v4_spec_window_example.py in this process, short: a local and a global layer, a chain and a tree, odd and even lengths,
    checked inside the example against torch over the dequantised visible set"""
    import importlib.util
    torch_mod()
    drop_engine()
    spec = importlib.util.spec_from_file_location("k8v4_spec_window_example", os.path.join(ROOT, "examples", "k8v4_spec_window_example.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(rounds=2, verbose=False) == 2


def test_a_walk_through_the_connector_on_a_local_and_a_global_layer(oracle):
    """two requests, write_prefill(59) and (6), then eight rounds of (attend_spec(window=33) on layer 0, attend_spec() on layer 1, commit of
    1..3 accepted positions): the first request's lo(0) walks 27 .. 40 across the tile bound at 32 and its stored count 58 .. 72 across
    the one at 64; odd and even lengths; every step against float64 over a shadow of the committed rows"""
    torch = torch_mod()
    rng = np.random.default_rng(7900)
    rows = lambda *shape: rng.standard_normal(shape).astype(np.float16)
    S, R, W, rids = 3, 4, 33, [7, 9]
    accepts = [[1, 3], [2, 1], [3, 2], [1, 1], [2, 3], [3, 1], [1, 2], [2, 2]]
    shadow = [[rows(L, n, H, D), rows(L, n, H, D)] for n in (59, 6)]
    worst, los, stores, parities = 0.0, [], [], set()
    with _pool(torch) as (lib, conn):
        keep = []
        for rid, (k, v) in zip(rids, shadow):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
        calls = []
        for name in ("attend_kv_spec", "attend_kv_spec_window"):
            real = getattr(lib, name)
            setattr(lib, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
        for step, accept in enumerate(accepts):
            lengths = [s[0].shape[1] for s in shadow]
            assert [conn.length(r) for r in rids] == lengths
            los.append(lo_of(lengths[0], 0, W)); stores.append(lengths[0] & ~1); parities.update(n & 1 for n in lengths)
            q5, k_new, v_new = rows(2, S, H, R, D), rows(2, S, L, H, D), rows(2, S, L, H, D)
            dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
            del calls[:]
            got = [conn.attend_spec(0, rids, dq, dk, dv, SM, window=W), conn.attend_spec(1, rids, dq, dk, dv, SM)]
            torch.cuda.synchronize()
            assert calls == ["attend_kv_spec_window", "attend_kv_spec"]
            base = [n & 1 for n in lengths]
            for layer, window in ((0, W), (1, 0)):
                words, depths = _tables(_chain(S), base, 2, window)
                for b, (sk, sv) in enumerate(shadow):
                    n, even = lengths[b], lengths[b] & ~1
                    region = _region(sk[layer, :even], sv[layer, :even], T)
                    one = Members.__new__(Members)
                    one.n, one.window, one.lengths, one.stored, one.own = 1, window, [n], [even], None
                    one.pair = lambda oracle, layer, i, region=region: (HeadChecker(oracle, FP8, region, T), HeadChecker(oracle, MX4, region, T))
                    one.tails = [(sk[:, -1], sv[:, -1]) if n & 1 else None]
                    kh, vh, _ = one.held(layer, k_new[b:b + 1], v_new[b:b + 1])
                    want = one.want(oracle, layer, _rows_of(q5[b:b + 1]), R, kh, vh, words[b:b + 1], depths[b:b + 1])
                    worst = max(worst, _compare(want, _rows_of(got[layer][b:b + 1].cpu().numpy()), None, f"walk step {step} layer {layer} length {n}"))
            keep += conn.commit(rids, dk, dv, accept)
            for b in range(2):
                shadow[b][0] = np.concatenate([shadow[b][0], k_new[b, :accept[b]].transpose(1, 0, 2, 3)], axis=1)
                shadow[b][1] = np.concatenate([shadow[b][1], v_new[b, :accept[b]].transpose(1, 0, 2, 3)], axis=1)
        torch.cuda.synchronize()
        del keep
    assert min(los) < 32 <= max(los) and min(stores) < 64 <= max(stores) and parities == {0, 1}
    print(f"k8v4 spec window connector walk: worst err / tol {worst:.3f}")
