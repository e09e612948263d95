"""-m gpu: shared-prefix attention over the split pool ("K8V4") -- speckv_ext_attend_prefix_fold_kv (the four (FP8, MXFP4) instances of
k_attend_prefix, whole and split, plain and WINDOW; k_prefix_combine[_window]) and SpeckvSplitKVConnector.attend_shared /
attend_chunk_shared on top of it.

Reference: the numpy float64 softmax of tests/test_gpu_shared_prefix.py::_decode_ref over up to four parts, restated per row so that
every part can carry a lower bound (what a row sees under a window is tests/test_gpu_shared_prefix_window.py::_visible, by brute
force).  Stored K rows are HeadChecker(oracle, FP8).kv(head)[0] and stored V rows HeadChecker(oracle, MXFP4).kv(head)[1], paired as
tests/test_gpu_k8v4_decode.py::_checker pairs them.  The prefix part takes the fp16 query; a member's own stored part takes the query
as E4M3 x a row scale in a decode step (HeadChecker(oracle, FP8).q_rows) and in fp16 on the chunk route; tails and new rows are fp16.
Bounds, the project's, unchanged:
  decode steps                                  |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta from the own part
  the chunk route, entry calls with a given own |err| <= 2e-3 sum p|v| + 1e-6, |lse err| <= 2e-3
Every (member, position, head, row) is compared.  Shapes: L = 2 (the layers' contents differ), H = 8, D = 128, T = 256; the split and
two-group cases at T = 512."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_shared_prefix import L, LAYER, NEG_INF, PATTERN, SM, T, _assert_decode, _dev, _f32, _rows, _softmax
from tests.test_gpu_shared_prefix_window import _visible
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
T2 = 512
FP8, MX4, INT4 = 4, 5, 3
OWN = [0, 1, 2, 37, 64]                              # no pool and no tail, a tail only, one page, pool and tail, whole tiles
PLENS = [2, 36, 64, 98, 254]
P0, P1 = 100, 101

_data, _pairs = {}, {}


def _inputs(rpp):
    """the 254-position prefix, a second one of 64, one of 480 (T = 512), the members' own prompts by length, query rows: the same everywhere"""
    if "prefix" not in _data:
        rng = np.random.default_rng(8431)
        _data["prefix"] = (_rows(rng, L, 254, H, D), _rows(rng, L, 254, H, D))
        _data["second"] = (_rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D))
        _data["long"] = (_rows(rng, L, 480, H, D), _rows(rng, L, 480, H, D))
        _data["own"] = {n: (_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in OWN}
    if ("q", rpp) not in _data:
        _data[("q", rpp)] = _rows(np.random.default_rng(700 + rpp), 18, H, rpp, D)
    return _data["prefix"], _data["second"], _data["long"], _data["own"], _data[("q", rpp)]


def _pair(oracle, kv, layer, t):
    """(HeadChecker over the FP8 records, HeadChecker over the MXFP4 records) of the even part of (k, v) [L][n][H][D] at `layer`, once per content"""
    k, v = kv
    key = (layer, t, k.shape[1], float(np.abs(k[layer].astype(np.float32)).sum()), float(np.abs(v[layer].astype(np.float32)).sum()))
    if key not in _pairs:
        even = k.shape[1] & ~1
        region = _region(k[layer, :even], v[layer, :even], t)
        _pairs[key] = (HeadChecker(oracle, FP8, region, t), HeadChecker(oracle, MX4, region, t))
    return _pairs[key]


def _want(oracle, layer, rows, quant_own):
    """float64 of any rows: row = (q [H][R][D] fp16, prefix (k, v) or None, its layout's T, the prefix positions the row sees, own (k, v)
    [L][n][H][D], its layout's T, the own positions the row sees, the new rows [(k [L][H][D], v [L][H][D])] it sees).  quant_own: the own
    stored part under the E4M3 query (a decode step).  -> want [N][H][R][D], lse [N][H][R], mag, delta [N][H], as _assert_decode takes them"""
    N, R = len(rows), rows[0][0].shape[1]
    want, mag = np.zeros((N, H, R, D)), np.zeros((N, H, R, D))
    wlse, delta = np.full((N, H, R), -np.inf), np.zeros((N, H))
    run = lambda ps: slice(ps[0], ps[-1] + 1)
    for head in range(H):
        for i, (q, prefix, tp, pre, own, to, mine, new) in enumerate(rows):
            qf = q[head].astype(np.float64)
            S_, V_ = [], []
            if pre:
                assert pre == list(range(pre[0], pre[-1] + 1))
                k8, v4 = _pair(oracle, prefix, layer, tp)
                S_.append(qf @ k8.kv(head)[0][run(pre)].T); V_.append(v4.kv(head)[1][run(pre)])
            n = own[0].shape[1]
            stored = [p for p in mine if p < (n & ~1)]
            if stored:
                assert stored == list(range(stored[0], stored[-1] + 1))
                k8, v4 = _pair(oracle, own, layer, to)
                Ko, qx = k8.kv(head)[0][run(stored)], qf
                if quant_own:
                    qx = k8.q_rows(q[head])
                    delta[i, head] = 3e-5 * float((np.abs(qx) @ np.abs(Ko).T).max()) * SM
                S_.append(qx @ Ko.T); V_.append(v4.kv(head)[1][run(stored)])
            if n & 1 and n - 1 in mine:
                S_.append(qf @ own[0][layer, n - 1, head].astype(np.float64)[:, None]); V_.append(own[1][layer, n - 1, head].astype(np.float64)[None])
            for k, v in new:
                S_.append(qf @ k[layer, head].astype(np.float64)[:, None]); V_.append(v[layer, head].astype(np.float64)[None])
            if S_:
                want[i, head], wlse[i, head], mag[i, head] = _softmax(S_, V_)
    return want, wlse, mag, delta


def _decode_rows(q, members, window, t=T):
    """the rows of a decode step: members[m] = (prefix or None, its T, prefix_len, own); the query is the member's last own position
    (none: it sits right behind the prefix)"""
    rows = []
    for m, (prefix, tp, plen, own) in enumerate(members):
        n = own[0].shape[1]
        pre, mine, _ = _visible(plen, n, -1 if n else 0, window if n or not window else window + 1)
        rows.append((q[m], prefix, tp, pre, own, t, mine, []))
    return rows


EMPTY = (np.zeros((L, 0, H, D), np.float16),) * 2


def _prefix_rows(q, prefix, tp, lens, lo=None):
    """entry-level rows over out = 0, lse = -inf: q [N][H][R][D], row i sees [lo[i], lens[i]) of the prefix and nothing else"""
    return [(q[i], prefix[i] if isinstance(prefix, list) else prefix, tp[i] if isinstance(tp, list) else tp,
             list(range(0 if lo is None else lo[i], lens[i])), EMPTY, T, [], []) for i in range(len(lens))]


@contextlib.contextmanager
def _world(torch, prefixes, owns, t=T):
    """a split connector that holds the prefixes {request id: (k, v)} and one member per entry of owns (request ids 0, 1, ...)"""
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvSplitKVConnector(lib, L, H, D, t)
        keep = []
        for rid, (k, v) in list(prefixes.items()) + list(enumerate(owns)):
            conn.add_request(rid)
            if k.shape[1]:
                keep += conn.write_prefill(rid, _dev(torch, k), _dev(torch, v))
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
        del keep
    finally:
        lib.finalize()


def _own_step(torch, conn, layer, rids, q, window=None):
    """the members' own decode step as attend(window=) issues it, with the log-sum-exp: (out [M][H][R][D], lse [M][H][R]) as int32 bits"""
    out, lse, _ = conn._attend_own(layer, rids, _dev(torch, q), SM, None, window)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.int32), lse.cpu().numpy().view(np.int32)


def _nothing(M, C_, R):
    return np.zeros((M, C_, H, R, D), np.int32), np.full((M, C_, H, R), NEG_INF, np.int32)


def _fold(torch, lib, kh, vh, first, layer, q, lens, n_q, out, lse, own_seen=None, depth=None, window=0, n_splits=1):
    """speckv_ext_attend_prefix_fold_kv itself: q [M][C][H][R][D] fp16, out / lse int32 bit patterns of what the members hold going in
    -> (out, lse) bit patterns coming out; depth [M][C] ints or None"""
    M, C_, _, R, _ = q.shape
    dq = _dev(torch, q)
    do, dl = _dev(torch, np.ascontiguousarray(out).reshape(M, C_, H, R, D)), _dev(torch, np.ascontiguousarray(lse).reshape(M, C_, H, R))
    dd = None if depth is None else _dev(torch, np.asarray(depth, np.uint32).reshape(M, C_).view(np.int32))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    lib.attend_prefix_fold_kv(np.asarray(kh, np.uint64), np.asarray(vh, np.uint64), np.asarray(first, np.uint32), layer, dq.data_ptr(), C_, R,
                              np.asarray(lens, np.uint32), np.asarray(n_q, np.uint32), None if own_seen is None else np.asarray(own_seen, np.uint32),
                              0 if dd is None else dd.data_ptr(), window, n_splits, SM, do.data_ptr(), dl.data_ptr(), st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    return do.cpu().numpy().reshape(np.shape(out)), dl.cpu().numpy().reshape(np.shape(lse))


def _handles(conn, *rids):
    return [conn.requests[r].k_handle for r in rids], [conn.requests[r].v_handle for r in rids]


# ----------------------------------------------------------------------------- 1. the entry, C = 1
@pytest.mark.parametrize("rpp", [1, 4, 16])
def test_the_entry_in_a_decode_step_against_float64(oracle, rpp):
    """one 254-position prefix; five members see 2, 36, 64, 98 and 254 positions of it and hold 0, 1, 2, 37 and 64 of their own.  Each
    arrives once with nothing (out 0, lse -inf: the prefix part alone, delta = 0) and once with the (out, lse) of a real attend; at
    layer 1, and (rows_per_pos 4) at layer 0 -- the layers' contents differ, so region `layer` of BOTH allocations is proven"""
    torch = torch_mod()
    prefix, _, _, owns, q = _inputs(rpp)
    q, rids = q[:5], list(range(5))
    mine = [owns[n] for n in OWN]
    with _world(torch, {P0: prefix}, mine) as (lib, conn):
        kh, vh = _handles(conn, P0)
        for layer in [LAYER, 0] if rpp == 4 else [LAYER]:
            out, lse = _nothing(5, 1, rpp)
            got, glse = _fold(torch, lib, kh, vh, [0, 5], layer, q[:, None], PLENS, [1] * 5, out, lse)
            ref = _want(oracle, layer, _prefix_rows(q, prefix, T, PLENS), False)
            assert not ref[3].any()
            _assert_decode(got[:, 0], glse[:, 0], ref, f"attend_prefix_fold_kv rows_per_pos {rpp} layer {layer}, nothing of their own")
            out, lse = _own_step(torch, conn, layer, rids, q)
            got, glse = _fold(torch, lib, kh, vh, [0, 5], layer, q[:, None], PLENS, [1] * 5, out[:, None], lse[:, None])
            ref = _want(oracle, layer, _decode_rows(q, [(prefix, T, PLENS[m], mine[m]) for m in rids], None), True)
            _assert_decode(got[:, 0], glse[:, 0], ref, f"attend_prefix_fold_kv rows_per_pos {rpp} layer {layer}, behind attend")


# ----------------------------------------------------------------------------- 2. dead pairs
def test_dead_pairs_keep_their_bits_and_a_group_without_a_live_pair_launches_nothing(oracle):
    """C = 3, rows_per_pos 4, six members with n_q 0, 1, 3, 3, 0, 2: out / lse prefilled with a bit pattern, every dead row identical
    bit for bit afterwards; the live pairs are the prefix-only attention.  A second group whose members are all dead, and a call
    without any live pair, write nothing"""
    torch = torch_mod()
    prefix, second, _, _, q = _inputs(4)
    C_, n_q, lens = 3, [0, 1, 3, 3, 0, 2], [36, 98, 254, 64, 2, 36]
    M = len(n_q)
    qc = np.ascontiguousarray(q[:M * C_].reshape(M, C_, H, 4, D))
    live = np.asarray([[j < n_q[m] for j in range(C_)] for m in range(M)])
    out, lse = np.full((M, C_, H, 4, D), PATTERN, np.int32), np.full((M, C_, H, 4), PATTERN, np.int32)
    out[live], lse[live] = 0, NEG_INF
    with _world(torch, {P0: prefix, P1: second}, []) as (lib, conn):
        kh, vh = _handles(conn, P0)
        flat = [(m, j) for m in range(M) for j in range(C_) if live[m, j]]
        ref = _want(oracle, LAYER, _prefix_rows(np.stack([qc[m, j] for m, j in flat]), prefix, T, [lens[m] for m, _ in flat]), False)
        for n_splits in (1, 3):
            got, glse = _fold(torch, lib, kh, vh, [0, M], LAYER, qc, lens, n_q, out, lse, n_splits=n_splits)
            assert np.all(got[~live] == PATTERN) and np.all(glse[~live] == PATTERN), (n_splits, "a dead pair was written")
            _assert_decode(np.stack([got[m, j] for m, j in flat]), np.stack([glse[m, j] for m, j in flat]), ref,
                           f"attend_prefix_fold_kv C = 3 with dead pairs, n_splits {n_splits}")
        # two groups, the second (members 4 and 5 over the other prefix) without a live pair: its rows keep the pattern
        kh2, vh2 = _handles(conn, P0, P1)
        dead2 = [0, 1, 3, 3, 0, 0]
        live2 = np.asarray([[j < dead2[m] for j in range(C_)] for m in range(M)])
        out2, lse2 = np.full_like(out, PATTERN), np.full_like(lse, PATTERN)
        out2[live2], lse2[live2] = 0, NEG_INF
        got, glse = _fold(torch, lib, kh2, vh2, [0, 4, M], LAYER, qc, [36, 98, 254, 64, 2, 36], dead2, out2, lse2)
        assert np.all(got[~live2] == PATTERN) and np.all(glse[~live2] == PATTERN) and not np.any(glse[live2] == NEG_INF)
        # nothing live at all: SPECKV_OK, nothing written
        for lens_, n_q_ in (([0] * M, n_q), (lens, [0] * M)):
            got, glse = _fold(torch, lib, kh, vh, [0, M], LAYER, qc, lens_, n_q_, out, lse)
            assert np.array_equal(got, out) and np.array_equal(glse, lse)


# ----------------------------------------------------------------------------- 3. two groups, two layouts
def test_two_groups_whose_prefixes_lie_in_layouts_of_256_and_512(oracle):
    """one prefix in a layout of T = 256, one in a layout of T = 512, first_member [0, 3, 5]: the region stride is each group's own, in
    both allocations; both layers"""
    torch = torch_mod()
    prefix, _, long_, _, q = _inputs(4)
    q = q[:5]
    lens = [98, 254, 2, 480, 34]
    with _world(torch, {P0: prefix}, []) as (lib, conn):
        big = SpeckvSplitKVConnector(lib, L, H, D, T2)
        big.add_request(P1)
        keep = big.write_prefill(P1, _dev(torch, long_[0]), _dev(torch, long_[1]))
        torch.cuda.synchronize()
        kh = [conn.requests[P0].k_handle, big.requests[P1].k_handle]
        vh = [conn.requests[P0].v_handle, big.requests[P1].v_handle]
        for layer in range(L):
            out, lse = _nothing(5, 1, 4)
            got, glse = _fold(torch, lib, kh, vh, [0, 3, 5], layer, q[:, None], lens, [1] * 5, out, lse)
            ref = _want(oracle, layer, _prefix_rows(q, [prefix] * 3 + [long_] * 2, [T] * 3 + [T2] * 2, lens), False)
            _assert_decode(got[:, 0], glse[:, 0], ref, f"attend_prefix_fold_kv two groups, layouts of 256 and 512, layer {layer}")
        del keep


# ----------------------------------------------------------------------------- 4. split
def test_pieces_over_a_prefix_of_fifteen_tiles_against_float64(oracle):
    """T = 512, a 480-position prefix (15 tiles), n_splits 0, 2, 3 and 15; one member sees 34 positions, so pieces beyond its length
    weigh nothing; the members come from their own attend.  Forced pieces did run the piece launch and the merge: other bits"""
    torch = torch_mod()
    _, _, long_, owns, q = _inputs(4)
    lens, mine = [480, 34, 480, 2], [owns[37], owns[64], owns[0], owns[1]]
    n = len(lens)
    q, rids = q[:n], list(range(n))
    with _world(torch, {P0: long_}, mine, t=T2) as (lib, conn):
        kh, vh = _handles(conn, P0)
        out, lse = _own_step(torch, conn, LAYER, rids, q)
        ref = _want(oracle, LAYER, _decode_rows(q, [(long_, T2, lens[m], mine[m]) for m in rids], None, t=T2), True)
        seen = {}
        for n_splits in (1, 0, 2, 3, 15):
            got, glse = _fold(torch, lib, kh, vh, [0, n], LAYER, q[:, None], lens, [1] * n, out[:, None], lse[:, None], n_splits=n_splits)
            _assert_decode(got[:, 0], glse[:, 0], ref, f"attend_prefix_fold_kv n_splits {n_splits}")
            seen[n_splits] = got
        assert np.array_equal(seen[0], seen[1])                           # the rule cuts nothing this short: 15 tiles < 2 x 32
        for n_splits in (2, 3, 15):
            assert not np.array_equal(seen[n_splits], seen[1]), n_splits


# ----------------------------------------------------------------------------- 5. window
W = 70
WIN_LENS, WIN_SEEN = [254, 254, 254, 98, 36], [5, 8, 70, 30, 64]          # lo = 189 (inside tile 5), 192 (a tile boundary), dead, 58, 30


def _win_live_lo(lens, seen, depth, window):
    """(live [M][C], lo [M][C]) by the rule stated at the entry: lo = max(0, prefix_len + own_seen + d - W), dead where lo >= prefix_len"""
    lo = np.asarray([[max(0, lens[m] + seen[m] + d - window) for d in depth[m]] for m in range(len(lens))])
    return lo < np.asarray(lens)[:, None], lo


def test_the_window_form_against_float64_and_what_it_leaves_untouched(oracle):
    """W = 70 at the entry over a given own part (out 0, lse -inf: 2e-3): lo inside a tile (prefix_len 254, own_seen 5: 189), lo on a
    tile boundary (own_seen 8: 192), a member with own_seen >= W that keeps a fill pattern bit for bit, shorter lengths beside them;
    a window that cuts nothing gives the window = 0 call's bits; a depth table with C = 3 and depths [0, 1, 1] (a chain would be
    0, 1, 2: the third position shows the table is read); and the window together with n_splits = 2"""
    torch = torch_mod()
    prefix, _, _, _, q = _inputs(4)
    M = len(WIN_LENS)
    with _world(torch, {P0: prefix}, []) as (lib, conn):
        kh, vh = _handles(conn, P0)
        q1 = q[:M]
        live, lo = _win_live_lo(WIN_LENS, WIN_SEEN, [[0]] * M, W)
        assert [int(x) for x in lo[:, 0]] == [189, 192, 254, 58, 30] and [bool(x) for x in live[:, 0]] == [True, True, False, True, True]
        rows = [r for r, ok in zip(_prefix_rows(q1, prefix, T, WIN_LENS, lo[:, 0]), live[:, 0]) if ok]
        ref = _want(oracle, LAYER, rows, False)
        out, lse = np.full((M, 1, H, 4, D), PATTERN, np.int32), np.full((M, 1, H, 4), PATTERN, np.int32)
        out[live], lse[live] = 0, NEG_INF
        for n_splits in (1, 2):
            got, glse = _fold(torch, lib, kh, vh, [0, M], LAYER, q1[:, None], WIN_LENS, [1] * M, out, lse, WIN_SEEN, None, W, n_splits)
            assert np.all(got[2] == PATTERN) and np.all(glse[2] == PATTERN), "a member whose window lies in its own part was touched"
            _assert_decode(got[live[:, 0], 0], glse[live[:, 0], 0], ref, f"attend_prefix_fold_kv W {W} n_splits {n_splits}")
        # a window that cuts nothing: the unwindowed launches and their bits, with and without own_seen
        out0, lse0 = _nothing(M, 1, 4)
        plain = _fold(torch, lib, kh, vh, [0, M], LAYER, q1[:, None], WIN_LENS, [1] * M, out0, lse0)
        wide = _fold(torch, lib, kh, vh, [0, M], LAYER, q1[:, None], WIN_LENS, [1] * M, out0, lse0, WIN_SEEN, None, 400)
        zero = _fold(torch, lib, kh, vh, [0, M], LAYER, q1[:, None], WIN_LENS, [1] * M, out0, lse0, WIN_SEEN, None, 0)
        for other in (wide, zero):
            assert np.array_equal(other[0], plain[0]) and np.array_equal(other[1], plain[1])
        # a depth table: C = 3, depths [0, 1, 1]
        C_, depth = 3, [[0, 1, 1]] * M
        qc = np.ascontiguousarray(q[:M * C_].reshape(M, C_, H, 4, D))
        live, lo = _win_live_lo(WIN_LENS, WIN_SEEN, depth, W)
        flat = [(m, j) for m in range(M) for j in range(C_) if live[m, j]]
        rows = _prefix_rows(np.stack([qc[m, j] for m, j in flat]), prefix, T, [WIN_LENS[m] for m, _ in flat], [int(lo[m, j]) for m, j in flat])
        ref = _want(oracle, LAYER, rows, False)
        out, lse = np.full((M, C_, H, 4, D), PATTERN, np.int32), np.full((M, C_, H, 4), PATTERN, np.int32)
        out[live], lse[live] = 0, NEG_INF
        got, glse = _fold(torch, lib, kh, vh, [0, M], LAYER, qc, WIN_LENS, [3] * M, out, lse, WIN_SEEN, depth, W)
        assert np.all(got[~live] == PATTERN) and np.all(glse[~live] == PATTERN)
        _assert_decode(np.stack([got[m, j] for m, j in flat]), np.stack([glse[m, j] for m, j in flat]), ref, f"attend_prefix_fold_kv W {W}, depths 0 1 1")
        chain = _fold(torch, lib, kh, vh, [0, M], LAYER, qc, WIN_LENS, [3] * M, out, lse, WIN_SEEN, None, W)
        assert np.array_equal(chain[0][:, :2], got[:, :2]) and not np.array_equal(chain[0][0, 2], got[0, 2])


# ----------------------------------------------------------------------------- 6. refusals
def test_the_entry_refuses_and_launches_nothing():
    torch = torch_mod()
    prefix, second, long_, _, q = _inputs(4)
    n = 4
    q, lens = q[:n, None], [98, 36, 2, 64]
    out, lse = np.full((n, 1, H, 4, D), PATTERN, np.int32), np.full((n, 1, H, 4), PATTERN, np.int32)
    with _world(torch, {P0: prefix, P1: second}, []) as (lib, conn):
        (k0, k1), (v0, v1) = _handles(conn, P0, P1)
        lib.set_compression_scheme(INT4)
        int4 = lib.alloc(T * L * H * D * 2); lib.set_layout(int4, T, L // 2, H, D, 2)
        big = SpeckvSplitKVConnector(lib, L, H, D, T2)                    # the same content in a layout of other num_tokens
        big.add_request(7)
        kbig = big.requests[7].k_handle
        dq, do, dl = _dev(torch, q), _dev(torch, out), _dev(torch, lse)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()

        def args(kh=(k0, k1), vh=(v0, v1), first=(0, 2, 4), lens=lens, own_seen=None, **change):
            a = dict(k_handles=None if kh is None else np.asarray(kh, np.uint64), v_handles=None if vh is None else np.asarray(vh, np.uint64),
                     first_member=np.asarray(first, np.uint32), layer=LAYER, d_q=dq.data_ptr(), C=1, rows_per_pos=4,
                     prefix_len=np.asarray(lens, np.uint32), n_q=np.ones(n, np.uint32), own_seen=own_seen, d_depth=0, window=0, n_splits=1,
                     sm_scale=SM, d_out=do.data_ptr(), d_lse=dl.data_ptr(), stream=st.cuda_stream)
            a.update(change)
            return a

        def refused(status, what, **change):
            with pytest.raises(SpeckvError) as e:
                lib.attend_prefix_fold_kv(**args(**change))
                pytest.fail(what)
            assert e.value.status == status, (what, e.value.status)
            st.synchronize(); torch.cuda.synchronize()
            assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all()), (what, "a refused call wrote out / lse")

        invalid = {
            "K and V handles swapped": dict(kh=(v0, v1), vh=(k0, k1)), "an INT4 allocation as K": dict(kh=(k0, int4)),
            "an FP8 allocation as V": dict(vh=(v0, k1)), "NULL v_handles": dict(vh=None), "NULL k_handles": dict(kh=None),
            "an odd prefix_len": dict(lens=[98, 35, 2, 64]), "a prefix_len beyond T": dict(lens=[98, 36, 2, T + 2]),
            "a layer beyond the regions": dict(layer=L), "a layer far beyond": dict(layer=1000),
            "num_tokens that differ inside a group": dict(kh=(k0, kbig)), "NULL own_seen with a window": dict(window=50),
            "n_splits 65": dict(n_splits=65), "rows_per_pos 3": dict(rows_per_pos=3), "NULL lse": dict(d_lse=0),
        }
        for what, change in invalid.items():
            refused(-4, what, **change)                                      # SPECKV_ERR_INVAL
        refused(-1, "an unknown K handle", kh=(k0, 0xDEAD))                  # SPECKV_ERR_GENERAL
        refused(-1, "an unknown V handle", vh=(v0, 0xDEAD))
        refused(-4, "a late refusal with forced pieces", vh=(v0, k1), n_splits=3)
        # capture: refused, nothing launched
        s = torch.cuda.Stream()
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            with pytest.raises(SpeckvError) as e:
                lib.attend_prefix_fold_kv(**args(stream=s.cuda_stream))
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all())
        # and the same buffers ARE written by the call that is not refused
        ok_out, ok_lse = torch.zeros_like(do), torch.full_like(dl, int(NEG_INF))
        lib.attend_prefix_fold_kv(**args(d_out=ok_out.data_ptr(), d_lse=ok_lse.data_ptr()))
        st.synchronize()
        assert not bool((ok_lse == int(NEG_INF)).any())
        lib.free(int4)


# ----------------------------------------------------------------------------- 7. attend_shared
SH_OWN = [0, 1, 2, 37, 64, 64]
SH_PIDS = [P0, P0, None, P0, P1, P0]                                        # not adjacent: the permutation runs
SH_LENS = [98, 254, None, 36, 64, 2]


@pytest.mark.parametrize("g", [1, 4])
def test_attend_shared_against_float64(oracle, g):
    """six members with own lengths 0, 1, 2, 37, 64, 64 and prefix_ids [P0, P0, None, P0, P1, P0], mixed prefix_lens; a global layer
    and W = 100; both layers.  The member without a prefix keeps attend()'s bits; all None returns the bits of attend"""
    torch = torch_mod()
    prefix, second, _, owns, q = _inputs(g)
    mine = [owns[n] for n in SH_OWN]
    M = len(mine)
    q, rids = q[:M], list(range(M))
    which = {P0: prefix, P1: second, None: None}
    members = [(which[SH_PIDS[m]], T, SH_LENS[m] or 0, mine[m]) for m in rids]
    with _world(torch, {P0: prefix, P1: second}, mine) as (lib, conn):
        assert SpeckvSplitKVConnector.shared_groups(rids, SH_PIDS)[0] != rids
        for window in (None, 100):
            for layer in range(L):
                got = conn.attend_shared(layer, rids, SH_PIDS, _dev(torch, q), SM, prefix_lens=SH_LENS, window=window)
                torch.cuda.synchronize()
                got = got.cpu().numpy().view(np.int32)
                ref = _want(oracle, layer, _decode_rows(q, members, window), True)
                _assert_decode(got, None, ref, f"attend_shared g {g} W {window} layer {layer}")
                plain = conn.attend(layer, rids, _dev(torch, q), SM, window=window)
                torch.cuda.synchronize()
                plain = plain.cpu().numpy().view(np.int32)
                assert np.array_equal(got[2], plain[2]), "the member without a prefix lost attend()'s bits"
                assert not np.array_equal(got[0], plain[0])
                none = conn.attend_shared(layer, rids, [None] * M, _dev(torch, q), SM, window=window)
                torch.cuda.synchronize()
                assert np.array_equal(none.cpu().numpy().view(np.int32), plain), "all None is not attend"


# ----------------------------------------------------------------------------- 8. attend_chunk_shared
def _step_rows(q, new, members, parents, n_new, window):
    """the live rows of a step: node j of member m sees the prefix and its own positions by its depth's bound and the new rows on its
    root path that the window leaves.  -> (rows, [(m, j)])"""
    rows, at, depths = [], [], {}
    for a in range(len(parents)):                                         # (a parent stands in front of its children)
        depths[a] = 0 if parents[a] < 0 else depths[parents[a]] + 1
    for m, (prefix, plen, own) in enumerate(members):
        for j in range(n_new[m]):
            path, a = [], j
            while a >= 0:
                path.append(a)
                a = parents[a]
            path = path[::-1]
            pre, mine, keep = _visible(plen, own[0].shape[1], depths[j], window, [depths[a] for a in path])
            rows.append((q[m, j], prefix, T, pre, own, T, mine, [(new[0][m, path[k]], new[1][m, path[k]]) for k in keep]))
            at.append((m, j))
    return rows, at


@pytest.mark.parametrize("form", ["causal", "window", "tree", "tree-window"])
def test_attend_chunk_shared_against_float64(oracle, form):
    """S = 3, rows_per_pos 4, ragged n_new over the members of the attend_shared case: causal, under W = 100, with parents [-1, 0, 0],
    and that tree under the window (by depth: the fold reads the depth table the own call reads).  Rows that are not live are zero"""
    torch = torch_mod()
    prefix, second, _, owns, _ = _inputs(4)
    mine = [owns[n] for n in SH_OWN]
    M, S_ = len(mine), 3
    rids = list(range(M))
    rng = np.random.default_rng(5150)
    q, new = _rows(rng, M, S_, H, 4, D), (_rows(rng, M, S_, L, H, D), _rows(rng, M, S_, L, H, D))
    n_new = [3, 1, 2, 0, 3, 3]
    parents = [-1, 0, 0] if "tree" in form else [-1, 0, 1]
    window = 100 if "window" in form else None
    which = {P0: prefix, P1: second, None: None}
    members = [(which[SH_PIDS[m]], SH_LENS[m] or 0, mine[m]) for m in rids]
    with _world(torch, {P0: prefix, P1: second}, mine) as (lib, conn):
        for layer in range(L):
            got = conn.attend_chunk_shared(layer, rids, SH_PIDS, _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1]), SM, n_new=n_new,
                                           prefix_lens=SH_LENS, window=window, parents=parents if "tree" in form else None)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            rows, at = _step_rows(q, new, members, parents, n_new, window)
            ref = _want(oracle, layer, rows, False)
            assert not ref[3].any()
            _assert_decode(np.stack([got[m, j] for m, j in at]).view(np.int32), None, ref, f"attend_chunk_shared {form} layer {layer}")
            for m, n in enumerate(n_new):
                assert not got[m, n:].any(), (form, m, "a row that is not live is not zero")
        none = conn.attend_chunk_shared(LAYER, rids, [None] * M, _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1]), SM, n_new=n_new,
                                        window=window, parents=parents if "tree" in form else None)
        plain = conn.attend_chunk(LAYER, rids, _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1]), SM, n_new=n_new, window=window,
                                  parents=parents if "tree" in form else None)
        torch.cuda.synchronize()
        assert np.array_equal(none.cpu().numpy().view(np.int32), plain.cpu().numpy().view(np.int32)), "all None is not attend_chunk"


# ----------------------------------------------------------------------------- the example
def test_the_example_runs():
    """examples/k8v4_shared_prefix_example.py in this process, short: a system prompt held once, members with suffixes, decode steps
    checked inside the example against members that hold a full copy"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "k8v4_shared_prefix_example.py")
    spec = importlib.util.spec_from_file_location("k8v4_shared_prefix_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(prompt=98, members=3, steps=2, verbose=False) == 3 * 2
