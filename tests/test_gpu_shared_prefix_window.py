"""-m gpu: shared-prefix attention on sliding-window layers and under draft trees -- speckv_ext_attend_prefix_fold_window
(k_attend_prefix's WINDOW form whole and split, k_prefix_combine_window) and SpeckvKVConnector.attend_shared(window=) /
attend_chunk_shared(window=, parents=) / attend_tree_shared on top of it.

Reference: the numpy float64 three-part softmax of tests/test_gpu_shared_prefix.py with a lower bound on every part.  A row sees the
last W positions of prefix + own (+ its root path among the new rows): what that is, is restated here by brute force per row
(_visible).  The prefix scores come from the fp16 query over the oracle's decoded prefix rows [lo, prefix_len) (HeadChecker.kv); a
member's own stored scores from the query as the format's decode kernel takes it (HeadChecker.q_rows) in a decode step, from the
fp16 query on the chunk and tree routes, over the own rows from the window's bound on (what HeadChecker.want_rows(pos_begin=)
takes); the tail and the new rows from the fp16 query.  Bounds, the project's, unchanged:
  decode steps           |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta from the own part
  chunk and tree routes  |err| <= 2e-3 sum p|v| + 1e-6, |lse err| <= 2e-3

Shapes: L = 2, T = 256, 8 x 128 heads; prefix lengths 2, 36, 64, 98 and 254 of one 254-position prefix, members that hold 0, 1, 2, 37
and 64 positions of their own; the split cases at T = 512 over a 481-position prefix."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_shared_prefix import (ALL, L, LAYER, NEG_INF, OWN, P0, P1, PATTERN, PLENS, SM, T, T2, _assert_decode, _checker, _dev, _f32,
                                          _fold, _hostile, _inputs, _rows, _softmax, _split_inputs, _world)

pytestmark = pytest.mark.gpu
WINDOWS = [1, 2, 31, 32, 33, 40, 64, 100, 300]
_worst = {}


def _note(family, scheme, value):
    """the worst err / tol per test family and format, printed as it grows (for DESIGN 8.4 (10))"""
    key = (family, scheme)
    if value > _worst.get(key, -1.0):
        _worst[key] = value
        print(f"WORST {family} {scheme}: {value:.3f}")


# ----------------------------------------------------------------------------- what a row sees, by brute force
def _visible(plen, n_own, depth, window, path=()):
    """A row whose query sits `depth` positions behind the member's n_own own ones (a decode step after append: depth = -1, the query
    IS the last own position), with `path` = the depths of the new rows on its root path, itself included: the absolute positions are
    the prefix [0, plen), the own [plen, plen + n_own), a new row of depth a at plen + n_own + a.  The row sits at P and sees (P - W, P].
    -> (prefix positions, own positions (indices into the member's own), indices into `path`)"""
    P = plen + n_own + depth
    lo = 0 if not window else P + 1 - window
    return ([t for t in range(plen) if t >= lo], [i for i in range(n_own) if plen + i >= lo],
            [k for k, a in enumerate(path) if plen + n_own + a >= lo])


def _want(oracle, scheme, layer, rows, t=T, quant_own=False):
    """float64 of any rows: row = (q [H][R][D] fp16, prefix (k, v) [L][n][H][D] or None, prefix positions, own (k, v) [L][n][H][D], own
    positions, new rows [(k [L][H][D], v [L][H][D])] the row sees).  Stored own positions (below the even part of the member's
    length) come from the oracle's records -- with quant_own under the query as the format's decode kernel takes it -- the odd last
    one and the new rows are fp16.  -> want [N][H][R][D], lse [N][H][R], mag, delta [N][H], as _assert_decode takes them"""
    N, R = len(rows), rows[0][0].shape[1]
    want, mag = np.zeros((N, H, R, D)), np.zeros((N, H, R, D))
    wlse, delta = np.full((N, H, R), -np.inf), np.zeros((N, H))

    memo = {}

    def checker(kv):                                                     # (_checker keys by content: once per array and call here)
        if id(kv[0]) not in memo:
            memo[id(kv[0])] = _checker(oracle, scheme, kv, layer, t)
        return memo[id(kv[0])]

    def run(positions):                                                  # what a window leaves of a part is one run of positions
        assert positions == list(range(positions[0], positions[-1] + 1))
        return slice(positions[0], positions[-1] + 1)
    for head in range(H):
        qo = None
        for i, (q, prefix, pre, own, mine, new) in enumerate(rows):
            qf = q[head].astype(np.float64)
            S_, V_ = [], []
            if pre:
                Kp, Vp = checker(prefix).kv(head)
                pre = run(pre)
                S_.append(qf @ Kp[pre].T); V_.append(Vp[pre])
            n = own[0].shape[1]
            stored = [p for p in mine if p < (n & ~1)]
            if stored:
                stored = run(stored)
                c = checker(own)
                Ko, Vo = c.kv(head)
                qx = qf
                if quant_own:
                    if qo is None:
                        qo = HeadChecker.q_rows(c, np.stack([r[0][head] for r in rows])).reshape(N, R, D)
                    qx = qo[i]
                    if scheme != "int4":
                        delta[i, head] = 3e-5 * float((np.abs(qx) @ np.abs(Ko[stored]).T).max()) * SM
                S_.append(qx @ Ko[stored].T); V_.append(Vo[stored])
            if n & 1 and n - 1 in mine:
                S_.append(qf @ own[0][layer, n - 1, head].astype(np.float64)[:, None]); V_.append(own[1][layer, n - 1, head].astype(np.float64)[None])
            for k, v in new:
                S_.append(qf @ k[layer, head].astype(np.float64)[:, None]); V_.append(v[layer, head].astype(np.float64)[None])
            if S_:
                want[i, head], wlse[i, head], mag[i, head] = _softmax(S_, V_)
    return want, wlse, mag, delta


def _decode_rows(q, members, window):
    """the rows of a decode step: members[m] = (prefix, plen, own); the query is the member's last own position (none: it sits right
    behind the prefix and sees the last W positions of it)"""
    rows = []
    for m, (prefix, plen, own) in enumerate(members):
        n = own[0].shape[1]
        pre, mine, _ = _visible(plen, n, -1 if n else 0, window if n or not window else window + 1)
        rows.append((q[m], prefix, pre, own, mine, []))
    return rows


def _own_step(torch, conn, layer, rids, q, window):
    """the members' own decode step as attend(window=W) issues it, with the log-sum-exp: (out, lse) as int32 bit patterns"""
    out, lse, _ = conn._attend_layers_lse(layer, 1, rids, _dev(torch, q)[None], SM, None, window)
    torch.cuda.synchronize()
    return out[0].cpu().numpy().view(np.int32), lse[0].cpu().numpy().view(np.int32)


def _fold_w(torch, lib, handles, first, layer, q, lens, n_q, own_seen, depth, window, out, lse, n_splits=1):
    """speckv_ext_attend_prefix_fold_window itself, as _fold calls the unwindowed entry: depth [M][C] ints or None"""
    M, C_, _, R, _ = q.shape
    dq = _dev(torch, q)
    do, dl = _dev(torch, np.ascontiguousarray(out).reshape(M, C_, H, R, D)), _dev(torch, np.ascontiguousarray(lse).reshape(M, C_, H, R))
    dd = None if depth is None else _dev(torch, np.asarray(depth, np.uint32).reshape(M, C_).view(np.int32))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    lib.attend_prefix_fold_window(np.asarray(handles, np.uint64), np.asarray(first, np.uint32), layer, dq.data_ptr(), C_, R, np.asarray(lens, np.uint32),
                                  np.asarray(n_q, np.uint32), np.asarray(own_seen, np.uint32), 0 if dd is None else dd.data_ptr(), window, n_splits,
                                  SM, do.data_ptr(), dl.data_ptr(), st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    return do.cpu().numpy().reshape(np.shape(out)), dl.cpu().numpy().reshape(np.shape(lse))


def _shared(torch, conn, layer, rids, pids, q, lens=None, **kw):
    got = conn.attend_shared(layer, rids, pids, _dev(torch, q), SM, prefix_lens=lens, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.int32)


def _bits(torch, x):
    torch.cuda.synchronize()
    return x.cpu().numpy().view(np.int32)


# ----------------------------------------------------------------------------- 1. decode steps
@pytest.mark.parametrize("rpp,n", [(1, 65), (4, 17), (16, 5), (4, 1)])
@pytest.mark.parametrize("scheme", ALL)
def test_decode_steps_under_a_window_against_float64(oracle, scheme, rpp, n):
    """groups of 65 (rows_per_pos 1), 17 (4), 5 (16) members and of one; prefix lengths 2, 36, 64, 98, 254 and own lengths 0, 1, 2, 37,
    64 mixed inside a block; every W.  The own step is attend(window=W)'s, the entry folds the prefix part into it: against float64;
    members whose window lies wholly in their own part (length >= W) sit beside members that see the prefix and keep the bits of
    attend(window=W); SpeckvKVConnector.attend_shared(window=W) gives the entry's bits"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(rpp)
    q, rids = q[:n], list(range(n))
    lens = [PLENS[(m + m // 5) % 5] for m in rids]
    own_n = [OWN[m % 5] for m in rids]
    mine = [owns[k] for k in own_n]
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        h = conn.requests[P0].handle
        for window in WINDOWS:
            for layer in range(L) if window == 40 else [LAYER]:
                out, lse = _own_step(torch, conn, layer, rids, q, window)
                got, glse = _fold_w(torch, lib, [h], [0, n], layer, q[:, None], lens, [1] * n, own_n, None, window, out, lse)
                ref = _want(oracle, scheme, layer, _decode_rows(q, [(prefix, lens[m], mine[m]) for m in rids], window), quant_own=True)
                _note("decode", scheme, _assert_decode(got, glse, ref, f"attend_prefix_fold_window {scheme} rows_per_pos {rpp} members {n} W {window} layer {layer}"))
                for m in rids:
                    if own_n[m] >= window:                               # dead for the fold: not touched
                        assert np.array_equal(got[m], out[m]) and np.array_equal(glse[m], lse[m]), (scheme, window, m)
                    else:
                        assert not np.array_equal(glse[m], lse[m]), (scheme, window, m, "a row that sees the prefix was not folded")
                via = _shared(torch, conn, layer, rids, [P0] * n, q, lens, window=window, splits=1)
                assert np.array_equal(via, got), (scheme, rpp, n, window, layer, "the connector does not give the entry's bits")
                plain = _bits(torch, conn.attend(layer, rids, _dev(torch, q), SM, window=window))
                assert np.array_equal(plain, out)


# ----------------------------------------------------------------------------- 2. hostile rows below the bound
@pytest.mark.parametrize("scheme", ALL)
def test_rows_below_a_members_bound_stay_out_position_by_position(oracle, scheme):
    """W = 40 over ONE 98-position prefix, one block: members (prefix_len, own) = (98, 0), (98, 37), (64, 2), (36, 1), (98, 64), (2, 0)
    have lo = 58, 95, 26, 0, dead, 0.  The prefix rows below X are made hostile (K x 200, V = +-1000) for X = 26, 58, 95: the members
    with lo >= X see no hostile row and are judged (the others too where the reference holds the kernel's operands exactly: INT4 and
    MXFP4; over FP8 they are only required finite, as tests/test_gpu_shared_prefix.py explains).  Then over the calm prefix stored
    position t is replaced (negated) for t = lo - 1 and lo of every member: exactly the rows with lo <= t < prefix_len change"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    calm = (prefix[0][:, :98], prefix[1][:, :98])
    W = 40
    lens, own_n = [98, 98, 64, 36, 98, 2], [0, 37, 2, 1, 64, 0]
    lo = [max(0, p + o - W) for p, o in zip(lens, own_n)]
    assert lo == [58, 95, 26, 0, 122, 0]
    mine = [owns[k] for k in own_n]
    rids = list(range(len(lens)))
    q = q[:len(lens)]
    hostile = {X: _hostile(calm, slice(0, X)) for X in (26, 58, 95)}
    places = (25, 26, 57, 58, 94, 95)
    variants = {}
    for i, t_ in enumerate(places):
        k2, v2 = calm[0].copy(), calm[1].copy()
        k2[:, t_], v2[:, t_] = -k2[:, t_], -v2[:, t_]
        variants[110 + i] = (k2, v2)
    with _world(torch, scheme, {P1: calm, **{200 + X: kv for X, kv in hostile.items()}, **variants}, mine) as (lib, conn):
        for layer in range(L):
            for X, pre in hostile.items():
                got = _shared(torch, conn, layer, rids, [200 + X] * len(rids), q, lens, window=W)
                ref = _want(oracle, scheme, layer, _decode_rows(q, [(pre, lens[m], mine[m]) for m in rids], W), quant_own=True)
                judged = [m for m in rids if lo[m] >= X or scheme != "fp8"]
                _note("hostile", scheme, _assert_decode(got, None, ref, f"attend_shared {scheme} W {W}, prefix rows below {X} hostile, layer {layer}", judged))
        got = _shared(torch, conn, LAYER, rids, [P1] * len(rids), q, lens, window=W)
        for i, t_ in enumerate(places):
            other = _shared(torch, conn, LAYER, rids, [110 + i] * len(rids), q, lens, window=W)
            for m, n in enumerate(lens):
                changed = (other[m] != got[m]).any(axis=-1)
                if lo[m] <= t_ < n:
                    assert changed.all(), (scheme, t_, m, "a row that sees the replaced position kept its bits")
                else:
                    assert not changed.any(), (scheme, t_, m, "a row that does not see the replaced position changed")


# ----------------------------------------------------------------------------- 3. forced pieces
@pytest.mark.parametrize("scheme", ALL)
def test_pieces_under_a_window_over_a_long_prefix_against_float64(oracle, scheme):
    """T = 512, a 481-position prefix (15 tiles), W = 33 / 100 / 300, forced 2 / 3 / 5 / 16 pieces and the rule.  Three groups: all six
    members (first_tile 0: the members that see 480 positions have pieces wholly below their bound, those that see 34 and 2 pieces
    wholly beyond their prefix_len); the members of 480 alone (first_tile inside the prefix: the pieces cut the tiles that are
    left); one member alone whose bound lies in the last tile.  Every plan against float64, so split and unsplit agree within it"""
    torch = torch_mod()
    _, _, owns, q = _inputs(4)
    prefix = _split_inputs()
    lens, own_n = [34, 480, 480, 34, 2, 480], [0, 37, 1, 64, 2, 0]
    mine = [owns[k] for k in own_n]
    n = len(lens)
    q = q[:n]
    with _world(torch, scheme, {P0: prefix}, mine, t=T2) as (lib, conn):
        h = conn.requests[P0].handle
        first_tiles = set()
        for window in (33, 100, 300):
            out, lse = _own_step(torch, conn, LAYER, list(range(n)), q, window)
            ref = _want(oracle, scheme, LAYER, _decode_rows(q, [(prefix, lens[m], mine[m]) for m in range(n)], window), t=T2, quant_own=True)
            for members in ([0, 1, 2, 3, 4, 5], [1, 2, 5], [2]):
                k = len(members)
                sub = lambda x: np.ascontiguousarray(np.asarray(x)[members])
                walk = lib.prefix_window_walk([0, k], sub(lens), sub(own_n), [1] * k, window)
                assert SpeckvKVConnector.prefix_window_walk([0, k], sub(lens), sub(own_n), [1] * k, window) == [(walk[0][0], walk[1][0])]
                first_tiles.add(walk[0][0])
                seen = {}
                for n_splits in (1, 2, 3, 5, 16, 0):
                    got, glse = _fold_w(torch, lib, [h], [0, k], LAYER, sub(q)[:, None], sub(lens), [1] * k, sub(own_n), None, window, sub(out), sub(lse), n_splits)
                    part = tuple(x[members] for x in ref)
                    _note("pieces", scheme, _assert_decode(got, glse, part, f"attend_prefix_fold_window {scheme} W {window} members {members} n_splits {n_splits}"))
                    seen[n_splits] = got
                assert np.array_equal(seen[0], seen[1])                  # the rule cuts nothing this short
                if window == 300:                                       # a row's range spans several pieces (under 33 it may lie in one)
                    assert not np.array_equal(seen[5], seen[1]), (scheme, window, members, "forced pieces did not run the piece launch")
                if members == [0, 1, 2, 3, 4, 5]:
                    via = _shared(torch, conn, LAYER, members, [P0] * n, q, lens, window=window, splits=5)
                    assert np.array_equal(via, seen[5]), (scheme, window, "attend_shared(window, splits=5)")
        assert first_tiles == {0, 13, 14, 11, 5}, first_tiles           # 0, inside the prefix, the last tile


# ----------------------------------------------------------------------------- 4. bit identities
@pytest.mark.parametrize("scheme", ALL)
def test_a_window_that_cuts_nothing_one_position_less_and_a_member_alone(scheme):
    """prefix_len + own <= 318 for every member: W = 318 cuts nothing and gives the bits of speckv_ext_attend_prefix_fold through the
    entry and through the connector (as does W = 0 at the entry); W = 317 moves exactly the member at the edge (254 + 64); and under
    W = 40 a member alone gives the bits it gives inside its group (the tiles in front of its bound add nothing, exactly)"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    lens, own_n = [254, 254, 98, 36, 254, 2, 64], [64, 37, 64, 1, 0, 2, 37]
    n = len(lens)
    q, rids, mine = q[:n], list(range(n)), [owns[k] for k in own_n]
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        h = conn.requests[P0].handle
        for window, edge in ((318, []), (317, [0])):
            out, lse = _own_step(torch, conn, LAYER, rids, q, window)
            want = _fold(torch, lib, [h], [0, n], LAYER, q[:, None], lens, [1] * n, out, lse)
            got = _fold_w(torch, lib, [h], [0, n], LAYER, q[:, None], lens, [1] * n, own_n, None, window, out, lse)
            via = _shared(torch, conn, LAYER, rids, [P0] * n, q, lens, window=window, splits=1)
            assert np.array_equal(via, got[0])
            for m in rids:
                same = np.array_equal(got[0][m], want[0][m]) and np.array_equal(got[1][m], want[1][m])
                assert same == (m not in edge), (scheme, window, m)
            if not edge:
                zero = _fold_w(torch, lib, [h], [0, n], LAYER, q[:, None], lens, [1] * n, own_n, None, 0, out, lse)
                assert np.array_equal(zero[0], want[0]) and np.array_equal(zero[1], want[1])
        out, lse = _own_step(torch, conn, LAYER, rids, q, 40)
        group = _fold_w(torch, lib, [h], [0, n], LAYER, q[:, None], lens, [1] * n, own_n, None, 40, out, lse)
        for m in rids:
            one = _fold_w(torch, lib, [h], [0, 1], LAYER, q[m:m + 1, None], lens[m:m + 1], [1], own_n[m:m + 1], None, 40, out[m:m + 1], lse[m:m + 1])
            assert np.array_equal(one[0][0], group[0][m]) and np.array_equal(one[1][0], group[1][m]), (scheme, m)


# ----------------------------------------------------------------------------- 5. / 6. chunks and trees
def _tree_rows(q, new, members, trees, n_new, window):
    """the rows of a chunk or tree step: q [M][S][H][R][D], new (k, v) [M][S][L][H][D], members[m] = (prefix, plen, own), trees[m] =
    parents; every live node as a row that sees the last W positions on its root path -> (rows, [(m, j)])"""
    rows, where = [], []
    for m, (prefix, plen, own) in enumerate(members):
        depth = SpeckvKVConnector.chunk_tree_depths(trees[m])[0]
        for j in range(n_new[m]):
            path, a = [], j
            while a >= 0:
                path.append(a)
                a = trees[m][a]
            pre, mine, on_path = _visible(plen, own[0].shape[1], depth[j], window, [depth[a] for a in path])
            rows.append((q[m, j], prefix, pre, own, mine, [(new[0][m, path[k]], new[1][m, path[k]]) for k in on_path]))
            where.append((m, j))
    return rows, where


def _judge_step(oracle, scheme, layer, got, q, new, members, trees, n_new, window, what, family):
    """got [M][S][H][R][D] fp32 of a chunk or tree step against float64; rows of dead nodes are zeros"""
    rows, where = _tree_rows(q, new, members, trees, n_new, window)
    ref = _want(oracle, scheme, layer, rows)
    flat = np.stack([got[m, j] for m, j in where])
    _note(family, scheme, _assert_decode(flat.view(np.int32), None, ref, what))
    for m, k in enumerate(n_new):
        assert not got[m, k:].any(), (what, m, "a dead node's row is not zero")


def _chain(S_):
    return list(range(-1, S_ - 1))


def _random_tree(rng, S_):
    return [-1] + [int(rng.integers(-1, j)) for j in range(1, S_)]


def _step_inputs(seed, M, S_, R):
    rng = np.random.default_rng(seed)
    return _rows(rng, M, S_, H, R, D), (_rows(rng, M, S_, L, H, D), _rows(rng, M, S_, L, H, D)), rng


STEP_LENS, STEP_OWN = [98, 254, 36, 64, 2, 98], [0, 37, 1, 2, 64, 64]


@pytest.mark.parametrize("S_,window", [(5, 4), (33, 20), (70, 40)])
@pytest.mark.parametrize("scheme", ALL)
def test_chunks_under_a_window_whose_later_rows_lose_the_prefix(oracle, scheme, S_, window):
    """attend_chunk_shared(window=W) with chunks of 5, 33 and 70 positions over members that hold 0, 37, 1, 2, 64, 64 positions: a
    row loses the prefix from position W - 1 - length on, so earlier rows keep it while later ones lose it, and the members of 64
    see none of it.  Against float64; and the entry over a fill pattern in the rows that are dead by the rule leaves it there"""
    torch = torch_mod()
    prefix, _, owns, _ = _inputs(4)
    M = len(STEP_LENS)
    q, new, _ = _step_inputs(500 + S_, M, S_, 4)
    n_new = [S_, S_, max(S_ - 3, 1), S_, S_, 0]
    mine = [owns[k] for k in STEP_OWN]
    rids = list(range(M))
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        for layer in range(L) if S_ == 33 else [LAYER]:
            got = conn.attend_chunk_shared(layer, rids, [P0] * M, _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1]), SM, n_new=n_new,
                                           prefix_lens=STEP_LENS, window=window)
            torch.cuda.synchronize()
            _judge_step(oracle, scheme, layer, got.cpu().numpy(), q, new, [(prefix, STEP_LENS[m], mine[m]) for m in rids], [_chain(S_)] * M, n_new,
                        window, f"attend_chunk_shared {scheme} S {S_} W {window} layer {layer}", "chunk")
        live = np.asarray([[j < n_new[m] and STEP_OWN[m] + 1 + j < window for j in range(S_)] for m in rids])
        assert live.any() and not live[:, -1].any() and live[0, 0] and not live[4].any()
        out, lse = np.full((M, S_, H, 4, D), PATTERN, np.int32), np.full((M, S_, H, 4), PATTERN, np.int32)
        out[live], lse[live] = 0, NEG_INF
        for n_splits in (1, 3):
            got, glse = _fold_w(torch, lib, [conn.requests[P0].handle], [0, M], LAYER, q, STEP_LENS, n_new, [k + 1 for k in STEP_OWN], None, window,
                                out, lse, n_splits)
            assert np.all(got[~live] == PATTERN) and np.all(glse[~live] == PATTERN), (scheme, S_, n_splits, "a dead row was written")
            assert not np.any(glse[live] == NEG_INF) and np.all(np.isfinite(_f32(got)[live]))


def _trees(S_):
    rng = np.random.default_rng(900 + S_)
    return {"random": [_random_tree(rng, S_) for _ in STEP_LENS], "star": [[-1] * S_] * len(STEP_LENS)}


@pytest.mark.parametrize("S_", [5, 16, 33, 70])
@pytest.mark.parametrize("scheme", ALL)
def test_trees_on_global_and_local_layers_against_float64(oracle, scheme, S_):
    """random trees of 5, 16, 33 and 70 nodes (deep nodes in front of roots inside a wave) and the star, one tree per member:
    attend_chunk_shared(parents=) against the masked chunk's reference plus the whole prefix; attend_tree_shared(window=W) for
    W = 1, 2, 33, 100, 300 against what each node sees on its root path, restated by brute force; attend_tree_shared(window=None)
    gives the bits of attend_chunk_shared(parents=)"""
    torch = torch_mod()
    prefix, _, owns, _ = _inputs(4)
    M = len(STEP_LENS)
    q, new, _ = _step_inputs(600 + S_, M, S_, 4)
    n_new = [S_, S_, max(S_ - 3, 1), S_, S_, 0]
    mine = [owns[k] for k in STEP_OWN]
    rids = list(range(M))
    members = [(prefix, STEP_LENS[m], mine[m]) for m in rids]
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        dq, dk, dv = _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1])
        for name, trees in _trees(S_).items():
            glob = conn.attend_chunk_shared(LAYER, rids, [P0] * M, dq, dk, dv, SM, n_new=n_new, prefix_lens=STEP_LENS, parents=trees)
            same = conn.attend_tree_shared(LAYER, rids, [P0] * M, dq, dk, dv, SM, trees, n_new=n_new, prefix_lens=STEP_LENS)
            assert np.array_equal(_bits(torch, glob), _bits(torch, same)), (scheme, S_, name)
            _judge_step(oracle, scheme, LAYER, glob.cpu().numpy(), q, new, members, trees, n_new, None,
                        f"attend_chunk_shared(parents) {scheme} {name} tree of {S_}", "tree global")
            for window in (1, 2, 33, 100, 300):
                got = conn.attend_tree_shared(LAYER, rids, [P0] * M, dq, dk, dv, SM, trees, n_new=n_new, prefix_lens=STEP_LENS, window=window)
                torch.cuda.synchronize()
                _judge_step(oracle, scheme, LAYER, got.cpu().numpy(), q, new, members, trees, n_new, window,
                            f"attend_tree_shared {scheme} {name} tree of {S_} W {window}", "tree local")


@pytest.mark.parametrize("scheme", ALL)
def test_a_chain_given_as_a_tree_agrees_with_the_windowed_chunk(oracle, scheme):
    """a chain of 33 as parents j - 1: attend_tree_shared(window=20) and attend_chunk_shared(window=20) both meet the float64 reference
    of the same rows (they agree within two bounds, not bit for bit: the own parts are two launches' roundings)"""
    torch = torch_mod()
    prefix, _, owns, _ = _inputs(4)
    M, S_, window = len(STEP_LENS), 33, 20
    q, new, _ = _step_inputs(733, M, S_, 4)
    n_new = [S_] * M
    mine = [owns[k] for k in STEP_OWN]
    rids = list(range(M))
    members = [(prefix, STEP_LENS[m], mine[m]) for m in rids]
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        dq, dk, dv = _dev(torch, q), _dev(torch, new[0]), _dev(torch, new[1])
        tree = conn.attend_tree_shared(LAYER, rids, [P0] * M, dq, dk, dv, SM, _chain(S_), prefix_lens=STEP_LENS, window=window)
        chunk = conn.attend_chunk_shared(LAYER, rids, [P0] * M, dq, dk, dv, SM, prefix_lens=STEP_LENS, window=window)
        torch.cuda.synchronize()
        for got, what in ((tree, "as a tree"), (chunk, "as a chunk")):
            _judge_step(oracle, scheme, LAYER, got.cpu().numpy(), q, new, members, [_chain(S_)] * M, n_new, window,
                        f"a chain of {S_} {what} {scheme} W {window}", "chain as tree")


# ----------------------------------------------------------------------------- 7. end to end
def _end_to_end(torch, oracle, scheme, pre_scale, window=24, **env):
    """a 64-position prefix in front of three members on a model whose layer 0 is local (W) and whose layer 1 is global: six decode
    steps (attend_shared(window) / attend_shared, append), then a tree step (attend_tree_shared on both layers) and
    commit(nodes=path), then one more decode step.  Every step against float64 -- with the K pre-scale over what the kernels are
    given -- and the forked twins, which hold copies of the prefix, at every step too: over INT4 against the SAME reference, over FP8
    and MXFP4 against the reference of their own composition (attend quantises the query over the prefix part as well)"""
    from tests.test_gpu_chunk import _f16_times, _kscale
    rng = np.random.default_rng(97)
    ks = _kscale() if pre_scale else np.ones((L, H, D), np.float32)
    inv = 1.0 / ks
    scaled = lambda k: _f16_times(k, inv[:, None])
    prefix = (_rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D))
    pre_prefix = (scaled(prefix[0]), prefix[1])
    M, R = 3, 4
    starts = [0, 5, 18]
    own = [(_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in starts]
    rids, twins = [0, 1, 2], [10, 11, 12]
    windows = [window, None]                                             # layer 0 local, layer 1 global
    with _world(torch, scheme, {P0: prefix}, own, kscale=ks if pre_scale else None, **env) as (lib, conn):
        keep = [conn.fork([P0] * M, twins)]
        for m, (k, v) in enumerate(own):                                 # the twins take the members' own prompts behind their copy
            for t_ in range(starts[m]):
                keep.append(conn.append([twins[m]], _dev(torch, np.ascontiguousarray(k[:, t_])[None]), _dev(torch, np.ascontiguousarray(v[:, t_])[None])))
        if env:                                                          # a migrated page of the prefix inside the window
            h = conn.requests[P0].handle
            lib.migrate(h, 0 * T + 25, 3, 1)
            lib.migrate(h, 0 * T + T // 2 + 28, 2, 0)
        worst = twin_worst = 0.0

        def decode_step(step):
            nonlocal worst, twin_worst, own
            q = _rows(rng, L, M, H, R, D)
            kn, vn = _rows(rng, M, L, H, D), _rows(rng, M, L, H, D)
            for layer in range(L):
                W = windows[layer]
                qs = _f16_times(q[layer], ks[layer][None, :, None, :])
                mine = [(scaled(k), v) for k, v in own]
                got = _shared(torch, conn, layer, rids, [P0] * M, q[layer], window=W)
                ref = _want(oracle, scheme, layer, _decode_rows(qs, [(pre_prefix, 64, mine[m]) for m in range(M)], W), quant_own=True)
                worst = max(worst, _assert_decode(got, None, ref, f"attend_shared {scheme} W {W} step {step} layer {layer}"))
                twin = _bits(torch, conn.attend(layer, twins, _dev(torch, q[layer]), SM, window=W))
                if scheme == "int4":
                    _assert_decode(twin, None, ref, f"fork + attend {scheme} against the shared reference, W {W} step {step} layer {layer}")
                whole = [(np.concatenate([pre_prefix[0], k], axis=1), np.concatenate([pre_prefix[1], v], axis=1)) for k, v in mine]
                ref = _want(oracle, scheme, layer, _decode_rows(qs, [(None, 0, whole[m]) for m in range(M)], W), quant_own=True)
                twin_worst = max(twin_worst, _assert_decode(twin, None, ref, f"fork + attend {scheme} W {W} step {step} layer {layer}"))
            dkn, dvn = _dev(torch, kn), _dev(torch, vn)
            keep.extend([conn.append(rids, dkn, dvn), conn.append(twins, dkn, dvn)])
            own = [(np.concatenate([k, kn[m][:, None]], axis=1), np.concatenate([v, vn[m][:, None]], axis=1)) for m, (k, v) in enumerate(own)]

        for step in range(6):
            decode_step(step)
        # the tree step: 9 nodes, two branches; the accepted path is committed in the members and in the twins
        tree = [-1, 0, 1, 1, 0, 4, 5, -1, 7]
        S_, path = len(tree), [0, 4, 5, 6]
        qt, new = _rows(rng, L, M, S_, H, R, D), (_rows(rng, M, S_, L, H, D), _rows(rng, M, S_, L, H, D))
        dk, dv = _dev(torch, new[0]), _dev(torch, new[1])
        new_pre = (_f16_times(new[0], inv[None, None]), new[1])
        for layer in range(L):
            W = windows[layer]
            qs = _f16_times(qt[layer], ks[layer][None, None, :, None, :])
            mine = [(scaled(k), v) for k, v in own]
            got = conn.attend_tree_shared(layer, rids, [P0] * M, _dev(torch, qt[layer]), dk, dv, SM, tree, window=W)
            torch.cuda.synchronize()
            members = [(pre_prefix, 64, mine[m]) for m in range(M)]
            _judge_step(oracle, scheme, layer, got.cpu().numpy(), qs, new_pre, members, [tree] * M, [S_] * M, W,
                        f"attend_tree_shared {scheme} W {W} end to end, layer {layer}", "end to end")
            twin = conn.attend_tree(layer, twins, _dev(torch, qt[layer]), dk, dv, SM, tree, window=W)
            torch.cuda.synchronize()
            whole = [(None, 0, (np.concatenate([pre_prefix[0], k], axis=1), np.concatenate([pre_prefix[1], v], axis=1))) for k, v in mine]
            _judge_step(oracle, scheme, layer, twin.cpu().numpy(), qs, new_pre, whole, [tree] * M, [S_] * M, W,
                        f"fork + attend_tree {scheme} W {W} end to end, layer {layer}", "end to end")
        keep.append(conn.commit(rids, dk, dv, [path] * M))
        keep.append(conn.commit(twins, dk, dv, [path] * M))
        own = [(np.concatenate([k] + [new[0][m, j][:, None] for j in path], axis=1), np.concatenate([v] + [new[1][m, j][:, None] for j in path], axis=1))
               for m, (k, v) in enumerate(own)]
        decode_step(6)
        torch.cuda.synchronize()
        for m, r in enumerate(rids):
            assert conn.length(r) == starts[m] + 6 + len(path) + 1 and conn.length(twins[m]) == 64 + conn.length(r)
        assert conn.length(P0) == 64
        _note("end to end", scheme, worst)
        _note("end to end twins", scheme, twin_worst)
        del keep


@pytest.mark.parametrize("pre_scale", [False, True], ids=["plain", "k-pre-scale"])
@pytest.mark.parametrize("scheme", ALL)
def test_connector_end_to_end_over_alternating_local_and_global_layers(oracle, scheme, pre_scale):
    _end_to_end(torch_mod(), oracle, scheme, pre_scale)


def test_end_to_end_on_a_pool_striped_over_three(oracle):
    _end_to_end(torch_mod(), oracle, "int4", False, SPECKV_POOL_DEVICES="0,0,0")


def test_end_to_end_with_a_migrated_page_of_the_prefix(oracle):
    _end_to_end(torch_mod(), oracle, "fp8", False, SPECKV_POOL_DEVICES="0,0")


# ----------------------------------------------------------------------------- 8. refusals
def test_the_window_entry_refuses_bad_arguments_and_capture_and_launches_nothing():
    torch = torch_mod()
    prefix, second, owns, q = _inputs(4)
    n = 4
    q, lens = q[:n, None], [98, 36, 2, 64]
    out, lse = np.full((n, 1, H, 4, D), PATTERN, np.int32), np.full((n, 1, H, 4), PATTERN, np.int32)
    with _world(torch, "fp8", {P0: prefix, P1: second}, []) as (lib, conn):
        h0, h1 = conn.requests[P0].handle, conn.requests[P1].handle
        lib.set_compression_scheme(3)
        int4 = lib.alloc(2 * T * L * H * D * 2); lib.set_layout(int4, T, L, H, D, 2)
        lib.set_compression_scheme(4)
        dq, do, dl = _dev(torch, q), _dev(torch, out), _dev(torch, lse)
        depth = _dev(torch, np.zeros(n + 1, np.int32))
        st = torch.cuda.Stream()
        torch.cuda.synchronize()

        def call(**change):
            args = dict(prefix_handles=np.asarray([h0, h1], np.uint64), first_member=np.asarray([0, 2, 4], np.uint32), layer=LAYER, d_q=dq.data_ptr(),
                        C=1, rows_per_pos=4, prefix_len=np.asarray(lens, np.uint32), n_q=np.ones(n, np.uint32), own_seen=np.asarray([3, 0, 1, 7], np.uint32),
                        d_depth=0, window=40, n_splits=1, sm_scale=SM, d_out=do.data_ptr(), d_lse=dl.data_ptr(), stream=st.cuda_stream)
            args.update(change)
            lib.attend_prefix_fold_window(**args)

        def refused(status, what, **change):
            with pytest.raises(SpeckvError) as e:
                call(**change)
                pytest.fail(what)
            assert e.value.status == status, (what, e.value.status)
            st.synchronize(); torch.cuda.synchronize()
            assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all()), (what, "a refused call wrote out / lse")

        u32 = lambda *xs: np.asarray(xs, np.uint32)
        invalid = {
            "NULL own_seen": dict(own_seen=None), "NULL own_seen without a window": dict(own_seen=None, window=0),
            "a misaligned d_depth": dict(d_depth=depth.data_ptr() + 2), "a misaligned d_depth without a window": dict(d_depth=depth.data_ptr() + 2, window=0),
            "NULL stream": dict(stream=0), "NULL q": dict(d_q=0), "NULL out": dict(d_out=0), "NULL lse": dict(d_lse=0),
            "a misaligned q": dict(d_q=dq.data_ptr() + 8), "a misaligned out": dict(d_out=do.data_ptr() + 8), "rows_per_pos 3": dict(rows_per_pos=3),
            "C 0": dict(C=0), "an odd prefix_len": dict(prefix_len=u32(98, 35, 2, 64)), "a prefix_len beyond the layout": dict(prefix_len=u32(98, 36, 2, T + 2)),
            "n_q > C": dict(n_q=u32(1, 2, 1, 1)), "first_member not from 0": dict(first_member=u32(1, 2, 4)),
            "first_member descending": dict(first_member=u32(0, 3, 2)), "mixed schemes": dict(prefix_handles=np.asarray([h0, int4], np.uint64)),
            "mixed schemes, forced pieces": dict(prefix_handles=np.asarray([h0, int4], np.uint64), n_splits=3),
            "a layer beyond the layout": dict(layer=L), "n_splits 65": dict(n_splits=65),
        }
        for what, change in invalid.items():
            refused(-4, what, **change)                                      # SPECKV_ERR_INVAL
        refused(-1, "an unknown handle", prefix_handles=np.asarray([h0, 0xDEAD], np.uint64))
        # the same buffers ARE written by the call that is not refused -- with a depth table, 4-byte aligned, too
        ok_out, ok_lse = torch.zeros_like(do), torch.full_like(dl, int(NEG_INF))
        torch.cuda.synchronize()
        call(d_out=ok_out.data_ptr(), d_lse=ok_lse.data_ptr(), d_depth=depth.data_ptr() + 4)
        st.synchronize()
        assert not bool((ok_lse == int(NEG_INF)).any())
        # capture: refused, nothing launched
        s = torch.cuda.Stream()
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            with pytest.raises(SpeckvError) as e:
                call(stream=s.cuda_stream)
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all())
        lib.free(int4)


# ----------------------------------------------------------------------------- 9. the example
def test_the_shared_prefix_window_example_runs():
    """examples/shared_prefix_window_example.py in this process, short: a system prompt in front of users on a model with alternating
    local and global layers, decode steps and a tree step, compared against forked twins"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "shared_prefix_window_example.py")
    spec = importlib.util.spec_from_file_location("shared_prefix_window_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run("int4", prompt=98, users=5, steps=4, window=40, verbose=False) == 5 * (4 + 1)
