"""-m gpu: draft trees on sliding-window layers -- speckv_ext_attend_chunk_tree_window (k_attend_chunk's MASKED + WINDOW form, whole
and split) and SpeckvKVConnector.attend_tree on top of it.

Reference and bound are those of tests/test_gpu_chunk_tree.py and tests/test_gpu_chunk_window.py, unchanged: numpy float64 softmax
attention with the fp16 query as given, the oracle's records (HeadChecker.kv) for the stored part, the fp16 held rows for the rest;
|err| <= 2e-3 sum p|v| + 1e-6 and |lse err| <= 2e-3, the sum over what the row sees.  WHAT a row sees is restated here by brute force
(_sees), never taken from chunk_tree_masks or the kernel: a request holds length = pos_end + base positions, node j of depth d sits at
P = length + d and sees [lo, P] on its root path, lo = max(0, P + 1 - W): stored t iff lo <= t < pos_end, the tail (absolute position
pos_end) iff base == 1 and pos_end >= lo, ancestor a iff length + depth(a) >= lo, itself always.

Shapes: L = 2, T = 256, the prompts of tests/test_gpu_chunk.py (0, 1, 2, 37, 64, 98 positions) with trees of 5, 16, 33 and 70 nodes; the
split form at T = 512 over the prompts of tests/test_gpu_chunk_split.py (up to 481 positions)."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_chunk_split as split
from tests._gpu import D, H, graph_capture, torch_mod
from tests.test_gpu_chunk import (L, LAYER, PATTERN, PROMPTS, RIDS, S, SM, T, _batch, _f16_times, _f32, _inputs, _kscale, _rows, _stored64)
from tests.test_gpu_chunk_tree import _entry_m, _longest_path
from tests.test_gpu_chunk_window import _check as _check_chain
from tests.test_gpu_chunk_window import _entry as _window_entry
from tests.test_gpu_chunk_window import _hostile, _scores
from tests.test_gpu_spec_step import SCHEMES

pytestmark = pytest.mark.gpu
ALL = ["fp8", "int4", "mxfp4"]
WINDOWS = [1, 2, 31, 32, 33, 40, 64, 100, 300]
BASES = [p & 1 for p in PROMPTS]
N_TW = [70, 33, 17, 16, 40, 70]                      # live counts over the prompts of 0, 1, 2, 37, 64 and 98 positions
FULL = [S] * len(PROMPTS)
DEEP_FIRST = [-1 if j % 9 == 0 else j - 1 for j in range(S)]      # chains of 9: a root right behind a node of depth 8, over and over
CHAIN = list(range(-1, S - 1))


# ----------------------------------------------------------------------------- the test's own rules
def _depths(tree):
    d = []
    for p in tree:
        d.append(0 if p < 0 else d[p] + 1)
    return d


def _sees(tree, n, pos_end, base, window):
    """by walking up from every node: live [S] (the node and its ancestors are all < n) and seen [S][pos_end + base + S] by absolute
    position, under window (0: none)"""
    n_nodes, length, depth = len(tree), pos_end + base, _depths(tree)
    live, seen = np.zeros(n_nodes, bool), np.zeros((n_nodes, length + n_nodes), bool)
    for j in range(n_nodes):
        lo = max(0, length + depth[j] + 1 - window) if window else 0
        seen[j, min(lo, pos_end):pos_end] = True
        if base and pos_end >= lo:
            seen[j, pos_end] = True
        a, ok = j, True
        while a >= 0:
            ok = ok and a < n
            if a == j or length + depth[a] >= lo:
                seen[j, length + a] = True
            a = tree[a]
        live[j] = ok
    return live, seen


def _words(tree, n, base, window, words=None):
    """mask rows uint32 [S][words] built bit by bit from _sees (the rows do not depend on pos_end: 64 serves)"""
    n_nodes = len(tree)
    words = words or (n_nodes + 1 + 31) // 32
    live, seen = _sees(tree, n, 64, base, window)
    rows = np.zeros((n_nodes, words), np.uint32)
    for j in np.nonzero(live)[0]:
        for t in np.nonzero(seen[j, 64:])[0]:
            rows[j, t >> 5] |= np.uint32(1 << (int(t) & 31))
    return rows


def _tables(trees, n_new, bases, window):
    return (np.stack([_words(t, n, b, window) for t, n, b in zip(trees, n_new, bases)]),
            np.asarray([_depths(t) for t in trees], np.uint32))


def _random_trees(seed, n_nodes, count=len(PROMPTS)):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(max(-1, j - 6), j)) for j in range(n_nodes)] for _ in range(count)]


def _entry(torch, lib, conn, rids, q, k_new, v_new, n_new, masks, depths, window, n_splits=1, keep=None, **kw):
    """speckv_ext_attend_chunk_tree_window over what the connector holds: (out, lse) as numpy int32 bit patterns"""
    _, args, out, lse, st, held = split._stage(torch, conn, rids, q, k_new, v_new, n_new, None, masks, entry="masked", **kw)
    dd = torch.from_numpy(np.ascontiguousarray(depths).view(np.int32)).cuda()
    args.setdefault("d_depth", dd.data_ptr())
    args.setdefault("window", window)
    args.setdefault("n_splits", n_splits)
    if keep is not None:
        keep.update(out=out, lse=lse, args=args, held=(held, dd))
    torch.cuda.synchronize()
    lib.attend_chunk_tree_window(**args)
    st.synchronize()
    del held, dd
    return out.cpu().numpy(), lse.cpu().numpy()


def _check(stored, conn, b, rid, prompt, q, new, tree, n, outs, what, layer=LAYER, rows=None):
    """request b's live rows (or those of `rows`) against float64 at `layer` for every (window, out, lse) of outs; the scores are computed
    once per head and shared by the windows.  Returns the worst err / tol per window"""
    k, v = prompt
    even, base = k.shape[1] & ~1, k.shape[1] & 1
    r = conn.requests[rid]
    R, n_nodes = q.shape[3], len(tree)
    worst = {w: 0.0 for w, _, _ in outs}
    sees = {w: _sees(tree, n, even, base, w) for w, _, _ in outs}
    for head in range(H):
        K, V = stored(k, v, head)
        tail = None if not r.length & 1 else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        s_all, Va, _ = _scores(K[:even], V[:even], tail, q[b, :n_nodes, head], new[0][b, :n_nodes, layer, head], new[1][b, :n_nodes, layer, head])
        for w, out, lse in outs:
            live, seen = sees[w]
            pick = np.nonzero(live)[0] if rows is None else np.asarray([j for j in rows if live[j]], int)
            if not len(pick):
                continue
            at = (pick[:, None] * R + np.arange(R)[None]).reshape(-1)
            s = np.where(seen[pick].repeat(R, axis=0), s_all[at], -np.inf)
            mx = s.max(axis=1)
            p = np.exp(s - mx[:, None])
            l = p.sum(axis=1)
            want, wlse, mag = (p @ Va) / l[:, None], mx + np.log(l), (p @ np.abs(Va)) / l[:, None]
            got = _f32(out)[b, pick, head].reshape(-1, D)
            assert np.all(np.isfinite(got)), (what, w, b, head, "not finite")
            err, tol = np.abs(got - want), 2e-3 * mag + 1e-6
            lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, pick, head].reshape(-1) - wlse)
            worst[w] = max(worst[w], float((err / tol).max()), float(lerr.max() / 2e-3))
            assert np.all(err <= tol), (what, w, b, head, "out", float((err / tol).max()))
            assert np.all(lerr <= 2e-3), (what, w, b, head, "lse", float(lerr.max()))
    return worst


def _stored256(oracle, scheme, b, layer=LAYER):
    return lambda k, v, head: _stored64(oracle, scheme, b, k, v, head, layer)


def _merge(into, worst):
    for w, x in worst.items():
        into[w] = max(into.get(w, 0.0), x)


def _show(worst):
    return ", ".join(f"W {w}: {x:.3f}" for w, x in worst.items())


def _run_trees(torch, oracle, scheme, lib, conn, prompts, q, new, trees, n_new, windows, what, layer=LAYER, n_splits=1):
    """the batch under every window against float64; dead rows keep the fill pattern"""
    n_nodes = len(trees[0])
    qs, ns = np.ascontiguousarray(q[:, :n_nodes]), (np.ascontiguousarray(new[0][:, :n_nodes]), np.ascontiguousarray(new[1][:, :n_nodes]))
    outs = []
    for w in windows:
        masks, depths = _tables(trees, n_new, BASES, w)
        outs.append((w,) + _entry(torch, lib, conn, RIDS, qs, ns[0], ns[1], n_new, masks, depths, w, n_splits, layer=layer, fill=PATTERN))
    worst = {}
    for b in RIDS:
        live, _ = _sees(trees[b], n_new[b], 0, 0, 0)
        for w, out, lse in outs:
            assert np.all(out[b, ~live] == PATTERN) and np.all(lse[b, ~live] == PATTERN), (what, w, b, "a dead row was written")
            assert not np.any(lse[b, live] == PATTERN), (what, w, b, "a live row was not written")
        if live.any():
            _merge(worst, _check(_stored256(oracle, scheme, b, layer), conn, b, b, prompts[b], qs, ns, trees[b], n_new[b], outs, what, layer=layer))
    return worst


# ----------------------------------------------------------------------------- 1. random trees
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_random_trees_under_windows_against_float64(oracle, scheme, rpp):
    """one seeded random tree per request with 5, 16, 33 and 70 nodes (1 to 3 mask words, 1 to 18 query blocks), prompts with and
    without a tail, ragged n_new (dead nodes, and nodes below them), windows of 1, 2, around a tile, 40, 64, 100 and 300; the masks and
    depths handed to the entry are built here and are what the connector builds; both layers at 70 nodes"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        for n_nodes in (5, 16, 33, 70):
            trees = _random_trees(70 + n_nodes, n_nodes)
            n_new = [min(n, n_nodes) for n in N_TW]
            n_new[1] = max(n_nodes - 2, 1)
            for w in (2, 33):
                assert np.array_equal(_tables(trees, n_new, BASES, w)[0], np.asarray(SpeckvKVConnector.chunk_tree_masks(trees, BASES, n_new, window=w), np.uint32))
            assert np.array_equal(_tables(trees, n_new, BASES, 2)[1], np.asarray(SpeckvKVConnector.chunk_tree_depths(trees, len(trees)), np.uint32))
            for layer in range(L) if n_nodes == 70 else (LAYER,):
                worst = _run_trees(torch, oracle, scheme, lib, conn, prompts, q, new, trees, n_new, WINDOWS, ("random", scheme, rpp, n_nodes), layer)
                print(f"attend_chunk_tree_window {scheme} rows_per_pos {rpp} {n_nodes} nodes layer {layer}: worst err / tol {_show(worst)}")


# ----------------------------------------------------------------------------- 2. node order, star, chains
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_a_deep_node_in_front_of_a_root_the_star_and_a_chain_deeper_than_the_window(oracle, scheme, rpp):
    """chains of 9 nodes one behind the other: a root stands right behind a node of depth 8 inside one wave (rows_per_pos 1 and 4) and
    inside one query block (every rows_per_pos), and under W = 40 over 98 positions depth 0 starts in pool tile 1, depth >= 5 in tile
    2 -- a bound or a first tile taken from a wave's or a block's first row loses positions 59..63 for the roots.  The star (all depth
    0).  A chain of 70 under W of 8 and 33: ancestors drop out, and from depth W - 1 on no stored position and no tail is seen"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        for name, tree, windows in (("deep first", DEEP_FIRST, (40, 33, 8, 3)), ("star", [-1] * S, (40, 1)), ("chain", CHAIN, (8, 33))):
            worst = _run_trees(torch, oracle, scheme, lib, conn, prompts, q, new, [tree] * len(PROMPTS), N_TW, windows, (name, scheme, rpp))
            print(f"attend_chunk_tree_window {scheme} rows_per_pos {rpp} {name}: worst err / tol {_show(worst)}")


@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_a_chain_given_as_a_tree_against_the_chain_window(oracle, scheme, rpp):
    """parents[j] = j - 1: within the bound of the float64 CHAIN reference of tests/test_gpu_chunk_window.py, the one
    speckv_ext_attend_chunk_window's output is held to in the same breath -- so the two agree within two tolerances, not bit for bit
    (the walks start at different tiles)"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        outs = []
        for w in (2, 33, 40, 100):
            masks, depths = _tables([CHAIN] * len(PROMPTS), N_TW, BASES, w)
            outs.append((w,) + _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_TW, masks, depths, w))
        worst = {}
        for b in RIDS:
            _merge(worst, _check_chain(_stored256(oracle, scheme, b), conn, b, b, prompts[b], q, new, N_TW[b], outs, ("chain as tree", scheme, rpp)))
        print(f"attend_chunk_tree_window {scheme} rows_per_pos {rpp} chain as a tree: worst err / tol {_show(worst)}")
        chains = [(w,) + _window_entry(torch, lib, conn, RIDS, q, new[0], new[1], N_TW, w) for w, _, _ in outs]
        for b in RIDS:                                  # the chain entry against the same reference: the two are within two tolerances
            _check_chain(_stored256(oracle, scheme, b), conn, b, b, prompts[b], q, new, N_TW[b], chains, ("the chain entry", scheme, rpp))


# ----------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_a_window_that_cuts_nothing_gives_the_masked_bits_and_one_position_less_moves_the_deepest_rows(scheme, rpp):
    """window 0 and windows >= pos_end + base + n_q of every request: the bits of speckv_ext_attend_chunk_masked / _split with the same
    mask (the engine issues that launch; the depths are not read).  W = 98 + max depth + 1 < 168: the call runs on the tree-window
    instances, no node loses a position, every block walks from tile 0 in the same order -- still the masked entry's bits.  One less:
    exactly the deepest nodes of the 98-position request lose stored position 0 and change; every other row keeps its bits"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    trees = _random_trees(33, S)
    depth5 = np.asarray(_depths(trees[5]))
    deepest = int(depth5.max())
    assert 3 < deepest < 40
    with _batch(torch, scheme, prompts) as (lib, conn):
        masks, depths = _tables(trees, FULL, BASES, 0)
        want = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, fill=PATTERN)
        assert not np.all(want[0] == PATTERN)
        reach = max(p + n for p, n in zip(PROMPTS, FULL))
        assert reach == 168
        for window, n_splits in ((0, 1), (reach, 1), (reach, 0), (reach, 5), (10 ** 6, 1), (0xFFFFFFFF, 0)):
            got = _entry(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, depths + (7 if window != reach else 0), window, n_splits, fill=PATTERN)
            ref = split._entry(torch, lib, conn, RIDS, q, new[0], new[1], FULL, 5, masks, fill=PATTERN) if n_splits == 5 else want
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (scheme, rpp, window, n_splits)
        tight = 98 + deepest + 1
        masks_w, _ = _tables(trees, FULL, BASES, tight)
        assert np.array_equal(masks_w, masks)                                # deep enough for every ancestor and tail
        got = _entry(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks_w, depths, tight, fill=PATTERN)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scheme, rpp, "no node loses a position")
        masks_1, _ = _tables(trees, FULL, BASES, tight - 1)
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks_1, depths, tight - 1, fill=PATTERN)
        moved = np.stack([(_sees(tr, S, p & ~1, p & 1, tight - 1)[1] != _sees(tr, S, p & ~1, p & 1, 0)[1]).any(axis=1) for tr, p in zip(trees, PROMPTS)])
        assert np.array_equal(moved[5], depth5 == deepest) and moved[5].any() and not moved[:5].any()
        changed = (out != want[0]).any(axis=-1).reshape(len(PROMPTS), S, -1)
        assert changed[moved].all() and (lse != want[1]).reshape(len(PROMPTS), S, -1)[moved].all(), (scheme, rpp, "a row that lost a position kept its bits")
        assert not changed[~moved].any() and np.array_equal(lse[~moved], want[1][~moved]), (scheme, rpp, "a row that lost no position changed")


# ----------------------------------------------------------------------------- 4. hostile rows
@pytest.mark.parametrize("scheme", ALL)
def test_hostile_stored_rows_below_the_bounds_stay_out(oracle, scheme):
    """the 98-position prompt under W = 40 with the chains of 9 (lo = 59 + depth: 59 for the roots, 67 for the deepest nodes): stored
    positions [0, x) are K x 200, V = +-1000 for x around the shallowest bound (58, 59 and, one past it, 60) and the deepest (66, 67).
    Every row whose bound is at or above x -- all of them up to 59, the depths >= 1 at 60, the depths >= 7 and 8 at 66 and 67 -- sees
    none of them and goes against float64, whose sum p|v| runs over what the row sees; whole walk and 3 pieces"""
    torch = torch_mod()
    rpp = 4
    prompts, new, q = _inputs(rpp)
    k, v = prompts[5]
    edges = (58, 59, 60, 66, 67)
    depth = np.asarray(_depths(DEEP_FIRST))
    variants = []
    for x in edges:
        below = np.arange(x)
        variants.append((np.stack([_hostile(k[layer], below, "k") for layer in range(L)]), np.stack([_hostile(v[layer], below, "v") for layer in range(L)])))
    masks, depths = _tables([DEEP_FIRST], [S], [0], 40)
    with _batch(torch, scheme, variants) as (lib, conn):
        for at, x in enumerate(edges):
            for n_splits in (1, 3):
                out, lse = _entry(torch, lib, conn, [at], q[5:6], new[0][5:6], new[1][5:6], [S], masks, depths, 40, n_splits)
                stored = lambda kk, vv, head: _stored64(oracle, scheme, ("hostile", x), kk, vv, head)
                below = [int(j) for j in np.nonzero(59 + depth >= x)[0]]
                assert len(below) == {58: S, 59: S, 60: S - 8, 66: 14, 67: 7}[x]
                worst = _check(stored, conn, 0, at, variants[at], q[5:6], (new[0][5:6], new[1][5:6]), DEEP_FIRST, S, [(40, out, lse)],
                               ("hostile stored", scheme, x), rows=below)
                print(f"attend_chunk_tree_window {scheme} hostile stored rows below {x}, n_splits {n_splits}: worst err / tol {worst[40]:.3f}")


@pytest.mark.parametrize("scheme", ALL)
def test_a_hostile_tail_ancestors_out_of_the_window_and_siblings_stay_out(oracle, scheme):
    """the 37-position prompt (a tail) whose last position is K x 200, V = +-1000: under W = 3 the nodes of depth >= 2 do not see it
    and go against float64.  Then,
    for checked nodes of the chains of 9 on both sides of the mask words' edges, every new node the row does NOT see under W = 4 -- its
    ancestors further than 3 up, the other chains, what lies below it -- is K x 200, V x 1000"""
    torch = torch_mod()
    rpp = 4
    prompts, new, q = _inputs(rpp)
    k, v = prompts[3]
    last = np.asarray([36])
    hostile = (np.stack([_hostile(k[layer], last, "k") for layer in range(L)]), np.stack([_hostile(v[layer], last, "v") for layer in range(L)]))
    with _batch(torch, scheme, [hostile, prompts[3]]) as (lib, conn):
        stored = lambda kk, vv, head: _stored64(oracle, scheme, 3, kk, vv, head)
        masks, depths = _tables([DEEP_FIRST], [S], [1], 3)
        out, lse = _entry(torch, lib, conn, [0], q[3:4], new[0][3:4], new[1][3:4], [S], masks, depths, 3)
        out_of_reach = [j for j, d in enumerate(_depths(DEEP_FIRST)) if d >= 2]
        assert len(out_of_reach) == S - 16 and not _sees(DEEP_FIRST, S, 36, 1, 3)[1][out_of_reach, 36].any()
        worst = _check(stored, conn, 0, 0, hostile, q[3:4], (new[0][3:4], new[1][3:4]), DEEP_FIRST, S, [(3, out, lse)], ("hostile tail", scheme),
                       rows=out_of_reach)
        print(f"attend_chunk_tree_window {scheme} hostile tail out of W 3: worst err / tol {worst[3]:.3f}")
        masks, depths = _tables([DEEP_FIRST], [S], [1], 4)
        _, seen = _sees(DEEP_FIRST, S, 36, 1, 4)
        worst = 0.0
        for j in (4, 8, 9, 30, 31, 32, 35, 62, 63, 64, 69):
            hidden = ~seen[j, 37:]
            k2, v2 = new[0][3:4].copy(), new[1][3:4].copy()
            k2[:, hidden] = (k2[:, hidden].astype(np.float32) * 200).astype(np.float16)
            v2[:, hidden] = (v2[:, hidden].astype(np.float32) * 1000).astype(np.float16)
            assert hidden.sum() >= S - 4 and np.all(np.isfinite(k2)) and np.all(np.isfinite(v2))
            out, lse = _entry(torch, lib, conn, [1], q[3:4], k2, v2, [S], masks, depths, 4)
            worst = max(worst, _check(stored, conn, 0, 1, prompts[3], q[3:4], (k2, v2), DEEP_FIRST, S, [(4, out, lse)], ("hostile nodes", scheme, j), rows=[j])[4])
        print(f"attend_chunk_tree_window {scheme} hostile ancestors out of W 4 and siblings: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- 5. the probe on stored positions
@pytest.mark.parametrize("scheme", ALL)
def test_the_probe_on_stored_positions_goes_by_depth(scheme):
    """stored position t of the 98-position prompt negated, under W = 40 with the chains of 9 (lo_d = 59 + d): t = lo_d - 1 changes no
    row of depth >= d, t = lo_d changes exactly the rows of depth <= d -- for d = 0 (58: nobody; 59: the roots), d = 4 and 5 (the
    tile edge 63 / 64) and d = 8 (66, 67: everybody)"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    k, v = prompts[5]
    places = (58, 59, 62, 63, 64, 66, 67)
    variants = []
    for t in places:
        k2, v2 = k.copy(), v.copy()
        k2[:, t], v2[:, t] = -k2[:, t], -v2[:, t]
        variants.append((k2, v2))
    masks, depths = _tables([DEEP_FIRST], [S], [0], 40)
    depth = np.asarray(_depths(DEEP_FIRST))
    with _batch(torch, scheme, [prompts[5]] + variants) as (lib, conn):
        one = lambda rid: _entry(torch, lib, conn, [rid], q[5:6], new[0][5:6], new[1][5:6], [S], masks, depths, 40)
        out, lse = one(0)
        for at, t in enumerate(places):
            out2, lse2 = one(1 + at)
            sees = 59 + depth <= t
            changed = (out2[0] != out[0]).any(axis=-1).reshape(S, -1)
            assert changed[sees].all(), (scheme, t, "a row that sees the replaced position kept its bits")
            assert not changed[~sees].any() and np.array_equal(lse2[0][~sees], lse[0][~sees]), (scheme, t)
            assert sees.sum() == {58: 0, 59: 8, 67: S}.get(t, sees.sum()) and 0 < (59 + depth <= 63).sum() < (59 + depth <= 64).sum() < S


# ----------------------------------------------------------------------------- 6. split
N_SPLIT = [70, 33, 0, 16, 1, 70, 70]                # over split.PROMPTS = 0, 1, 2, 37, 98, 255, 481


@pytest.mark.parametrize("n_splits", [2, 3, 5, 0])
@pytest.mark.parametrize("scheme", ALL)
def test_pieces_under_a_window_against_float64(oracle, scheme, n_splits):
    """T = 512, prompts up to 481 positions, forced 2, 3 and 5 pieces and the rule, W in {33, 100, 300}, random trees and the chains
    of 9: the pieces start at a first tile > 0 and every block of a request shares it.  Live rows finite and within the float64
    bound, dead rows keep the fill pattern"""
    torch = torch_mod()
    t = split.T
    bases = [p & 1 for p in split.PROMPTS]
    with split._batch(torch, scheme, split._inputs(8)[0]) as (lib, conn):
        for rpp, trees in ((8, _random_trees(81, S, len(split.PROMPTS))), (1, [DEEP_FIRST] * len(split.PROMPTS))):
            prompts, new, q = split._inputs(rpp)
            outs = []
            for w in (33, 100, 300):
                masks = np.stack([_words(tr, n, b, w) for tr, n, b in zip(trees, N_SPLIT, bases)])
                depths = np.asarray([_depths(tr) for tr in trees], np.uint32)
                outs.append((w,) + _entry(torch, lib, conn, split.RIDS, q, new[0], new[1], N_SPLIT, masks, depths, w, n_splits, fill=PATTERN))
            if n_splits:
                plans = [SpeckvKVConnector.chunk_pieces(N_SPLIT, split.PROMPTS, rpp, n_splits, 256, window=w) for w, _, _ in outs]
                assert any(f > 0 and p > 1 for plan in plans for p, f in zip(plan[0], plan[3]))
            worst = {}
            for b in split.RIDS:
                live, _ = _sees(trees[b], N_SPLIT[b], 0, 0, 0)
                for w, out, lse in outs:
                    assert np.all(out[b, ~live] == PATTERN) and np.all(lse[b, ~live] == PATTERN), (scheme, n_splits, w, b)
                    assert np.all(np.isfinite(_f32(out)[b, live])) and np.all(np.isfinite(_f32(lse)[b, live])), (scheme, n_splits, w, b)
                if live.any():
                    stored = lambda k, v, head: split._stored64(oracle, scheme, k, v, head, LAYER, t)
                    _merge(worst, _check(stored, conn, b, b, prompts[b], q, new, trees[b], N_SPLIT[b], outs, ("pieces", scheme, n_splits, rpp)))
            print(f"attend_chunk_tree_window {scheme} n_splits {n_splits} rows_per_pos {rpp}: worst err / tol {_show(worst)}")


# ----------------------------------------------------------------------------- 7. placement
@pytest.mark.parametrize("scheme", ALL)
def test_a_tree_under_a_window_over_a_pool_striped_over_three(oracle, scheme):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts, SPECKV_POOL_DEVICES="0,0,0") as (lib, conn):
        worst = _run_trees(torch, oracle, scheme, lib, conn, prompts, q, new, _random_trees(91, S), N_TW, (40,), ("striped", scheme))
        print(f"attend_chunk_tree_window {scheme} striped over 3, W 40: worst err / tol {worst[40]:.3f}")


@pytest.mark.parametrize("scheme", ALL)
def test_pages_never_written_inside_the_window_count_as_zeros(oracle, scheme):
    """an allocation written through speckv_write except K page 13, V page 14 (positions 26..29) and the whole second tile of
    pos_end = 64, under W = 40 with a 33-node tree (lo of depth 0 = 25): all of them inside the window of some row"""
    import types
    torch = torch_mod()
    _, new, q = _inputs(4)
    rng = np.random.default_rng(71)
    k, v = _rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D)
    k[:, 26:28] = 0; v[:, 28:30] = 0
    k[:, 32:] = 0; v[:, 32:] = 0
    n = 33
    tree = _random_trees(72, n, 1)[0]
    with _batch(torch, scheme, []) as (lib, conn):
        lib.set_compression_scheme(SCHEMES[scheme])
        h = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(h, T, L, H, D, 2)
        page = lambda x, first, cnt: np.ascontiguousarray(x[LAYER, 2 * first:2 * (first + cnt)]).reshape(cnt, 2 * H * D)
        for x, region, skip in ((k, LAYER * T, 13), (v, LAYER * T + T // 2, 14)):
            for first, cnt in ((0, skip), (skip + 1, 16 - skip - 1)):
                img = page(x, first, cnt)
                lib.write(h, (region + first) * 4096, img.ctypes.data, img.nbytes, False)
        lib.sync()
        held = types.SimpleNamespace(requests={0: types.SimpleNamespace(handle=h, length=64, tail_k=None, tail_v=None)})
        qs, ns = np.ascontiguousarray(q[:1, :n]), (np.ascontiguousarray(new[0][:1, :n]), np.ascontiguousarray(new[1][:1, :n]))
        masks, depths = _tables([tree], [n], [0], 40)
        out, lse = _entry(torch, lib, held, [0], qs, ns[0], ns[1], [n], masks, depths, 40, fill=PATTERN)
        stored = lambda kk, vv, head: _stored64(oracle, scheme, 0, kk, vv, head)
        worst = _check(stored, held, 0, 0, (k, v), qs, ns, tree, n, [(40, out, lse)], ("never written", scheme))
        print(f"attend_chunk_tree_window {scheme} never-written pages inside W 40: worst err / tol {worst[40]:.3f}")
        lib.free(h)


# ----------------------------------------------------------------------------- 8. through the connector
S_TREE, S_NEXT = 40, 5
TREE_NEW = [40, 33, 17, 16, 1, 0]


@pytest.mark.parametrize("prescale", [False, True], ids=["plain", "k-pre-scale"])
@pytest.mark.parametrize("scheme", ALL)
def test_connector_tree_step_on_local_and_global_layers_commit_and_next_step(oracle, scheme, prescale):
    """attend_tree with a 40-node random tree per request, ragged n_new: layer 0 local (W = 8 and 40), layer 1 global (window=None: the
    bits of attend_chunk(parents=...)), live rows against float64 over what the kernel is given, dead rows zero; the layers' tables
    live side by side.  Then commit(nodes = the longest live path) and a second tree step over the longer requests on both layers"""
    torch = torch_mod()
    rpp = 4
    prompts, _, _ = _inputs(rpp)
    rng = np.random.default_rng(40)
    B = len(PROMPTS)
    new, q = (_rows(rng, B, S_TREE, L, H, D), _rows(rng, B, S_TREE, L, H, D)), _rows(rng, B, S_TREE, H, rpp, D)
    new2, q2 = (_rows(rng, B, S_NEXT, L, H, D), _rows(rng, B, S_NEXT, L, H, D)), _rows(rng, B, S_NEXT, H, rpp, D)
    trees, tree2 = _random_trees(41, S_TREE), [-1, 0, 0, 1, 3]
    ks = _kscale() if prescale else np.ones((L, H, D), np.float32)
    inv = 1.0 / ks
    pre = [(_f16_times(k, inv[:, None]), v) for k, v in prompts]
    new_pre, new2_pre = (_f16_times(new[0], inv[None, None]), new[1]), (_f16_times(new2[0], inv[None, None]), new2[1])
    dev = lambda x: torch.from_numpy(x).cuda()
    with _batch(torch, scheme, prompts, kscale=ks if prescale else None) as (lib, conn):
        def step(layer, qq, nn, tr, live, window, splits=1):
            got = conn.attend_tree(layer, RIDS, dev(qq), dev(nn[0]), dev(nn[1]), SM, tr, live, splits=splits, window=window)
            torch.cuda.synchronize()
            return got.cpu().numpy()

        def check(layer, qq, nn_pre, tr, live, outs, held, what):
            qs = _f16_times(qq, ks[layer][None, None, :, None, :])
            worst = {}
            for b in RIDS:
                lv, _ = _sees(tr[b], live[b], 0, 0, 0)
                for _, got, _ in outs:
                    assert not got[b, ~lv].any(), (scheme, b, "a dead row is not zero")
                if lv.any():
                    _merge(worst, _check(_stored256(oracle, scheme, b, layer), conn, b, b, held[b], qs, nn_pre, tr[b], live[b], outs, what, layer=layer))
            return worst

        local = [(w, step(0, q, new, trees, TREE_NEW, w, splits), None) for w, splits in ((8, 1), (40, 0))]
        table = conn._chunk_tree_wtabs[40]
        glob = step(1, q, new, trees, TREE_NEW, None)
        plain = conn.attend_chunk(1, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, TREE_NEW, parents=trees)
        torch.cuda.synchronize()
        assert np.array_equal(glob.view(np.uint32), plain.cpu().numpy().view(np.uint32))
        again = step(0, q, new, trees, TREE_NEW, 40, 0)
        assert conn._chunk_tree_wtabs[40] is table and np.array_equal(again.view(np.uint32), local[1][1].view(np.uint32))
        worst = check(0, q, new_pre, trees, TREE_NEW, local, pre, "connector local")
        _merge(worst, check(1, q, new_pre, trees, TREE_NEW, [(0, glob, None)], pre, "connector global"))
        print(f"attend_tree {scheme} {'pre-scaled ' if prescale else ''}local / global layers: worst err / tol {_show(worst)}")
        paths = [_longest_path(p, _sees(p, n, 0, 0, 0)[0]) for p, n in zip(trees, TREE_NEW)]
        assert len(paths[0]) > 1 and paths[-1] == []
        keep = conn.commit(RIDS, dev(new[0]), dev(new[1]), paths)
        torch.cuda.synchronize()
        assert [conn.length(b) for b in RIDS] == [p + len(path) for p, path in zip(PROMPTS, paths)]
        longer = [(np.concatenate([pre[b][0], new_pre[0][b, path].transpose(1, 0, 2, 3)], axis=1),
                   np.concatenate([pre[b][1], new_pre[1][b, path].transpose(1, 0, 2, 3)], axis=1)) for b, path in enumerate(paths)]
        after = check(0, q2, new2_pre, [tree2] * B, [S_NEXT] * B, [(8, step(0, q2, new2, tree2, None, 8), None)], longer, "second step local")
        _merge(after, check(1, q2, new2_pre, [tree2] * B, [S_NEXT] * B, [(0, step(1, q2, new2, tree2, None, 0), None)], longer, "second step global"))
        print(f"attend_tree after commit(nodes=path) {scheme}: worst err / tol {_show(after)}")
        with pytest.raises(ValueError, match="window"):
            conn.attend_chunk(0, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM, parents=tree2, window=8)
        del keep


# ----------------------------------------------------------------------------- 9. refusals at the entry
def test_the_tree_window_entry_refuses_bad_arguments_and_capture():
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    trees = _random_trees(55, S)
    with _batch(torch, "fp8", prompts) as (lib, conn):
        masks, depths = _tables(trees, N_TW, BASES, 33)
        probe = {}
        _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_TW, masks, depths, 33, keep=probe)
        d_mask, d_depth = probe["args"]["d_mask"], probe["args"]["d_depth"]
        pos_end = np.asarray([p & ~1 for p in PROMPTS], np.uint32)
        odd = pos_end.copy(); odd[3] = 35
        before = bytes(lib.stats())
        invalid = {"NULL d_mask": dict(d_mask=0), "d_mask off 4-byte alignment": dict(d_mask=d_mask + 2), "NULL d_depth": dict(d_depth=0),
                   "d_depth off 4-byte alignment": dict(d_depth=d_depth + 2), "mask_words one too small": dict(mask_words=masks.shape[2] - 1),
                   "rows_per_pos 3": dict(rows_per_pos=3), "n_q > C": dict(n_q=np.asarray([S + 1] + N_TW[1:], np.uint32)),
                   "an odd pos_end": dict(pos_end=odd), "n_splits 65": dict(n_splits=65), "NULL stream": dict(stream=0)}
        for what, change in invalid.items():
            for window in (0, 33):
                held = {}
                with pytest.raises(SpeckvError) as e:
                    _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_TW, masks, depths, window, fill=PATTERN, keep=held, **change)
                    pytest.fail(what)
                assert e.value.status == -4, (what, window, e.value.status)     # SPECKV_ERR_INVAL
                torch.cuda.synchronize()
                assert bool((held["out"] == PATTERN).all()) and bool((held["lse"] == PATTERN).all()), what
        assert bytes(lib.stats()) == before, "a refused call counted something"
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], [0] * len(RIDS), masks, depths, 33, fill=PATTERN)      # nothing to do
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)
        # capture: refused, nothing launched
        s = torch.cuda.Stream()
        held = {}
        _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_TW, masks, depths, 33, fill=PATTERN, keep=held, on=s)      # eager: fine
        torch.cuda.synchronize()
        out = held["out"]
        eager = out.clone()
        out.fill_(PATTERN)
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            with pytest.raises(SpeckvError) as e:
                lib.attend_chunk_tree_window(**held["args"])
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and not bool((eager == PATTERN).all())


# ----------------------------------------------------------------------------- 10. the example
def test_the_sliding_window_tree_example_agrees_with_its_torch_reference():
    """examples/sliding_window_tree_example.py in this process, short: a tree step over alternating local and global layers against
    torch on the device, commit of a path, the next step"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sliding_window_tree_example.py")
    spec = importlib.util.spec_from_file_location("sliding_window_tree_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run("fp8", window=24, prompt=75, steps=3, verbose=False) > 75
