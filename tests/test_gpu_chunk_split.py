"""-m gpu: chunk attention with the stored positions split across the chip -- speckv_ext_attend_chunk_split (k_attend_chunk's SPLIT
form + k_chunk_combine), speckv_ext_chunk_split_plan and SpeckvKVConnector.attend_chunk(splits=...) on top of them.

Reference and bound are those of tests/test_gpu_chunk.py and tests/test_gpu_chunk_tree.py, unchanged: numpy float64 softmax attention
with the fp16 query as given, the oracle's records (HeadChecker.kv) for the stored part, the fp16 held rows for the rest;
|err| <= 2e-3 sum p|v| + 1e-6 and |lse err| <= 2e-3.  The merge is fp32 and the bound takes no allowance for it.

Shapes: L = 2, T = 512, 8 x 128 heads, all three formats.  Prompts of 0, 1, 2, 37, 98, 255 and 481 positions: no pool; a tail only; one
page; 2 pool tiles, the last partial, plus a tail; 4 tiles, the last partial; 8 tiles, the last partial, plus a tail; 15 whole tiles plus
a tail.  The step is S = 70 new positions with 70, 33, 17, 16, 1, 0 and 20 of them live."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, torch_mod
from tests.test_gpu_chunk import PATTERN, SM, _f16_times, _f32, _kscale, _reference, _rows
from tests.test_gpu_chunk_tree import BRANCHES, _longest_path, _reference_tree, _tree, _words
from tests.test_gpu_spec_step import SCHEMES, _region

pytestmark = pytest.mark.gpu
ALL = ["fp8", "int4", "mxfp4"]
L, T, S = 2, 512, 70
LAYER = 1
PROMPTS = [0, 1, 2, 37, 98, 255, 481]
N_NEW = [70, 33, 17, 16, 1, 0, 20]
RIDS = list(range(len(PROMPTS)))
BASES = [p & 1 for p in PROMPTS]
FULL = [S] * len(PROMPTS)
W = (S + 1 + 31) // 32
LONG = 6                                            # the request of 481 positions: 15 pool tiles, forced 5 = 5 pieces of 3 tiles

_data, _kv64 = {}, {}


def _inputs(rpp):
    """the batch's prompts, new rows and query rows: the same for every scheme and every test"""
    if "prompts" not in _data:
        rng = np.random.default_rng(2025)
        _data["prompts"] = [(_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in PROMPTS]
        _data["new"] = (_rows(rng, len(PROMPTS), S, L, H, D), _rows(rng, len(PROMPTS), S, L, H, D))
    if ("q", rpp) not in _data:
        _data[("q", rpp)] = _rows(np.random.default_rng(177 + rpp), len(PROMPTS), S, H, rpp, D)
    return _data["prompts"], _data["new"], _data[("q", rpp)]


def _stored64(oracle, scheme, k, v, head, layer=LAYER, t=T):
    """float64 K and V rows of the even part of a prompt's layer, kv head `head`, as the oracle's records hold them (once per prompt)"""
    key = (scheme, layer, t, k.shape[1], float(np.abs(k[layer].astype(np.float32)).sum()), float(np.abs(v[layer].astype(np.float32)).sum()))
    if key not in _kv64:
        even = k.shape[1] & ~1
        _kv64[key] = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], t), t)
    return _kv64[key].kv(head)


@contextlib.contextmanager
def _batch(torch, scheme, prompts, rids=None, kscale=None, t=T):
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, t, scheme)
        if kscale is not None:
            conn.set_k_channel_scale(torch.from_numpy(kscale).cuda())
        keep = []
        for rid, (k, v) in zip(rids if rids is not None else range(len(prompts)), prompts):
            conn.add_request(rid)
            if k.shape[1]:
                keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
        del keep
    finally:
        lib.finalize()


def _stage(torch, conn, rids, q, k_new, v_new, n_new, n_splits, masks=None, layer=LAYER, fill=None, entry="split", on=None, **change):
    """the arguments of one of the three chunk entries over what the connector holds, inputs and pre-filled outputs on the device (the
    caller synchronises before it issues the call): (entry, args, out, lse, stream, what must stay alive).  entry: "split"
    (speckv_ext_attend_chunk_split; masks None = the causal form), "causal" or "masked" (the two existing entries)"""
    B, C_, _, R, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    st = on if on is not None else torch.cuda.Stream()
    tails = [r for r in reqs if r.length & 1]
    tail_idx, rank = [], 0
    for r in reqs:
        tail_idx.append(rank if r.length & 1 else -1)
        rank += r.length & 1
    tk = torch.stack([r.tail_k for r in tails]).contiguous() if tails else None
    tv = torch.stack([r.tail_v for r in tails]).contiguous() if tails else None
    dq, dk, dv = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (q, k_new, v_new))
    dm = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks).view(np.int32)).cuda()
    out = torch.full((B, C_, H, R, D), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    lse = torch.full((B, C_, H, R), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    row = H * D
    args = dict(handles=np.asarray([r.handle for r in reqs], np.uint64), layer=layer, d_q=dq.data_ptr(), C=C_, rows_per_pos=R,
                pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), n_q=np.asarray(n_new, np.uint32),
                d_k_new=dk.data_ptr() + 2 * layer * dk.stride(2), d_v_new=dv.data_ptr() + 2 * layer * dv.stride(2), seq_stride=dk.stride(0),
                pos_stride=dk.stride(1), tail_idx=np.asarray(tail_idx, np.int32), d_k_tail=tk.data_ptr() + 2 * layer * row if tails else 0,
                d_v_tail=tv.data_ptr() + 2 * layer * row if tails else 0, tail_stride=L * row, sm_scale=SM, d_out=out.data_ptr(),
                d_lse=lse.data_ptr(), stream=st.cuda_stream)
    if entry != "causal":
        args.update(d_mask=0 if dm is None else dm.data_ptr(), mask_words=0 if masks is None else masks.shape[2])
    if entry == "split":
        args.update(n_splits=n_splits)
    args.update(change)
    return entry, args, out, lse, st, (dq, dk, dv, dm, tk, tv, out, lse)


def _issue(lib, staged):
    """the staged call, not waited for: (out, lse, stream, what must stay alive)"""
    entry, args, out, lse, st, held = staged
    try:
        {"split": lib.attend_chunk_split, "causal": lib.attend_chunk, "masked": lib.attend_chunk_masked}[entry](**args)
    except SpeckvError as e:
        e.held = held
        raise
    return out, lse, st, held


def _launch(torch, lib, conn, rids, q, k_new, v_new, n_new, n_splits, masks=None, **kw):
    staged = _stage(torch, conn, rids, q, k_new, v_new, n_new, n_splits, masks, **kw)
    torch.cuda.synchronize()
    return _issue(lib, staged)


def _entry(torch, lib, conn, rids, q, k_new, v_new, n_new, n_splits, masks=None, **kw):
    """_launch, waited for: (out, lse) as numpy int32 bit patterns, [B][S][H][R][D] and [B][S][H][R]"""
    out, lse, st, held = _launch(torch, lib, conn, rids, q, k_new, v_new, n_new, n_splits, masks, **kw)
    st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _check(oracle, scheme, conn, b, rid, prompt, q, new, rows, vis, out, lse, what, layer=LAYER, t=T, other=None):
    """request b's rows `rows` (an int n: the first n, causal; indices with vis [S][S]: the tree reference) against float64 under the
    project's bound; lse None: the output only.  other: a second output of the same rows (another piece count) -- both are within
    tol of float64, so they are within 2 tol of each other, which is asserted too.  Returns the worst err / tol"""
    k, v = prompt
    even, worst = k.shape[1] & ~1, 0.0
    r = conn.requests[rid]
    rows = np.arange(rows) if np.isscalar(rows) else np.asarray(rows, int)
    for head in range(H):
        K, V = _stored64(oracle, scheme, k, v, head, layer, t)
        tail = None if not r.length & 1 else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        if vis is None:
            n = len(rows)
            want, wlse, mag = _reference(K[:even], V[:even], tail, q[b, :n, head], new[0][b, :n, layer, head], new[1][b, :n, layer, head])
        else:
            want, wlse, mag = _reference_tree(K[:even], V[:even], tail, q[b, rows, head], new[0][b, :, layer, head], new[1][b, :, layer, head],
                                              vis[rows])
        got = _f32(out)[b, rows, head]
        assert np.all(np.isfinite(got)), (what, scheme, b, head, "not finite")
        err, tol = np.abs(got - want), 2e-3 * mag + 1e-6
        lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, rows, head] - wlse)
        worst = max(worst, float((err / tol).max()), float(lerr.max() / 2e-3))
        assert np.all(err <= tol), (what, scheme, b, head, "out", float((err / tol).max()))
        assert np.all(lerr <= 2e-3), (what, scheme, b, head, "lse", float(lerr.max()))
        if other is not None:
            assert np.all(np.abs(got - _f32(other)[b, rows, head]) <= 2 * tol), (what, scheme, b, head, "against the other piece count")
    return worst


def _parents(seed, n_nodes=S, n_req=len(PROMPTS)):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(-1, j)) for j in range(n_nodes)] for _ in range(n_req)]


def _chain_words():
    full = np.ones(S, bool)
    return np.stack([_words(np.tril(np.ones((S, S), bool)), full, base, W) for base in BASES])


def _plan(lib, conn, rids, n_new, rpp, n_splits):
    return lib.chunk_split_plan([conn.requests[r].length & ~1 for r in rids], n_new, rpp, n_splits)


# ----------------------------------------------------------------------------- 1. forced counts, causal
@pytest.mark.parametrize("rpp", [1, 8, 16])
@pytest.mark.parametrize("n_splits", [2, 3, 5, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_forced_pieces_against_float64(oracle, scheme, n_splits, rpp):
    """the ragged batch at both layers: 3 and 5 do not divide the tile counts (2, 4, 8, 15), 16 exceeds every pool and is clamped, the
    requests of 0 and 1 pool tiles keep one piece beside split ones, one request is dead"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        pieces, tpp = _plan(lib, conn, RIDS, N_NEW, rpp, n_splits)
        # pool tiles 0, 0, 1, 2, 4, 8, 15: min(N, tiles) pieces, evened out (4 tiles in 3 = 2 x 2; 8 in 5 = 4 x 2; 15 in 16 = 15 x 1)
        assert pieces == {2: [1, 1, 1, 2, 2, 2, 2], 3: [1, 1, 1, 2, 2, 3, 3], 5: [1, 1, 1, 2, 4, 4, 5], 16: [1, 1, 1, 2, 4, 8, 15]}[n_splits]
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, n_splits, layer=layer, fill=PATTERN)
            worst = max(_check(oracle, scheme, conn, b, b, prompts[b], q, new, N_NEW[b], None, out, lse, ("forced", n_splits, layer), layer=layer)
                        for b in RIDS if N_NEW[b])
            print(f"attend_chunk_split {scheme} forced {n_splits} pieces {pieces} rows_per_pos {rpp} layer {layer}: worst err / tol {worst:.3f}")
            for b, n in enumerate(N_NEW):
                assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, b)


# ----------------------------------------------------------------------------- 2. forced counts under masks
@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("n_splits", [3, 5])
@pytest.mark.parametrize("scheme", ALL)
def test_forced_pieces_under_random_trees_and_a_star(oracle, scheme, n_splits, rpp):
    """one seeded random tree per request with ragged n_new at both layers, then a star (every node a child of the context: rows that
    see nothing of the held tiles but themselves): live rows against the tree reference, dead rows keep the fill pattern"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    parents = _parents(7)
    trees = [_tree(p, n) for p, n in zip(parents, N_NEW)]
    masks = np.stack([_words(vis, live, base, W) for (vis, live), base in zip(trees, BASES)])
    assert np.array_equal(masks, np.asarray(SpeckvKVConnector.chunk_tree_masks(parents, BASES, N_NEW), np.uint32))
    star_vis, star_live = _tree([-1] * S, S)
    star = np.stack([_words(star_vis, star_live, base, W) for base in BASES])
    with _batch(torch, scheme, prompts) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, n_splits, masks, layer=layer, fill=PATTERN)
            worst = 0.0
            for b, (vis, live) in enumerate(trees):
                dead = np.nonzero(~live)[0]
                assert np.all(out[b, dead] == PATTERN) and np.all(lse[b, dead] == PATTERN), (scheme, rpp, b, "a dead row was written")
                if live.any():
                    worst = max(worst, _check(oracle, scheme, conn, b, b, prompts[b], q, new, np.nonzero(live)[0], vis, out, lse,
                                              ("random trees", n_splits, layer), layer=layer))
            print(f"attend_chunk_split {scheme} forced {n_splits} rows_per_pos {rpp} random trees layer {layer}: worst err / tol {worst:.3f}")
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], FULL, n_splits, star, fill=PATTERN)
        assert np.all(np.isfinite(_f32(out))) and np.all(np.isfinite(_f32(lse)))
        worst = max(_check(oracle, scheme, conn, b, b, prompts[b], q, new, np.arange(S), star_vis, out, lse, ("star", n_splits)) for b in RIDS)
        print(f"attend_chunk_split {scheme} forced {n_splits} rows_per_pos {rpp} star: worst err / tol {worst:.3f}")


HOSTILE_ROWS = (1, 2, 31, 32, 33, 64, 65, 68, 69)


@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("n_splits", [3, 5])
@pytest.mark.parametrize("scheme", ALL)
def test_forced_pieces_do_not_see_hostile_siblings(oracle, scheme, n_splits, rpp):
    """the tree suite's two branches: for each checked row the K rows of every node invisible to it are x 200 and the V rows x 1000,
    and the row goes against float64 whose sum p|v| runs over the visible positions only"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    vis, live = _tree(BRANCHES, S)
    masks = np.asarray(SpeckvKVConnector.chunk_tree_masks(BRANCHES, BASES), np.uint32)
    worst = 0.0
    with _batch(torch, scheme, prompts) as (lib, conn):
        for j in HOSTILE_ROWS:
            hidden = ~vis[j]
            k2, v2 = new[0].copy(), new[1].copy()
            k2[:, hidden] = (k2[:, hidden].astype(np.float32) * 200).astype(np.float16)
            v2[:, hidden] = (v2[:, hidden].astype(np.float32) * 1000).astype(np.float16)
            assert np.all(np.isfinite(k2)) and np.all(np.isfinite(v2))
            out, lse = _entry(torch, lib, conn, RIDS, q, k2, v2, FULL, n_splits, masks)
            for b in RIDS:
                worst = max(worst, _check(oracle, scheme, conn, b, b, prompts[b], q, (k2, v2), [j], vis, out, lse, ("hostile", j)))
    print(f"attend_chunk_split {scheme} forced {n_splits} rows_per_pos {rpp} hostile siblings: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- 3. one piece = the existing entries' bits
@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("scheme", ALL)
def test_one_piece_gives_the_existing_entries_bits(scheme, rpp):
    """n_splits = 1 is speckv_ext_attend_chunk's launch (no mask) and speckv_ext_attend_chunk_masked's (chain words, a tree mask): out
    and lse bit for bit.  Every pool here is under the rule's floor of 32 tiles, so n_splits = 0 plans one piece and gives them too"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    parents = _parents(17)
    tree = np.stack([_words(*_tree(p, n), base, W) for p, n, base in zip(parents, N_NEW, BASES)])
    with _batch(torch, scheme, prompts) as (lib, conn):
        assert _plan(lib, conn, RIDS, N_NEW, rpp, 0)[0] == [1] * len(RIDS)
        want = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, None, entry="causal", fill=PATTERN)
        assert not np.all(want[0] == PATTERN)
        for n_splits in (1, 0):
            got = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, n_splits, fill=PATTERN)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scheme, rpp, n_splits, "causal")
        for what, masks in (("chain", _chain_words()), ("tree", tree)):
            want = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, None, masks, entry="masked", fill=PATTERN)
            for n_splits in (1, 0):
                got = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, n_splits, masks, fill=PATTERN)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scheme, rpp, n_splits, what)


# ----------------------------------------------------------------------------- 4. a forced count: batch-independent, deterministic
@pytest.mark.parametrize("scheme", ALL)
def test_a_forced_count_gives_the_same_bits_alone_and_in_any_batch(scheme):
    """request 481 alone, and inside the batch in two orders, at forced 5 (causal and under a tree): bit-equal rows; the same call
    twice gives equal bits"""
    torch = torch_mod()
    rpp = 8
    prompts, new, q = _inputs(rpp)
    parents = _parents(23)
    tree = np.stack([_words(*_tree(p, n), base, W) for p, n, base in zip(parents, N_NEW, BASES)])
    n = N_NEW[LONG]
    with _batch(torch, scheme, prompts) as (lib, conn):
        for masks in (None, tree):
            pick = lambda order: None if masks is None else masks[order]
            alone = _entry(torch, lib, conn, [LONG], q[[LONG]], new[0][[LONG]], new[1][[LONG]], [n], 5, pick([LONG]))
            for order in (RIDS, [3, LONG, 5, 0, 4, 2, 1]):
                o = np.asarray(order)
                args = (torch, lib, conn, order, q[o], new[0][o], new[1][o], [N_NEW[b] for b in order], 5, pick(o))
                out, lse = _entry(*args)
                at = order.index(LONG)
                assert np.array_equal(out[at, :n], alone[0][0, :n]) and np.array_equal(lse[at, :n], alone[1][0, :n]), (scheme, order)
                again = _entry(*args)
                assert np.array_equal(again[0], out) and np.array_equal(again[1], lse), (scheme, "not deterministic")


# ----------------------------------------------------------------------------- 5. dead rows
@pytest.mark.parametrize("scheme", ALL)
def test_nothing_is_written_for_dead_rows(scheme):
    """out / lse pre-filled with a pattern, forced 5.  Causal: the pattern survives in rows j >= n_q (the all-dead request included)
    and nowhere else.  Masked: also in rows < n_q whose own bit is clear.  Every live value is finite"""
    torch = torch_mod()
    rpp = 8
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, 5, fill=PATTERN)
        for b, n in enumerate(N_NEW):
            assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, b)
            assert np.all(np.isfinite(_f32(out)[b, :n])) and np.all(np.isfinite(_f32(lse)[b, :n])) and not np.any(lse[b, :n] == PATTERN)
            assert not np.any(np.all(out[b, :n] == PATTERN, axis=-1))
        parents = _parents(11)
        off = [0, 5, 31, 32, 33, 63, 64, 69]
        masks = np.stack([_words(*_tree(p, S), base, W) for p, base in zip(parents, BASES)])
        for b, base in enumerate(BASES):
            for j in off:
                masks[b, j, (base + j) >> 5] &= np.uint32(~(1 << ((base + j) & 31)) & 0xFFFFFFFF)
        n_q = [S, S, 40, S, S, 0, S]
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], n_q, 5, masks, fill=PATTERN)
        for b, n in enumerate(n_q):
            dead = np.asarray([j for j in range(S) if j >= n or j in off], int)
            on = np.asarray([j for j in range(S) if j < n and j not in off], int)
            assert np.all(out[b, dead] == PATTERN) and np.all(lse[b, dead] == PATTERN), (scheme, b, "a dead row was written")
            assert not np.any(lse[b, on] == PATTERN) and np.all(np.isfinite(_f32(out)[b, on])) and np.all(np.isfinite(_f32(lse)[b, on]))


# ----------------------------------------------------------------------------- 6. a needle in every piece
J, HEAD, SUB, VCONST, CNEEDLE = 15, 5, 2, 6.0, 2.0
NEEDLE_AT = {"piece-0": 50, "piece-1": 150, "piece-2": 250, "piece-3": 350, "piece-4": 450, "held": None}


def _merge(m, l, acc, mutation=None, dropped=None):
    """k_chunk_combine in numpy (float64, log2 domain): partials m [P], l [P], acc [P][D] of one row -> (out [D], lse).  mutation:
    "drop" leaves piece `dropped` out, "no-rescale" adds the partials without their weights, "wrong-max" weighs piece p by its
    neighbour's maximum (an index slip)"""
    P = len(m)
    use = [p for p in range(P) if not (mutation == "drop" and p == dropped)]
    M = max(m[p] for p in use)
    w = {p: 1.0 if mutation == "no-rescale" else np.exp2((m[(p + 1) % P] if mutation == "wrong-max" else m[p]) - M) for p in use}
    lsum = sum(l[p] * w[p] for p in use)
    return sum(acc[p] * w[p] for p in use) / lsum, (M + np.log2(lsum)) * np.log(2.0)


@pytest.mark.parametrize("where", list(NEEDLE_AT))
@pytest.mark.parametrize("scheme", ALL)
def test_a_needle_in_every_piece(oracle, scheme, where):
    """request 481 at forced 5: pieces of 3 tiles = stored positions [96 p, 96 p + 96).  One stored key 2 x the query row (J, HEAD, SUB)
    with a V row of 6.0 inside piece p (or at new position 3, in the held part) takes nearly all of that row's weight: every row goes
    against float64, and the aligned row is the needle's V row.  The merge restated in numpy over float64 partials of the same pieces
    reproduces the reference; with the needle's piece dropped (each piece is the needle's in one case), the rescale skipped or the
    maximum taken from the wrong piece it misses the bound for the aligned row -- so this test fails on each of those mistakes"""
    torch = torch_mod()
    rng = np.random.default_rng(4343)
    n = PROMPTS[LONG]
    k, v = _rows(rng, L, n, H, D), _rows(rng, L, n, H, D)
    kn, vn, q = _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, H, 4, D)
    needle = (np.float32(CNEEDLE) * q[0, J, HEAD, SUB].astype(np.float32)).astype(np.float16)
    if NEEDLE_AT[where] is None:
        kn[0, 3, LAYER, HEAD], vn[0, 3, LAYER, HEAD] = needle, np.float16(VCONST)
    else:
        k[LAYER, NEEDLE_AT[where], HEAD], v[LAYER, NEEDLE_AT[where], HEAD] = needle, np.float16(VCONST)
    with _batch(torch, scheme, [(k, v)]) as (lib, conn):
        assert _plan(lib, conn, [0], [S], 4, 5) == ([5], [3])
        out, lse = _entry(torch, lib, conn, [0], q, kn, vn, [S], 5)
        worst = _check(oracle, scheme, conn, 0, 0, (k, v), q, (kn, vn), S, None, out, lse, ("needle", where))
        print(f"attend_chunk_split {scheme} forced 5 needle {where}: worst err / tol {worst:.3f}")
        assert np.all(np.abs(_f32(out)[0, J, HEAD, SUB] - VCONST) < 1e-2), (scheme, where, _f32(out)[0, J, HEAD, SUB, :4])
        # the merge and its three mutations over float64 partials of the aligned row
        K, V = _stored64(oracle, scheme, k, v, HEAD)
        r = conn.requests[0]
        Ka = np.concatenate([K[:n - 1], r.tail_k[LAYER, HEAD].cpu().numpy()[None].astype(np.float64), kn[0, :J + 1, LAYER, HEAD].astype(np.float64)])
        Va = np.concatenate([V[:n - 1], r.tail_v[LAYER, HEAD].cpu().numpy()[None].astype(np.float64), vn[0, :J + 1, LAYER, HEAD].astype(np.float64)])
        s2 = (Ka @ q[0, J, HEAD, SUB].astype(np.float64)) * SM * np.log2(np.e)
        bounds = [(96 * p, 96 * p + 96) for p in range(4)] + [(384, len(Ka))]
        m = [s2[a:b].max() for a, b in bounds]
        l = [np.exp2(s2[a:b] - mp).sum() for (a, b), mp in zip(bounds, m)]
        acc = [np.exp2(s2[a:b] - mp) @ Va[a:b] for (a, b), mp in zip(bounds, m)]
        want, wlse, mag = _reference(K[:n - 1], V[:n - 1], (r.tail_k[LAYER, HEAD].cpu().numpy(), r.tail_v[LAYER, HEAD].cpu().numpy()),
                                     q[0, :J + 1, HEAD], kn[0, :J + 1, LAYER, HEAD], vn[0, :J + 1, LAYER, HEAD])
        want, wlse, tol = want[J, SUB], wlse[J, SUB], 2e-3 * mag[J, SUB] + 1e-6
        o, ls = _merge(m, l, acc)
        assert np.all(np.abs(o - want) <= 1e-9) and abs(ls - wlse) <= 1e-9
        needle_piece = list(NEEDLE_AT).index(where) if NEEDLE_AT[where] is not None else 4
        for mutation in ("drop", "no-rescale", "wrong-max"):
            o, ls = _merge(m, l, acc, mutation, needle_piece)
            missed = bool(np.any(np.abs(o - want) > tol)) or not abs(ls - wlse) <= 2e-3
            assert missed, (scheme, where, mutation, "the bound would not catch this merge")


# ----------------------------------------------------------------------------- 7. stale records behind a cut
@pytest.mark.parametrize("scheme", ALL)
def test_stale_records_behind_a_cut_are_not_seen_by_any_piece(oracle, scheme):
    """481 positions whose rows from 300 on are 1000 x larger, truncated to 300: 10 pool tiles, the last one partial (12 positions) with
    hostile records behind the cut in the same tile and in five more; forced 5 = pieces of 2 tiles"""
    torch = torch_mod()
    rpp = 8
    _, new, q = _inputs(rpp)
    rng = np.random.default_rng(19)
    k, v = _rows(rng, L, 481, H, D), _rows(rng, L, 481, H, D)
    k[:, 300:] *= np.float16(1000); v[:, 300:] *= np.float16(1000)
    with _batch(torch, scheme, [(k, v)]) as (lib, conn):
        conn.truncate([0], [300])
        torch.cuda.synchronize()
        assert conn.length(0) == 300 and _plan(lib, conn, [0], [S], rpp, 5) == ([5], [2])
        out, lse = _entry(torch, lib, conn, [0], q[:1], new[0][:1], new[1][:1], [S], 5)
        worst = _check(oracle, scheme, conn, 0, 0, (k[:, :300], v[:, :300]), q, new, S, None, out, lse, "behind a cut")
        print(f"attend_chunk_split {scheme} forced 5 behind a cut: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- 8. the rule itself splitting
T_LONG, N_LONG, S_SHORT = 4096, 4001, 5


@pytest.mark.parametrize("scheme", ALL)
def test_the_rule_splits_a_short_step_over_a_long_context(oracle, scheme):
    """one request of 4001 positions (125 pool tiles and a tail), a 5-node tree and a 5-position chain at rows_per_pos 8, n_splits = 0:
    the plan reports more than one piece -- the test cannot pass on the unsplit path -- and the rows go against float64"""
    torch = torch_mod()
    rpp = 8
    rng = np.random.default_rng(4001)
    k, v = _rows(rng, L, N_LONG, H, D), _rows(rng, L, N_LONG, H, D)
    new, q = (_rows(rng, 1, S_SHORT, L, H, D), _rows(rng, 1, S_SHORT, L, H, D)), _rows(rng, 1, S_SHORT, H, rpp, D)
    parents = [-1, 0, 0, 1, 2]
    vis, live = _tree(parents, S_SHORT)
    masks = _words(vis, live, 1, 1)[None]
    with _batch(torch, scheme, [(k, v)], t=T_LONG) as (lib, conn):
        pieces, tpp = _plan(lib, conn, [0], [S_SHORT], rpp, 0)
        assert pieces[0] > 1 and pieces[0] * tpp[0] >= 125 > (pieces[0] - 1) * tpp[0], (pieces, tpp)
        out, lse = _entry(torch, lib, conn, [0], q, new[0], new[1], [S_SHORT], 0, fill=PATTERN)
        worst = _check(oracle, scheme, conn, 0, 0, (k, v), q, new, S_SHORT, None, out, lse, "rule, chain", t=T_LONG)
        out, lse = _entry(torch, lib, conn, [0], q, new[0], new[1], [S_SHORT], 0, masks, fill=PATTERN)
        worst_tree = _check(oracle, scheme, conn, 0, 0, (k, v), q, new, np.arange(S_SHORT), vis, out, lse, "rule, tree", t=T_LONG)
        print(f"attend_chunk_split {scheme} rule: {pieces[0]} pieces of {tpp[0]} tiles; chain worst err / tol {worst:.3f}, tree {worst_tree:.3f}")


# ----------------------------------------------------------------------------- 9. through the connector
S_TREE, S_NEXT = 40, 5
TREE_NEW = [40, 33, 17, 16, 1, 0, 20]


@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("scheme", ALL)
def test_connector_splits_with_and_without_parents(oracle, scheme, splits):
    """attend_chunk(splits=...) of a connector with a K pre-scale, as a chain and with a 40-node random tree per request: against float64
    over what the kernel is given and against splits=1 within the bound; lengths unchanged.  Then commit(nodes = the longest live path)
    and a second step of 5 positions at the new (odd and even) lengths, again against float64 and against splits=1"""
    torch = torch_mod()
    rpp = 8
    prompts, _, _ = _inputs(rpp)
    rng = np.random.default_rng(41)
    B = len(PROMPTS)
    new, q = (_rows(rng, B, S_TREE, L, H, D), _rows(rng, B, S_TREE, L, H, D)), _rows(rng, B, S_TREE, H, rpp, D)
    new2, q2 = (_rows(rng, B, S_NEXT, L, H, D), _rows(rng, B, S_NEXT, L, H, D)), _rows(rng, B, S_NEXT, H, rpp, D)
    parents = _parents(43, S_TREE)
    trees = [_tree(p, n) for p, n in zip(parents, TREE_NEW)]
    ks = _kscale()
    inv = 1.0 / ks
    pre = [(_f16_times(k, inv[:, None]), v) for k, v in prompts]
    new_pre, new2_pre = (_f16_times(new[0], inv[None, None]), new[1]), (_f16_times(new2[0], inv[None, None]), new2[1])
    dev = lambda x: torch.from_numpy(x).cuda()

    with _batch(torch, scheme, prompts, kscale=ks) as (lib, conn):
        lengths = [conn.length(r) for r in RIDS]
        for layer in range(L):
            qs = _f16_times(q, ks[layer][None, None, :, None, :])
            for with_parents in (False, True):
                kw = dict(parents=parents) if with_parents else {}
                got = conn.attend_chunk(layer, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, TREE_NEW, splits=splits, **kw)
                base = conn.attend_chunk(layer, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, TREE_NEW, splits=1, **kw)
                torch.cuda.synchronize()
                got, base = got.cpu().numpy(), base.cpu().numpy()
                worst = 0.0
                for b, (vis, live) in enumerate(trees):
                    rows = np.nonzero(live)[0] if with_parents else np.arange(TREE_NEW[b])
                    dead = np.setdiff1d(np.arange(S_TREE), rows)
                    assert not got[b, dead].any(), (scheme, b, "a dead row is not zero")
                    if len(rows):
                        worst = max(worst, _check(oracle, scheme, conn, b, b, pre[b], qs, new_pre, rows if with_parents else len(rows),
                                                  vis if with_parents else None, got, None, ("connector", splits, with_parents, layer), layer=layer,
                                                  other=base))
                    assert np.array_equal(got[b, dead], base[b, dead])
                print(f"attend_chunk(splits={splits}{', parents' if with_parents else ''}) {scheme} layer {layer}: worst err / tol {worst:.3f}")
        assert [conn.length(r) for r in RIDS] == lengths                  # the attention calls change no state
        paths = [_longest_path(p, live) for p, (_, live) in zip(parents, trees)]
        keep = conn.commit(RIDS, dev(new[0]), dev(new[1]), paths)
        torch.cuda.synchronize()
        assert [conn.length(b) for b in RIDS] == [p + len(path) for p, path in zip(PROMPTS, paths)]
        longer = [(np.concatenate([pre[b][0], new_pre[0][b, path].transpose(1, 0, 2, 3)], axis=1),
                   np.concatenate([pre[b][1], new_pre[1][b, path].transpose(1, 0, 2, 3)], axis=1)) for b, path in enumerate(paths)]
        for layer in range(L):
            qs = _f16_times(q2, ks[layer][None, None, :, None, :])
            got = conn.attend_chunk(layer, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM, splits=splits)
            base = conn.attend_chunk(layer, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM)
            torch.cuda.synchronize()
            got, base = got.cpu().numpy(), base.cpu().numpy()
            worst = max(_check(oracle, scheme, conn, b, b, longer[b], qs, new2_pre, S_NEXT, None, got, None, ("after the path", layer), layer=layer,
                               other=base) for b in RIDS)
            print(f"attend_chunk(splits={splits}) after commit(nodes=path) {scheme} layer {layer}: worst err / tol {worst:.3f}")
        del keep


# ----------------------------------------------------------------------------- 10. refusals
def test_the_split_entry_refuses_what_the_other_two_refuse_and_launches_nothing():
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, "fp8", prompts) as (lib, conn):
        lib.set_compression_scheme(1)
        int8 = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(int8, T, L, H, D, 2)
        lib.set_compression_scheme(3)
        int4 = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(int4, T, L, H, D, 2)
        lib.set_compression_scheme(4)
        narrow = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(narrow, 2 * T, L, 4, D, 2)
        handles = np.asarray([conn.requests[r].handle for r in RIDS], np.uint64)
        with_handle = lambda b, h: np.concatenate([handles[:b], [np.uint64(h)], handles[b + 1:]])
        pos_end = np.asarray([p & ~1 for p in PROMPTS], np.uint32)
        with_pos = lambda b, p: np.concatenate([pos_end[:b], [np.uint32(p)], pos_end[b + 1:]])
        masks = _chain_words()
        probe = _launch(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, 5, masks)
        probe[2].synchronize()
        at = probe[3][3].data_ptr()
        before = bytes(lib.stats())
        invalid = {
            "n_splits 65": dict(n_splits=65), "n_splits 2^32 - 1": dict(n_splits=0xFFFFFFFF),
            "NULL stream": dict(stream=0), "NULL q": dict(d_q=0), "NULL out": dict(d_out=0), "NULL k_new": dict(d_k_new=0),
            "an odd pos_end": dict(pos_end=with_pos(3, 35)), "pos_end beyond the layout": dict(pos_end=with_pos(5, T + 2)),
            "n_q > C": dict(n_q=np.asarray([S + 1] + N_NEW[1:], np.uint32)),
            "rows_per_pos 3": dict(rows_per_pos=3), "rows_per_pos 0": dict(rows_per_pos=0), "rows_per_pos 32": dict(rows_per_pos=32),
            "a position stride that is no multiple of 8": dict(pos_stride=L * H * D + 4),
            "a sequence stride that is no multiple of 8": dict(seq_stride=S * L * H * D + 2),
            "a position stride shorter than a row": dict(pos_stride=H * D - 8),
            "a tail stride shorter than a row": dict(tail_stride=H * D - 8),
            "tails without rows": dict(d_k_tail=0),
            "a misaligned q": dict(d_q=0x1008),
            "another scheme among them": dict(handles=with_handle(2, int4)), "a scheme without a fused form": dict(handles=with_handle(2, int8)),
            "a layout of 4 heads": dict(handles=with_handle(2, narrow)), "a layer beyond the layout": dict(layer=L),
        }
        masked_only = {"mask_words one too small": dict(mask_words=W - 1), "d_mask off 4-byte alignment": dict(d_mask=at + 2)}
        for n_splits in (5, 0, 1):
            for use_mask in (False, True):
                cases = dict(invalid, **masked_only) if use_mask else invalid
                for what, change in cases.items():
                    change = dict(change)
                    count = change.pop("n_splits", n_splits)
                    with pytest.raises(SpeckvError) as e:
                        _launch(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, count, masks if use_mask else None, fill=PATTERN, **change)
                        pytest.fail(what)
                    assert e.value.status == -4, (what, n_splits, use_mask, e.value.status)             # SPECKV_ERR_INVAL
                    torch.cuda.synchronize()
                    assert bool((e.value.held[6] == PATTERN).all()) and bool((e.value.held[7] == PATTERN).all()), what
        with pytest.raises(SpeckvError) as e:
            _launch(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, 5, fill=PATTERN, handles=with_handle(1, 0xDEAD))
        assert e.value.status == -1                                          # SPECKV_ERR_GENERAL: an unknown handle
        torch.cuda.synchronize()
        assert bool((e.value.held[6] == PATTERN).all())
        assert bytes(lib.stats()) == before, "a refused call counted something"
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], [0] * len(RIDS), 5, fill=PATTERN)      # nothing to do
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)


# ----------------------------------------------------------------------------- 11. the scratch buffer across streams
@pytest.mark.parametrize("scheme", ALL)
def test_two_split_calls_on_two_streams_without_a_wait_between_them(oracle, scheme):
    """a split call on stream A (request 481 alone, 3 pieces), then a LARGER one on stream B (the batch, 16 forced: the scratch buffer
    grows) with no synchronisation between the two: both results are the ones each call gives alone, and within the float64 bound --
    the second call is ordered behind the first on the buffer they share"""
    torch = torch_mod()
    rpp = 8
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        one = ([LONG], q[[LONG]], new[0][[LONG]], new[1][[LONG]], [S], 3)
        two = (RIDS, q, new[0], new[1], FULL, 16)
        want_a = _entry(torch, lib, conn, *one)
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        sa, sb = _stage(torch, conn, *one, on=a), _stage(torch, conn, *two, on=b)
        torch.cuda.synchronize()
        ra = _issue(lib, sa)
        rb = _issue(lib, sb)                                    # nothing waits between the two calls
        a.synchronize(); b.synchronize()
        got_a = (ra[0].cpu().numpy(), ra[1].cpu().numpy())
        got_b = (rb[0].cpu().numpy(), rb[1].cpu().numpy())
        want_b = _entry(torch, lib, conn, *two)
        assert np.array_equal(got_a[0], want_a[0]) and np.array_equal(got_a[1], want_a[1]), scheme
        assert np.array_equal(got_b[0], want_b[0]) and np.array_equal(got_b[1], want_b[1]), scheme
        worst = max(_check(oracle, scheme, conn, bb, bb, prompts[bb], q, new, S, None, got_b[0], got_b[1], "two streams") for bb in RIDS)
        print(f"attend_chunk_split {scheme} two streams: worst err / tol {worst:.3f}")
