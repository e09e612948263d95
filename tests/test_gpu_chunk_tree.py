"""-m gpu: chunk attention under a tree mask -- speckv_ext_attend_chunk_masked (k_attend_chunk's MASKED form: trees of drafts of any
size in one launch) and SpeckvKVConnector.attend_chunk(parents=...) on top of it.

Reference: numpy float64 softmax attention with the fp16 query as given, the oracle's records for the stored part (HeadChecker.kv), the
fp16 held rows for the rest; which new positions a node sees comes from an ancestor walk over `parents` written HERE (_tree), never from
chunk_tree_masks.  Bound: the project's own for this kernel (tests/test_gpu_chunk.py): |err| <= 2e-3 sum p|v| + 1e-6 with the sum over
the VISIBLE positions only, |lse err| <= 2e-3.

Shapes: those of tests/test_gpu_chunk.py -- L = 2, T = 256, prompts of 0, 1, 2, 37, 64 and 98 positions (with and without a tail, an
empty pool, a partial last tile), C = 70 nodes = 3 mask words, so bits 31 / 32 and 63 / 64 are crossed with base 0 and with base 1;
all three formats; rows_per_pos 1 and 8 (16 too where the chain is compared with the causal entry)."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, torch_mod
from tests.test_gpu_chunk import (L, LAYER, N_NEW, PATTERN, PROMPTS, RIDS, S, SM, T, _batch, _check64, _entry, _f32, _inputs, _kscale,
                                  _f16_times, _rows, _stored64)

pytestmark = pytest.mark.gpu
ALL = ["fp8", "int4", "mxfp4"]
W = (S + 1 + 31) // 32
BASES = [p & 1 for p in PROMPTS]
FULL = [S] * len(PROMPTS)


# ----------------------------------------------------------------------------- the test's own tree rules
def _tree(parents, n):
    """by walking up from every node: vis [S][S] (node j sees new position a: itself and its ancestors), live [S] (the node and its
    ancestors are all < n)"""
    n_nodes = len(parents)
    vis, live = np.zeros((n_nodes, n_nodes), bool), np.zeros(n_nodes, bool)
    for j in range(n_nodes):
        a, ok = j, True
        while a >= 0:
            vis[j, a] = True
            ok = ok and a < n
            a = parents[a]
        live[j] = ok
    return vis, live


def _words(vis, live, base, words=W):
    """mask rows uint32 [S][words] of one request built bit by bit: the low `base` bits and bit base + a for every visible a; dead
    rows all zero"""
    rows = np.zeros((len(vis), words), np.uint32)
    for j in range(len(vis)):
        if live[j]:
            for t in list(range(base)) + [base + int(a) for a in np.nonzero(vis[j])[0]]:
                rows[j, t >> 5] |= np.uint32(1 << (t & 31))
    return rows


def _chain_words(words=W):
    full = np.ones(S, bool)
    return np.stack([_words(np.tril(np.ones((S, S), bool)), full, base, words) for base in BASES])


def _random_parents(seed, n_nodes=S):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(-1, j)) for j in range(n_nodes)] for _ in PROMPTS]


def _entry_m(torch, lib, conn, rids, q, k_new, v_new, n_new, masks, layer=LAYER, fill=None, keep=None, **change):
    """speckv_ext_attend_chunk_masked over what the connector holds, as tests.test_gpu_chunk._entry calls the causal entry: (out, lse)
    as numpy int32 bit patterns.  masks: uint32 [B][C][words].  keep: a dict that receives the device out / lse (a refused call)."""
    B, C_, _, R, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    st = torch.cuda.Stream()
    tails = [r for r in reqs if r.length & 1]
    tail_idx, rank = [], 0
    for r in reqs:
        tail_idx.append(rank if r.length & 1 else -1)
        rank += r.length & 1
    tk = torch.stack([r.tail_k for r in tails]).contiguous() if tails else None
    tv = torch.stack([r.tail_v for r in tails]).contiguous() if tails else None
    dq, dk, dv = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (q, k_new, v_new))
    dm = torch.from_numpy(np.ascontiguousarray(masks).view(np.int32)).cuda()
    out = torch.full((B, C_, H, R, D), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    lse = torch.full((B, C_, H, R), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    if keep is not None:
        keep["out"], keep["lse"], keep["mask"] = out, lse, dm
    row = H * D
    args = dict(handles=np.asarray([r.handle for r in reqs], np.uint64), layer=layer, d_q=dq.data_ptr(), C=C_, rows_per_pos=R,
                pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), n_q=np.asarray(n_new, np.uint32),
                d_k_new=dk.data_ptr() + 2 * layer * dk.stride(2), d_v_new=dv.data_ptr() + 2 * layer * dv.stride(2), seq_stride=dk.stride(0),
                pos_stride=dk.stride(1), tail_idx=np.asarray(tail_idx, np.int32), d_k_tail=tk.data_ptr() + 2 * layer * row if tails else 0,
                d_v_tail=tv.data_ptr() + 2 * layer * row if tails else 0, tail_stride=L * row, d_mask=dm.data_ptr(), mask_words=masks.shape[2],
                sm_scale=SM, d_out=out.data_ptr(), d_lse=lse.data_ptr(), stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    lib.attend_chunk_masked(**args)
    st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _reference_tree(K, V, tail, q, kn, vn, vis):
    """float64 for the rows given: q [n][R][D] fp16, stored rows K / V [even][D], tail (k, v) or None, ALL new rows kn / vn [S][D] fp16,
    vis [n][S] = the new positions each of the n rows sees -> out [n][R][D], lse [n][R], mag = sum p|v| over what the row sees"""
    n, R, _ = q.shape
    front = len(K) + (tail is not None)
    parts_k, parts_v = [K], [V]
    if tail is not None:
        parts_k.append(tail[0][None].astype(np.float64)); parts_v.append(tail[1][None].astype(np.float64))
    Ka, Va = np.concatenate(parts_k + [kn.astype(np.float64)]), np.concatenate(parts_v + [vn.astype(np.float64)])
    seen = np.concatenate([np.ones((n, front), bool), vis], axis=1).repeat(R, axis=0)
    s = (q.astype(np.float64).reshape(n * R, D) @ Ka.T) * SM
    s[~seen] = -np.inf
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    Vs = np.where(np.isfinite(Va), Va, 0.0)
    return ((p @ Vs) / l[:, None]).reshape(n, R, D), (mx + np.log(l)).reshape(n, R), ((p @ np.abs(Vs)) / l[:, None]).reshape(n, R, D)


def _check_tree(oracle, scheme, conn, b, rid, prompt, q, new, rows, vis, out, lse, what, layer=LAYER):
    """request b's rows `rows` (indices of live nodes) against float64 under vis [S][S]; lse None: the output only.  Returns the
    worst err / tol"""
    k, v = prompt
    even, worst = k.shape[1] & ~1, 0.0
    r = conn.requests[rid]
    rows = np.asarray(rows, int)
    for head in range(H):
        K, V = _stored64(oracle, scheme, b, k, v, head, layer)
        tail = None if not r.length & 1 else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        want, wlse, mag = _reference_tree(K[:even], V[:even], tail, q[b, rows, head], new[0][b, :, layer, head], new[1][b, :, layer, head], vis[rows])
        got = _f32(out)[b, rows, head]
        assert np.all(np.isfinite(got)), (what, scheme, b, head, "not finite")
        err, tol = np.abs(got - want), 2e-3 * mag + 1e-6
        lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, rows, head] - wlse)
        worst = max(worst, float((err / tol).max()), float(lerr.max() / 2e-3))
        assert np.all(err <= tol), (what, scheme, b, head, "out", float((err / tol).max()))
        assert np.all(lerr <= 2e-3), (what, scheme, b, head, "lse", float(lerr.max()))
    return worst


# ----------------------------------------------------------------------------- (a) chain words = the causal entry
@pytest.mark.parametrize("rpp", [1, 8, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_chain_words_give_the_causal_entrys_bits(scheme, rpp):
    """row j = the low base + j + 1 bits, ragged n_q (70, 33, 17, 16, 1, 0): out and lse bit for bit those of speckv_ext_attend_chunk
    (same arithmetic, same order), rows >= n_q keep the fill pattern.  A mask applied in new-position instead of held-position
    coordinates hides position j from row j at base 1 and fails here"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        want, want_lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN)
        got, got_lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, _chain_words(), fill=PATTERN)
        assert np.array_equal(got, want) and np.array_equal(got_lse, want_lse)
        for b, n in enumerate(N_NEW):
            assert np.all(got[b, n:] == PATTERN) and np.all(got_lse[b, n:] == PATTERN), (scheme, rpp, b)
            assert not np.any(got_lse[b, :n] == PATTERN)


# ----------------------------------------------------------------------------- (b) random trees
@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("scheme", ALL)
def test_random_trees_against_float64(oracle, scheme, rpp):
    """one seeded random tree per request (parents[j] uniform in -1 .. j-1), ragged n_new, both layers: live rows against float64, dead
    rows (>= n_new or below a dead node) keep the fill pattern"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    parents = _random_parents(7)
    trees = [_tree(p, n) for p, n in zip(parents, N_NEW)]
    masks = np.asarray(SpeckvKVConnector.chunk_tree_masks(parents, BASES, N_NEW), np.uint32)
    assert np.array_equal(masks, np.stack([_words(vis, live, base) for (vis, live), base in zip(trees, BASES)]))
    with _batch(torch, scheme, prompts) as (lib, conn):
        for layer in range(L):
            out, lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, masks, layer=layer, fill=PATTERN)
            worst = 0.0
            for b, (vis, live) in enumerate(trees):
                dead = np.nonzero(~live)[0]
                assert np.all(out[b, dead] == PATTERN) and np.all(lse[b, dead] == PATTERN), (scheme, rpp, b, "a dead row was written")
                if live.any():
                    worst = max(worst, _check_tree(oracle, scheme, conn, b, b, prompts[b], q, new, np.nonzero(live)[0], vis, out, lse,
                                                   ("random trees", layer), layer=layer))
            print(f"attend_chunk_masked {scheme} rows_per_pos {rpp} random trees layer {layer}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- (c) star
@pytest.mark.parametrize("rpp", [1, 8])
@pytest.mark.parametrize("scheme", ALL)
def test_a_star_every_node_a_child_of_the_context(oracle, scheme, rpp):
    """parents = [-1] * 70: a row sees the context and itself only.  For the empty request and the one that holds a tail only, rows
    j >= 32 see nothing (or one position) in held tile 0 and nothing in the tiles between: the running state must carry a row that has
    seen nothing (m = -inf, l = 0) to its own tile.  Everything finite and within the bound"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    parents = [-1] * S
    vis, live = _tree(parents, S)
    assert live.all() and np.array_equal(vis, np.eye(S, dtype=bool))
    masks = np.asarray(SpeckvKVConnector.chunk_tree_masks(parents, BASES), np.uint32)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, fill=PATTERN)
        assert np.all(np.isfinite(_f32(out))) and np.all(np.isfinite(_f32(lse)))
        worst = max(_check_tree(oracle, scheme, conn, b, b, prompts[b], q, new, np.arange(S), vis, out, lse, "star") for b in RIDS)
        print(f"attend_chunk_masked {scheme} rows_per_pos {rpp} star: worst err / tol {worst:.3f}")
        if rpp == 1:                                    # the empty request's rows see themselves alone: out = v exactly, lse = the score
            assert np.array_equal(_f32(out)[0, :, :, 0], new[1][0, :, LAYER].astype(np.float32))


# ----------------------------------------------------------------------------- (d) hostile siblings
BRANCHES = [-1, 0, 0] + list(range(1, S - 2))            # a root and two branches from it: odd nodes 1, 3, 5 .., even nodes 2, 4, 6 ..
CHECKED = (1, 2, 29, 30, 31, 32, 33, 34, 61, 62, 63, 64, 65, 68, 69)


@pytest.mark.parametrize("scheme", ALL)
def test_hostile_siblings_are_not_seen(oracle, scheme):
    """for each checked row (on both branches, so the branches swap roles; on and beside bits 31 / 32 and 63 / 64 at base 0 and 1) the K
    rows of EVERY node invisible to it -- the other branch, and its own branch below it -- are multiplied by 200 and the V rows by
    1000 (finite fp16), the visible set keeps its N(0, 1) magnitudes, and the row goes against float64 whose sum p|v| runs over the
    visible positions only: a hostile V of ~1000 leaking with a weight of 1e-5 is ~1e-2 against a tolerance of ~2e-3"""
    torch = torch_mod()
    rpp = 8
    prompts, new, q = _inputs(rpp)
    vis, live = _tree(BRANCHES, S)
    assert live.all() and vis[69, 1::2].all() and not vis[69, 2::2].any() and vis[68, 2::2].all() and not vis[68, 1::2].any()
    masks = np.asarray(SpeckvKVConnector.chunk_tree_masks(BRANCHES, BASES), np.uint32)
    worst = 0.0
    with _batch(torch, scheme, prompts) as (lib, conn):
        for j in CHECKED:
            hidden = ~vis[j]
            k2, v2 = new[0].copy(), new[1].copy()
            k2[:, hidden] = (k2[:, hidden].astype(np.float32) * 200).astype(np.float16)
            v2[:, hidden] = (v2[:, hidden].astype(np.float32) * 1000).astype(np.float16)
            assert np.all(np.isfinite(k2)) and np.all(np.isfinite(v2)) and np.abs(v2[:, hidden].astype(np.float32)).mean() > 500
            out, lse = _entry_m(torch, lib, conn, RIDS, q, k2, v2, FULL, masks)
            for b in RIDS:
                worst = max(worst, _check_tree(oracle, scheme, conn, b, b, prompts[b], q, (k2, v2), [j], vis, out, lse, ("hostile", j)))
    print(f"attend_chunk_masked {scheme} hostile siblings: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- (e) dead rows, ignored bits
@pytest.mark.parametrize("scheme", ALL)
def test_rows_without_their_own_bit_are_not_written_and_bits_beyond_the_row_are_ignored(scheme):
    """masks built here bit by bit.  Rows (all < n_q) whose own bit base + j is clear keep the fill pattern in out and lse although
    other bits of theirs are set (a liveness rule by n_q alone fails here); every other row is written.  Then every bit at or beyond
    base + j + 1 is set in every row: the output is bit for bit the one without them"""
    torch = torch_mod()
    rpp = 8
    prompts, new, q = _inputs(rpp)
    parents = _random_parents(11)
    off = [0, 5, 30, 31, 32, 33, 62, 63, 64, 69]
    masks = np.stack([_words(*_tree(p, S), base) for p, base in zip(parents, BASES)])
    for b, base in enumerate(BASES):
        for j in off:
            masks[b, j, (base + j) >> 5] &= np.uint32(~(1 << ((base + j) & 31)) & 0xFFFFFFFF)
    on = np.asarray([j for j in range(S) if j not in off])
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, fill=PATTERN)
        assert np.all(out[:, off] == PATTERN) and np.all(lse[:, off] == PATTERN), "a row without its own bit was written"
        assert not np.any(lse[:, on] == PATTERN) and np.all(np.isfinite(_f32(out)[:, on])) and np.all(np.isfinite(_f32(lse)[:, on]))
        more = masks.copy()
        for b, base in enumerate(BASES):
            for j in range(S):
                for t in range(base + j + 1, 32 * W):
                    more[b, j, t >> 5] |= np.uint32(1 << (t & 31))
        assert not np.array_equal(more, masks)
        out2, lse2 = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, more, fill=PATTERN)
        assert np.array_equal(out2, out) and np.array_equal(lse2, lse)


# ----------------------------------------------------------------------------- (f) refusals
def test_the_masked_entry_refuses_a_bad_mask_and_launches_nothing():
    torch = torch_mod()
    prompts, new, q = _inputs(8)
    with _batch(torch, "fp8", prompts) as (lib, conn):
        masks = _chain_words()
        probe = {}
        _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, keep=probe)
        before = bytes(lib.stats())
        at = probe["mask"].data_ptr()
        for what, change in {"NULL d_mask": dict(d_mask=0), "d_mask off 4-byte alignment": dict(d_mask=at + 2),
                             "mask_words one too small": dict(mask_words=W - 1), "NULL stream": dict(stream=0),
                             "n_q > C": dict(n_q=np.asarray([S + 1] * len(RIDS), np.uint32))}.items():
            held = {}
            with pytest.raises(SpeckvError) as e:
                _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], FULL, masks, fill=PATTERN, keep=held, **change)
                pytest.fail(what)
            assert e.value.status == -4, (what, e.value.status)              # SPECKV_ERR_INVAL
            torch.cuda.synchronize()
            assert bool((held["out"] == PATTERN).all()) and bool((held["lse"] == PATTERN).all()), what
        assert bytes(lib.stats()) == before, "a refused call counted something"
        out, lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], [0] * len(RIDS), masks, fill=PATTERN)      # nothing to do
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)


# ----------------------------------------------------------------------------- (h) a row stride larger than needed
@pytest.mark.parametrize("scheme", ALL)
def test_a_row_stride_of_five_words(scheme):
    """the same bits in rows 5 words apart (3 needed for C = 70), the words behind them filled: the same result bit for bit"""
    torch = torch_mod()
    prompts, new, q = _inputs(8)
    parents = _random_parents(13)
    masks = np.stack([_words(*_tree(p, n), base) for p, n, base in zip(parents, N_NEW, BASES)])
    wide = np.full(masks.shape[:2] + (5,), 0xA5A5A5A5, np.uint32)
    wide[:, :, :W] = masks
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, masks, fill=PATTERN)
        out2, lse2 = _entry_m(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, wide, fill=PATTERN)
        assert np.array_equal(out2, out) and np.array_equal(lse2, lse)
        assert not np.all(out == PATTERN)


# ----------------------------------------------------------------------------- (g) connector
S_TREE, S_NEXT = 40, 5
TREE_NEW = [40, 33, 17, 16, 1, 0]


def _longest_path(parents, live):
    """the root-to-node chain of live nodes with the most nodes (ascending: a parent precedes its children)"""
    best = []
    for j in np.nonzero(live)[0]:
        path, a = [], int(j)
        while a >= 0:
            path.append(a)
            a = parents[a]
        if len(path) > len(best):
            best = path[::-1]
    return best


@pytest.mark.parametrize("prescale", [False, True], ids=["plain", "k-pre-scale"])
@pytest.mark.parametrize("scheme", ALL)
def test_connector_tree_step_commit_and_next_step(oracle, scheme, prescale):
    """attend_chunk(parents=...) with a 40-node random tree per request, ragged n_new, both layers: live rows against float64 over what
    the kernel is given (with the K pre-scale: the records of k / scale, k_new / scale, q x scale), dead rows zero.  Then
    commit(nodes = the longest live root-to-node path) -- lengths and tails as commit documents -- and a plain attend_chunk of 5 further
    positions against float64 over exactly the committed rows"""
    torch = torch_mod()
    rpp = 8
    prompts, _, _ = _inputs(rpp)
    rng = np.random.default_rng(40)
    B = len(PROMPTS)
    new, q = (_rows(rng, B, S_TREE, L, H, D), _rows(rng, B, S_TREE, L, H, D)), _rows(rng, B, S_TREE, H, rpp, D)
    new2, q2 = (_rows(rng, B, S_NEXT, L, H, D), _rows(rng, B, S_NEXT, L, H, D)), _rows(rng, B, S_NEXT, H, rpp, D)
    parents = _random_parents(41, S_TREE)
    trees = [_tree(p, n) for p, n in zip(parents, TREE_NEW)]
    ks = _kscale() if prescale else np.ones((L, H, D), np.float32)
    inv = 1.0 / ks
    pre = [(_f16_times(k, inv[:, None]), v) for k, v in prompts]
    new_pre, new2_pre = (_f16_times(new[0], inv[None, None]), new[1]), (_f16_times(new2[0], inv[None, None]), new2[1])
    dev = lambda x: torch.from_numpy(x).cuda()
    with _batch(torch, scheme, prompts, kscale=ks if prescale else None) as (lib, conn):
        for layer in range(L):
            qs = _f16_times(q, ks[layer][None, None, :, None, :])
            got = conn.attend_chunk(layer, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, TREE_NEW, parents=parents)
            table = conn._chunk_tree_masks
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            worst = 0.0
            for b, (vis, live) in enumerate(trees):
                assert not got[b, ~live].any(), (scheme, b, "a dead row is not zero")
                if live.any():
                    worst = max(worst, _check_tree(oracle, scheme, conn, b, b, pre[b], qs, new_pre, np.nonzero(live)[0], vis, got, None,
                                                   ("connector tree", layer), layer=layer))
            print(f"attend_chunk(parents) {scheme} {'pre-scaled ' if prescale else ''}layer {layer}: worst err / tol {worst:.3f}")
        assert conn._chunk_tree_masks is table                              # the layers share one table
        paths = [_longest_path(p, live) for p, (_, live) in zip(parents, trees)]
        assert len(paths[0]) > 1 and paths[-1] == []
        keep = conn.commit(RIDS, dev(new[0]), dev(new[1]), paths)
        torch.cuda.synchronize()
        assert [conn.length(b) for b in RIDS] == [p + len(path) for p, path in zip(PROMPTS, paths)]
        for b, path in enumerate(paths):
            r, total = conn.requests[b], PROMPTS[b] + len(path)
            assert (r.tail_k is not None) == bool(total & 1)
            if total & 1 and path:                                          # the odd last position is the path's last node, as stored
                assert np.array_equal(r.tail_k.cpu().numpy(), new_pre[0][b, path[-1]]) and np.array_equal(r.tail_v.cpu().numpy(), new[1][b, path[-1]])
        longer = [(np.concatenate([pre[b][0], new_pre[0][b, path].transpose(1, 0, 2, 3)], axis=1),
                   np.concatenate([pre[b][1], new_pre[1][b, path].transpose(1, 0, 2, 3)], axis=1)) for b, path in enumerate(paths)]
        for layer in range(L):
            qs = _f16_times(q2, ks[layer][None, None, :, None, :])
            got = conn.attend_chunk(layer, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            worst = max(_check64(oracle, scheme, conn, b, b, longer[b], qs, new2_pre, S_NEXT, got, None, ("after the path", layer), layer=layer)
                        for b in RIDS)
            print(f"attend_chunk after commit(nodes=path) {scheme} layer {layer}: worst err / tol {worst:.3f}")
        del keep
