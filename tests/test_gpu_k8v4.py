"""-m gpu: the split pool ("K8V4") -- speckv_ext_attend_chunk_kv (K pages of an FP8_E4M3 allocation, V pages of an MXFP4 allocation, one
chunk-attention launch) and SpeckvSplitKVConnector on top of it.

Reference: numpy float64 softmax attention as tests/test_gpu_chunk.py::_reference computes it, with the fp16 query as given; the stored K
rows are HeadChecker(oracle, FP8).kv(head)[0] -- the oracle's FP8 records of the prompt's K -- and the stored V rows
HeadChecker(oracle, MXFP4).kv(head)[1] over the same prompt; the held rows are fp16.  Bound: the project's, |err| <= 2e-3 sum p|v| + 1e-6,
|lse err| <= 2e-3.  Geometry of tests/test_gpu_chunk.py: L = 2, T = 256, prompts of 0, 1, 2, 37, 64, 98 positions, S = 70 new positions
with 70, 33, 17, 16, 1, 0 of them live."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
L, T, S = 2, 256, 70
LAYER = 1
PROMPTS = [0, 1, 2, 37, 64, 98]
N_NEW = [70, 33, 17, 16, 1, 0]
RIDS = list(range(len(PROMPTS)))
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19
FP8, MX4 = 4, 5

_data, _kv64 = {}, {}


def _rows(rng, *shape):
    return rng.standard_normal(shape).astype(np.float16)


def _inputs(rpp):
    """the batch's prompts, new rows and query rows: the same for every test"""
    if "prompts" not in _data:
        rng = np.random.default_rng(2026)
        _data["prompts"] = [(_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in PROMPTS]
        _data["new"] = (_rows(rng, len(PROMPTS), S, L, H, D), _rows(rng, len(PROMPTS), S, L, H, D))
    if ("q", rpp) not in _data:
        _data[("q", rpp)] = _rows(np.random.default_rng(91 + rpp), len(PROMPTS), S, H, rpp, D)
    return _data["prompts"], _data["new"], _data[("q", rpp)]


def _stored64(oracle, tag, k, v, head, layer):
    """float64 (K rows as the FP8 records hold them, V rows as the MXFP4 records hold them) of the even part of a prompt's layer, kv
    head `head`; computed once per (tag, layer)"""
    key = (tag, layer)
    if key not in _kv64:
        even = k.shape[1] & ~1
        region = _region(k[layer, :even], v[layer, :even], T)
        _kv64[key] = (HeadChecker(oracle, FP8, region, T), HeadChecker(oracle, MX4, region, T))
    k8, v4 = _kv64[key]
    return k8.kv(head)[0], v4.kv(head)[1]


@contextlib.contextmanager
def _batch(torch, prompts, rids=None):
    """a split connector whose requests hold the prompts"""
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
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


def _prepare(torch, conn, rids, q, k_new, v_new, n_new, layer=LAYER, fill=None, on=None, **change):
    """the arguments of speckv_ext_attend_chunk_kv over what the connector holds -> (args, out, lse, stream, what the launch reads).
    fill: the 32-bit pattern out and lse hold before the call.  change: arguments to replace."""
    B, C_, _, R, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    st = on if on is not None else torch.cuda.Stream()                     # (`stream` among the changes: the raw argument)
    tails = [r for r in reqs if r.length & 1]
    tail_idx, rank = [], 0
    for r in reqs:
        tail_idx.append(rank if r.length & 1 else -1)
        rank += r.length & 1
    tk = torch.stack([r.tail_k for r in tails]).contiguous() if tails else None          # [n][L][H][D]
    tv = torch.stack([r.tail_v for r in tails]).contiguous() if tails else None
    dq, dk, dv = (t if hasattr(t, "data_ptr") else torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (q, k_new, v_new))
    out = torch.full((B, C_, H, R, D), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    lse = torch.full((B, C_, H, R), 0 if fill is None else fill, dtype=torch.int32, device="cuda")
    row = H * D
    args = dict(k_handles=np.asarray([r.k_handle for r in reqs], np.uint64), v_handles=np.asarray([r.v_handle for r in reqs], np.uint64),
                layer=layer, d_q=dq.data_ptr(), C=C_, rows_per_pos=R, pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32),
                n_q=np.asarray(n_new, np.uint32), d_k_new=dk.data_ptr() + 2 * layer * dk.stride(2), d_v_new=dv.data_ptr() + 2 * layer * dv.stride(2),
                seq_stride=dk.stride(0), pos_stride=dk.stride(1), tail_idx=np.asarray(tail_idx, np.int32),
                d_k_tail=tk.data_ptr() + 2 * layer * row if tails else 0, d_v_tail=tv.data_ptr() + 2 * layer * row if tails else 0,
                tail_stride=L * row, d_mask=0, mask_words=0, d_depth=0, window=0, n_splits=1, sm_scale=SM, d_out=out.data_ptr(),
                d_lse=lse.data_ptr(), stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    return args, out, lse, st, (dq, dk, dv, tk, tv)


def _entry(torch, lib, conn, rids, q, k_new, v_new, n_new, **how):
    """speckv_ext_attend_chunk_kv itself: (out, lse) as numpy, [B][S][H][R][D] and [B][S][H][R]"""
    args, out, lse, st, held = _prepare(torch, conn, rids, q, k_new, v_new, n_new, **how)
    lib.attend_chunk_kv(**args)
    st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _f32(x):
    return x.view(np.float32)


def _visible(n_stored, base, n, window=None, parents=None):
    """bool [n][n_stored + base + n]: what new position (node) j sees of the stored positions, the tail and the new positions.  Causal
    chain by default; window W: the absolute positions [max(0, P + 1 - W), P], P = n_stored + base + j (a tree: + depth(j), on its root
    path); parents: a node sees what the request holds, its ancestors and itself"""
    total = n_stored + base + n
    vis = np.zeros((n, total), bool)
    depth = []
    for j in range(n):
        if parents is None:
            path, d = list(range(j + 1)), j
        else:
            path, a = [], j
            while a >= 0:
                path.append(a)
                a = parents[a]
            d = len(path) - 1
        depth.append(d)
        lo = 0 if not window else max(0, n_stored + base + d + 1 - window)
        vis[j, lo:n_stored + base] = True
        for a in path:
            da = a if parents is None else depth[a]
            if n_stored + base + da >= lo:
                vis[j, n_stored + base + a] = True
    return vis


def _reference(K, V, tail, q, kn, vn, vis=None):
    """float64, as tests/test_gpu_chunk.py::_reference: q [n][R][D] fp16 as given, stored rows K / V [even][D], tail (k [D], v [D]) fp16
    or None, new rows kn / vn [n][D] fp16, vis [n][all positions] (None: causal) -> out [n][R][D], lse [n][R], mag [n][R][D] = sum p|v|"""
    n, R, _ = q.shape
    parts_k, parts_v = [K], [V]
    if tail is not None:
        parts_k.append(tail[0][None].astype(np.float64)); parts_v.append(tail[1][None].astype(np.float64))
    Ka, Va = np.concatenate(parts_k + [kn.astype(np.float64)]), np.concatenate(parts_v + [vn.astype(np.float64)])
    s = (q.astype(np.float64).reshape(n * R, D) @ Ka.T) * SM
    if vis is None:
        vis = _visible(len(K), int(tail is not None), n)
    s[~np.repeat(vis, R, axis=0)] = -np.inf
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return ((p @ Va) / l[:, None]).reshape(n, R, D), (mx + np.log(l)).reshape(n, R), ((p @ np.abs(Va)) / l[:, None]).reshape(n, R, D)


def _check64(oracle, tag, conn, b, rid, prompt, q, new, n, out, lse, what, layer=LAYER, window=None, parents=None, live=None):
    """rows of request b's first n new positions (live: which of them, default all) against float64 at `layer`; lse None: the output
    only.  Returns the worst err / tol"""
    k, v = prompt
    even, worst = k.shape[1] & ~1, 0.0
    r = conn.requests[rid]
    base = r.length & 1
    vis = _visible(even, base, n, window, parents)
    rows = np.arange(n) if live is None else np.asarray(live)
    for head in range(H):
        K, V = _stored64(oracle, tag, k, v, head, layer)
        tail = None if not base else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        want, wlse, mag = _reference(K[:even], V[:even], tail, q[b, :n, head], new[0][b, :n, layer, head], new[1][b, :n, layer, head], vis)
        err, tol = np.abs(_f32(out)[b, :n, head] - want)[rows], (2e-3 * mag + 1e-6)[rows]
        lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, :n, head] - wlse)[rows]
        worst = max(worst, float((err / tol).max()), float(lerr.max() / 2e-3))
        assert np.all(err <= tol), (what, b, head, "out", float((err / tol).max()))
        assert np.all(lerr <= 2e-3), (what, b, head, "lse", float(lerr.max()))
    return worst


# ----------------------------------------------------------------------------- the entry over the ragged batch
@pytest.mark.parametrize("rpp", [1, 4, 16])
def test_attend_chunk_kv_against_float64(oracle, rpp):
    """both layers of the ragged batch; rows that are not live keep the fill pattern; SpeckvSplitKVConnector.attend_chunk gives the
    entry's bits (zeros for the rows that are not live) with one library call"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, prompts) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, layer=layer, fill=PATTERN)
            worst = max(_check64(oracle, ("batch", b), conn, b, b, prompts[b], q, new, N_NEW[b], out, lse, ("batch", layer), layer=layer)
                        for b in RIDS if N_NEW[b])
            print(f"attend_chunk_kv rows_per_pos {rpp} layer {layer}: worst err / tol {worst:.3f}")
            for b, n in enumerate(N_NEW):
                assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (layer, b, "a dead row was written")
        calls, real = [], lib.attend_chunk_kv
        lib.attend_chunk_kv = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        got = conn.attend_chunk(LAYER, RIDS, torch.from_numpy(q).cuda(), torch.from_numpy(new[0]).cuda(), torch.from_numpy(new[1]).cuda(), SM, N_NEW)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert len(calls) == 1 and [conn.length(r) for r in RIDS] == PROMPTS
        for b, n in enumerate(N_NEW):
            assert np.array_equal(got[b, :n].view(np.uint32), out[b, :n].view(np.uint32)), (rpp, b)
            assert not got[b, n:].any()


def test_translate_reports_the_scheme_of_either_allocation():
    torch = torch_mod()
    prompts, _, _ = _inputs(4)
    with _batch(torch, prompts) as (lib, conn):
        r = conn.requests[5]                                               # 98 positions: pages 0..48 of either layer's region
        for layer in range(L):
            for page in (0, 17, 48):
                at = (layer * (T // 2) + page) * 4096
                ki, vi = lib.translate(r.k_handle, at), lib.translate(r.v_handle, at)
                assert (ki.scheme, ki.rec_bytes) == (FP8, 2048), (layer, page, ki.scheme, ki.rec_bytes)
                assert (vi.scheme, vi.rec_bytes) == (MX4, 1088), (layer, page, vi.scheme, vi.rec_bytes)
            at = (layer * (T // 2) + 49) * 4096                            # never written
            assert lib.translate(r.k_handle, at).rec_bytes == 0 and lib.translate(r.v_handle, at).rec_bytes == 0


# ----------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("n_splits", [2, 3, 5, 0])
def test_stored_positions_split_across_the_chip(oracle, n_splits):
    """a 200-position prompt (7 pool tiles, the last partial) and one with a tail, 17 and 70 new positions: forced pieces and the
    library's rule against float64"""
    torch = torch_mod()
    _, new, q = _inputs(4)
    if "split" not in _data:
        rng = np.random.default_rng(200)
        _data["split"] = [(_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in (200, 131)]
    prompts, n_new = _data["split"], [17, 70]
    with _batch(torch, prompts) as (lib, conn):
        pieces, _ = lib.chunk_split_plan([200, 130], n_new, 4, n_splits)
        if n_splits:                                                       # min(N, tiles) pieces, then no piece empty (chunk_split.hpp)
            even = lambda tiles: -(-tiles // -(-tiles // min(n_splits, tiles)))
            assert pieces == [even(7), even(5)] and min(pieces) > 1
        else:
            assert pieces == [1, 1]                                        # the rule cuts no piece under 32 tiles: the unsplit launch
        out, lse = _entry(torch, lib, conn, [0, 1], q[:2], new[0][:2], new[1][:2], n_new, fill=PATTERN, n_splits=n_splits)
        worst = max(_check64(oracle, ("split", b), conn, b, b, prompts[b], q, new, n_new[b], out, lse, ("pieces", n_splits)) for b in (0, 1))
        print(f"attend_chunk_kv n_splits {n_splits} (pieces {pieces}): worst err / tol {worst:.3f}")
        assert np.all(out[0, 17:] == PATTERN) and np.all(lse[0, 17:] == PATTERN)


# ----------------------------------------------------------------------------- windows and trees
@pytest.mark.parametrize("window", [1, 33, 100])
def test_sliding_windows(oracle, window):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN, window=window)
        worst = max(_check64(oracle, ("batch", b), conn, b, b, prompts[b], q, new, N_NEW[b], out, lse, ("window", window), window=window)
                    for b in RIDS if N_NEW[b])
        print(f"attend_chunk_kv window {window}: worst err / tol {worst:.3f}")
        got = conn.attend_chunk(LAYER, RIDS, torch.from_numpy(q).cuda(), torch.from_numpy(new[0]).cuda(), torch.from_numpy(new[1]).cuda(), SM, N_NEW,
                                window=window)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for b, n in enumerate(N_NEW):
            assert np.array_equal(got[b, :n].view(np.uint32), out[b, :n].view(np.uint32)) and not got[b, n:].any(), (window, b)


N_TREE = 33


def _tree():
    rng = np.random.default_rng(3301)
    return [-1] + [int(rng.integers(-1, j)) for j in range(1, N_TREE)]


@pytest.mark.parametrize("window", [None, 33])
def test_a_random_tree_of_33_nodes(oracle, window):
    """the same random tree under every request of the ragged batch (all 33 nodes live, but 20 for the request of 37 positions: the
    nodes behind them and below them are dead and not written), alone and under a window that goes by depth; through the entry with
    the tables of SpeckvKVConnector.chunk_tree_masks / chunk_tree_depths, and through the connector"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    parents = _tree()
    live_n = [N_TREE, N_TREE, N_TREE, 20, N_TREE, N_TREE]
    qt, kt, vt = q[:, :N_TREE], np.ascontiguousarray(new[0][:, :N_TREE]), np.ascontiguousarray(new[1][:, :N_TREE])
    assert max(SpeckvKVConnector.chunk_tree_depths(parents)[0]) >= 3
    with _batch(torch, prompts) as (lib, conn):
        base = [p & 1 for p in PROMPTS]
        rows = SpeckvKVConnector.chunk_tree_masks(parents, base, live_n, window=window)
        masks = torch.from_numpy(np.asarray(rows, np.uint32).view(np.int32)).cuda()
        depths = torch.from_numpy(np.asarray(SpeckvKVConnector.chunk_tree_depths(parents, len(RIDS)), np.uint32).view(np.int32)).cuda()
        out, lse = _entry(torch, lib, conn, RIDS, qt, kt, vt, live_n, fill=PATTERN, d_mask=masks.data_ptr(), mask_words=masks.shape[2],
                          d_depth=depths.data_ptr() if window else 0, window=window or 0)
        worst = 0.0
        for b in RIDS:
            alive = [j for j in range(N_TREE) if any(rows[b][j])]
            dead = [j for j in range(N_TREE) if j not in alive]
            assert (b == 3) == bool(dead)
            worst = max(worst, _check64(oracle, ("batch", b), conn, b, b, prompts[b], qt, (kt, vt), N_TREE, out, lse, ("tree", window), window=window,
                                        parents=parents, live=alive))
            assert np.all(out[b, dead] == PATTERN) and np.all(lse[b, dead] == PATTERN), b
        print(f"attend_chunk_kv tree of {N_TREE} nodes, window {window}: worst err / tol {worst:.3f}")
        got = conn.attend_chunk(LAYER, RIDS, torch.from_numpy(qt).cuda(), torch.from_numpy(kt).cuda(), torch.from_numpy(vt).cuda(), SM, live_n,
                                window=window, parents=parents)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for b in RIDS:
            alive = [j for j in range(N_TREE) if any(rows[b][j])]
            assert np.array_equal(got[b, alive].view(np.uint32), out[b, alive].view(np.uint32)), (window, b)


# ----------------------------------------------------------------------------- a key that takes nearly all the weight
J, HEAD, SUB, VCONST = 40, 5, 2, 6.0


@pytest.mark.parametrize("where,pos", [("stored", 31), ("stored", 97), ("new", 33)])
def test_a_key_that_takes_nearly_all_the_weight(oracle, where, pos):
    """a key 2 x the query row (J, HEAD, SUB) with a V row of 6.0 in a pool tile / in a held tile: about 22 natural units above the
    N(0, 1) rest.  The bound's argument (fp32 accumulation of exact fp16 products costs a score < 1e-4 while sum |q k| sm < 64) is
    asserted for the inputs; the aligned row's output is the needle's V row as the MXFP4 record (stored) or the fp16 row (held) has it"""
    torch = torch_mod()
    rng = np.random.default_rng(4242)
    k, v = _rows(rng, L, 98, H, D), _rows(rng, L, 98, H, D)
    kn, vn, q = _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, H, 4, D)
    needle = (np.float32(2.0) * q[0, J, HEAD, SUB].astype(np.float32)).astype(np.float16)
    if where == "stored":
        k[LAYER, pos, HEAD], v[LAYER, pos, HEAD] = needle, np.float16(VCONST)
    else:
        kn[0, pos, LAYER, HEAD], vn[0, pos, LAYER, HEAD] = needle, np.float16(VCONST)
    with _batch(torch, [(k, v)]) as (lib, conn):
        reach = 0.0
        for head in range(H):
            K, _ = _stored64(oracle, ("needle", where, pos), k, v, head, LAYER)
            keys = np.concatenate([np.abs(K[:98]), np.abs(kn[0, :, LAYER, head].astype(np.float64))])
            reach = max(reach, float((np.abs(q[0, :, head].astype(np.float64)).reshape(-1, D) @ keys.T).max()) * SM)
        assert reach < 64.0, ("the inputs left the reach of the bound's argument", reach)
        out, lse = _entry(torch, lib, conn, [0], q, kn, vn, [S])
        worst = _check64(oracle, ("needle", where, pos), conn, 0, 0, (k, v), q, (kn, vn), S, out, lse, ("needle", where, pos))
        print(f"attend_chunk_kv needle {where} {pos}: worst err / tol {worst:.3f} (sum |q k| sm <= {reach:.1f})")
        assert np.all(np.abs(_f32(out)[0, J, HEAD, SUB] - VCONST) < 1e-2), _f32(out)[0, J, HEAD, SUB, :4]


# ----------------------------------------------------------------------------- pages never written
@pytest.mark.parametrize("layer", [0, 1])
def test_pages_never_written_count_as_zeros(oracle, layer):
    """the two allocations written through speckv_write except K page 5, V page 9 and the whole second tile (pages 16..31 of both) of
    pos_end = 64: a never-written K row scores 0, a never-written V row adds nothing"""
    torch = torch_mod()
    _, new, q = _inputs(4)
    rng = np.random.default_rng(70 + layer)
    k, v = _rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D)
    k[:, 2 * 5:2 * 5 + 2] = 0; v[:, 2 * 9:2 * 9 + 2] = 0
    k[:, 32:] = 0; v[:, 32:] = 0
    with _batch(torch, []) as (lib, conn):
        hk, hv = conn.add_request(0)
        page = lambda x, first, n: np.ascontiguousarray(x[layer, 2 * first:2 * (first + n)]).reshape(n, 2 * H * D)
        for x, h, skip in ((k, hk, 5), (v, hv, 9)):
            for first, n in ((0, skip), (skip + 1, 16 - skip - 1)):
                img = page(x, first, n)
                lib.write(h, (layer * (T // 2) + first) * 4096, img.ctypes.data, img.nbytes, False)
        lib.sync()
        conn.requests[0].length = 64
        n = 33
        out, lse = _entry(torch, lib, conn, [0], q[:1], new[0][:1], new[1][:1], [n], layer=layer, fill=PATTERN)
        assert np.all(np.isfinite(_f32(out)[0, :n])) and np.all(np.isfinite(_f32(lse)[0, :n]))
        assert np.all(out[0, n:] == PATTERN) and np.all(lse[0, n:] == PATTERN)
        worst = _check64(oracle, ("never", layer), conn, 0, 0, (k, v), q, new, n, out, lse, ("never written", layer), layer=layer)
        print(f"attend_chunk_kv never-written pages layer {layer}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, prompts) as (lib, conn):
        size = T * L * H * D * 2

        def alloc(scheme, tokens=T, layers=L // 2, heads=H, nbytes=size):
            lib.set_compression_scheme(scheme)
            h = lib.alloc(nbytes)
            lib.set_layout(h, tokens, layers, heads, D, 2)
            return h
        v_fp8, k_mx4, int4 = alloc(FP8), alloc(MX4), alloc(3)
        narrow = alloc(FP8, 2 * T, L // 2, 4)
        half_v = alloc(MX4, T // 2, L)                                   # the same pages, num_tokens differs from the K allocation's
        one_k, one_v = alloc(FP8, T, 1, H, size // 2), alloc(MX4, T, 1, H, size // 2)          # the layout's two regions, the pages of one
        kh = np.asarray([conn.requests[r].k_handle for r in RIDS], np.uint64)
        vh = np.asarray([conn.requests[r].v_handle for r in RIDS], np.uint64)
        with_h = lambda hs, b, h: np.concatenate([hs[:b], [np.uint64(h)], hs[b + 1:]])
        pos_end = np.asarray([p & ~1 for p in PROMPTS], np.uint32)
        with_pos = lambda b, p: np.concatenate([pos_end[:b], [np.uint32(p)], pos_end[b + 1:]])
        rows = SpeckvKVConnector.chunk_tree_masks(list(range(-1, S - 1)), [p & 1 for p in PROMPTS], N_NEW)
        masks = torch.from_numpy(np.asarray(rows, np.uint32).view(np.int32)).cuda()
        mask = dict(d_mask=masks.data_ptr(), mask_words=masks.shape[2])
        def refused(**change):
            """the status of the refused call; out and lse keep the fill pattern"""
            args, out, lse, st, held = _prepare(torch, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN, **change)
            with pytest.raises(SpeckvError) as e:
                lib.attend_chunk_kv(**args)
            st.synchronize(); torch.cuda.synchronize()
            assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all()), (change.keys(), "a refused call wrote something")
            return e.value.status
        before = bytes(lib.stats())
        invalid = {
            # what the chunk entries refuse
            "NULL stream": dict(stream=0), "NULL q": dict(d_q=0), "NULL out": dict(d_out=0), "NULL k_new": dict(d_k_new=0),
            "an odd pos_end": dict(pos_end=with_pos(3, 35)), "pos_end beyond the layout": dict(pos_end=with_pos(5, T + 2)),
            "n_q > C": dict(n_q=np.asarray([S + 1] + N_NEW[1:], np.uint32)),
            "rows_per_pos 3": dict(rows_per_pos=3), "rows_per_pos 0": dict(rows_per_pos=0), "rows_per_pos 32": dict(rows_per_pos=32),
            "a position stride that is no multiple of 8": dict(pos_stride=L * H * D + 4),
            "a position stride shorter than a row": dict(pos_stride=H * D - 8),
            "a tail stride shorter than a row": dict(tail_stride=H * D - 8), "tails without rows": dict(d_k_tail=0),
            "a misaligned q": dict(d_q=0x1008), "n_splits beyond the most": dict(n_splits=65),
            "a misaligned mask": dict(d_mask=masks.data_ptr() + 2, mask_words=masks.shape[2]), "too few mask words": dict(d_mask=masks.data_ptr(), mask_words=2),
            "a mask under a window without depths": dict(window=33, **mask),
            # the split pool's own
            "NULL k_handles": dict(k_handles=None), "NULL v_handles": dict(v_handles=None),
            "swapped handle arrays": dict(k_handles=vh, v_handles=kh),
            "a V allocation of FP8": dict(v_handles=with_h(vh, 2, v_fp8)), "a K allocation of MXFP4": dict(k_handles=with_h(kh, 2, k_mx4)),
            "a K allocation of INT4": dict(k_handles=with_h(kh, 2, int4)), "a V allocation of INT4": dict(v_handles=with_h(vh, 2, int4)),
            "a layout of 4 heads": dict(k_handles=with_h(kh, 2, narrow)),
            "unequal num_tokens": dict(v_handles=with_h(vh, 2, half_v)),
            "a layer beyond the layout": dict(layer=L),
            "a region beyond the K allocation's pages": dict(k_handles=with_h(kh, 0, one_k), layer=1),
            "a region beyond the V allocation's pages": dict(v_handles=with_h(vh, 0, one_v), layer=1),
        }
        for what, change in invalid.items():
            assert refused(**change) == -4, what                             # SPECKV_ERR_INVAL
        for change in (dict(k_handles=with_h(kh, 1, 0xDEAD)), dict(v_handles=with_h(vh, 1, 0xDEAD))):
            assert refused(**change) == -1                                   # SPECKV_ERR_GENERAL: an unknown handle
        assert bytes(lib.stats()) == before, "a refused call counted something"
        # nothing to do: no launch, nothing written
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN, n_q=np.zeros(len(RIDS), np.uint32))
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)


def test_a_capturing_stream_is_refused():
    """the valid call on a stream that is being captured (tests/_gpu.graph_capture): SPECKV_ERR_INVAL, out and lse keep the fill pattern;
    the capture is abandoned, and the same arguments are taken once the stream captures no more"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, prompts) as (lib, conn):
        st = torch.cuda.Stream()
        args, out, lse, _, held = _prepare(torch, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN, on=st)
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            with pytest.raises(SpeckvError) as e:
                lib.attend_chunk_kv(**args)
            assert e.value.status == -4
            bump.add_(1)
        del g
        torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all())
        # and the same arguments are taken once the stream captures no more
        lib.attend_chunk_kv(**args)
        st.synchronize()
        assert not bool((out[0] == PATTERN).any()) and not bool((lse[0] == PATTERN).any())


# ----------------------------------------------------------------------------- a walk through the connector
def test_a_walk_through_the_connector(oracle):
    """prefill 37, a chunk of 33 positions + commit, six single-position steps + commit (one of them accepts nothing): every step's rows
    against a float64 shadow that keeps the rows -- stored K through the oracle's FP8 records, stored V through its MXFP4 records, the
    tail as fp16 -- and the library calls counted: one attention call per attend_chunk, two write calls per commit"""
    torch = torch_mod()
    rng = np.random.default_rng(515)
    rpp = 4
    k0, v0 = _rows(rng, L, 37, H, D), _rows(rng, L, 37, H, D)
    with _batch(torch, [(k0, v0)], rids=[9]) as (lib, conn):
        counts = {"attend_chunk_kv": 0, "write_pairs": 0}
        for name in counts:
            real = getattr(lib, name)
            setattr(lib, name, (lambda real, name: lambda *a, **k: (counts.__setitem__(name, counts[name] + 1), real(*a, **k))[1])(real, name))
        shadow_k, shadow_v = k0.copy(), v0.copy()                          # [L][n][H][D]: every committed row
        steps = [(33, 33)] + [(1, a) for a in (1, 1, 0, 1, 1, 1)]
        keep = []
        for i, (n, accept) in enumerate(steps):
            kn, vn, q = _rows(rng, 1, n, L, H, D), _rows(rng, 1, n, L, H, D), _rows(rng, L, 1, n, H, rpp, D)
            dk, dv = torch.from_numpy(kn).cuda(), torch.from_numpy(vn).cuda()
            before = dict(counts)
            outs = [conn.attend_chunk(layer, [9], torch.from_numpy(q[layer]).cuda(), dk, dv, SM) for layer in range(L)]
            torch.cuda.synchronize()
            assert counts["attend_chunk_kv"] == before["attend_chunk_kv"] + L and counts["write_pairs"] == before["write_pairs"]
            length = shadow_k.shape[1]
            assert conn.length(9) == length
            for layer in range(L):
                worst = _check64(oracle, ("walk", i), conn, 0, 9, (shadow_k, shadow_v), q[layer], (kn, vn), n, outs[layer].cpu().numpy(), None,
                                 ("walk", i, layer), layer=layer)
                print(f"walk step {i} (length {length}, {n} new, accepts {accept}) layer {layer}: worst err / tol {worst:.3f}")
            keep += conn.commit([9], dk, dv, [accept])
            # two write calls per commit that stores a pair (a commit that only moves the tail, or accepts nothing, writes nothing)
            pairs = ((length & 1) + accept) // 2
            assert counts["write_pairs"] == before["write_pairs"] + (2 if pairs else 0), (i, counts)
            shadow_k = np.concatenate([shadow_k, kn[0, :accept].transpose(1, 0, 2, 3)], axis=1)
            shadow_v = np.concatenate([shadow_v, vn[0, :accept].transpose(1, 0, 2, 3)], axis=1)
            assert conn.length(9) == shadow_k.shape[1]
            r = conn.requests[9]
            if r.length & 1:
                torch.cuda.synchronize()
                assert np.array_equal(r.tail_k.cpu().numpy(), shadow_k[:, -1]) and np.array_equal(r.tail_v.cpu().numpy(), shadow_v[:, -1])
        assert conn.length(9) == 37 + 33 + 5
        # what the pool holds in the end is what the oracle's records of the shadow's rows decode to, page for page
        torch.cuda.synchronize()
        even = conn.length(9) & ~1
        for handle, rows, scheme in ((conn.requests[9].k_handle, shadow_k, FP8), (conn.requests[9].v_handle, shadow_v, MX4)):
            for layer in range(L):
                got = torch.empty((even // 2, 2048), dtype=torch.float16, device="cuda")
                lib.fetch_range(handle, layer * (T // 2), even // 2, got.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                blocks = np.ascontiguousarray(rows[layer, :even]).reshape(even // 2, 2048)
                scales, lens, recs = oracle.compress_blocks_f16(blocks, scheme, 0)
                want = oracle.decompress_blocks_f16(recs, lens, scales, scheme, 0)
                assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16)), (scheme, layer)
        del keep


# ----------------------------------------------------------------------------- two streams
def test_two_calls_on_two_streams(oracle):
    """the two layers of the ragged batch issued back to back on two streams, neither waited for in between: both within the bound, and
    bit for bit what each gives alone"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, prompts) as (lib, conn):
        alone = [_entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, layer=layer) for layer in range(L)]
        dq, dk, dv = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (q, new[0], new[1]))
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        runs = [_prepare(torch, conn, RIDS, dq, dk, dv, N_NEW, layer=layer, on=streams[layer]) for layer in range(L)]
        for args, *_ in runs:
            lib.attend_chunk_kv(**args)
        for s in streams:
            s.synchronize()
        for layer, (_, out, lse, _, held) in enumerate(runs):
            out, lse = out.cpu().numpy(), lse.cpu().numpy()
            for b, n in enumerate(N_NEW):
                assert np.array_equal(out[b, :n], alone[layer][0][b, :n]) and np.array_equal(lse[b, :n], alone[layer][1][b, :n]), (layer, b)
            worst = max(_check64(oracle, ("batch", b), conn, b, b, prompts[b], q, new, N_NEW[b], out, lse, ("streams", layer), layer=layer)
                        for b in RIDS if N_NEW[b])
            print(f"attend_chunk_kv two streams layer {layer}: worst err / tol {worst:.3f}")
