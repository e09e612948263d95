"""-m gpu: chunk attention -- speckv_ext_attend_chunk (one launch: causal attention of a chunk of new positions per request over stored
and held positions, any chunk length) and SpeckvKVConnector.attend_chunk on top of it.

Reference: numpy float64 softmax attention with the fp16 query AS GIVEN (this entry does not quantise it), HeadChecker.kv rows -- the
oracle's records of the prompt -- for the stored part, the fp16 held rows for the rest, causal.  Bound: the project's own bound of its
fp16-query path, HeadChecker.check with delta = 0: |err| <= 2e-3 sum p|v| + 1e-6, |lse err| <= 2e-3.

L = 2, T = 256, 8 x 128 heads; the batch holds prompts of 0, 1, 2, 37, 64 and 98 positions (no pool and no tail, a tail only, one page,
a partial last tile with a tail, whole tiles, three tiles and a partial one) and takes S = 70 new positions with 70, 33, 17, 16, 1 and 0
of them live: 1 to 3 held tiles, 1 to 18 query blocks, the last block partial; every rows_per_pos the entry takes (1, 2, 4, 8, 16) and
both layers.  Batch order, peaked scores, long chunks, the layout's end, striped pools, the K pre-scale and never-written pages: the
second half of this file."""
import contextlib
import types

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, torch_mod
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_spec_step import SCHEMES, _region

pytestmark = pytest.mark.gpu
L, T, S = 2, 256, 70
LAYER = 1
PROMPTS = [0, 1, 2, 37, 64, 98]
N_NEW = [70, 33, 17, 16, 1, 0]
RIDS = list(range(len(PROMPTS)))
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19

_data, _kv64 = {}, {}


def _inputs(rpp):
    """the batch's prompts, new rows and query rows: the same for every scheme and every test"""
    if "prompts" not in _data:
        rng = np.random.default_rng(2024)
        _data["prompts"] = [(rng.standard_normal((L, n, H, D)).astype(np.float16), rng.standard_normal((L, n, H, D)).astype(np.float16)) for n in PROMPTS]
        _data["new"] = (rng.standard_normal((len(PROMPTS), S, L, H, D)).astype(np.float16), rng.standard_normal((len(PROMPTS), S, L, H, D)).astype(np.float16))
    if ("q", rpp) not in _data:
        _data[("q", rpp)] = np.random.default_rng(77 + rpp).standard_normal((len(PROMPTS), S, H, rpp, D)).astype(np.float16)
    return _data["prompts"], _data["new"], _data[("q", rpp)]


def _stored64(oracle, scheme, b, k, v, head, layer=LAYER):
    """float64 K and V rows of the even part of a prompt's layer, kv head `head`, as the oracle's records hold them (computed once per
    prompt and layer)"""
    key = (scheme, b, layer, k.shape[1], float(np.abs(k[layer].astype(np.float32)).sum()), float(np.abs(v[layer].astype(np.float32)).sum()))
    if key not in _kv64:
        even = k.shape[1] & ~1
        _kv64[key] = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], T), T)
    return _kv64[key].kv(head)


@contextlib.contextmanager
def _batch(torch, scheme, prompts, rids=None, kscale=None, **env):
    """a connector whose requests hold the prompts; kscale: a K pre-scale [L][H][D] set before the first write"""
    lib = open_lib(**env) if env else pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
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


def _entry(torch, lib, conn, rids, q, k_new, v_new, n_new, layer=LAYER, fill=None, **change):
    """speckv_ext_attend_chunk itself over what the connector holds: (out, lse) as numpy, [B][S][H][R][D] and [B][S][H][R].  fill: the
    32-bit pattern out and lse hold before the call.  change: arguments to replace (the refusals)."""
    B, C_, _, R, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    st = torch.cuda.Stream()
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
    args = dict(handles=np.asarray([r.handle for r in reqs], np.uint64), layer=layer, d_q=dq.data_ptr(), C=C_, rows_per_pos=R,
                pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), n_q=np.asarray(n_new, np.uint32),
                d_k_new=dk.data_ptr() + 2 * layer * dk.stride(2), d_v_new=dv.data_ptr() + 2 * layer * dv.stride(2), seq_stride=dk.stride(0),
                pos_stride=dk.stride(1), tail_idx=np.asarray(tail_idx, np.int32), d_k_tail=tk.data_ptr() + 2 * layer * row if tails else 0,
                d_v_tail=tv.data_ptr() + 2 * layer * row if tails else 0, tail_stride=L * row, sm_scale=SM, d_out=out.data_ptr(),
                d_lse=lse.data_ptr(), stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    lib.attend_chunk(**args)
    st.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def _f32(x):
    return x.view(np.float32)


def _reference(K, V, tail, q, kn, vn):
    """float64: q [n][R][D] fp16 as given, stored rows K / V [even][D], tail (k [D], v [D]) fp16 or None, new rows kn / vn [n][D] fp16 ->
    out [n][R][D], lse [n][R], mag [n][R][D] = sum p|v|"""
    n, R, _ = q.shape
    parts_k, parts_v = [K], [V]
    if tail is not None:
        parts_k.append(tail[0][None].astype(np.float64)); parts_v.append(tail[1][None].astype(np.float64))
    Ka, Va = np.concatenate(parts_k + [kn.astype(np.float64)]), np.concatenate(parts_v + [vn.astype(np.float64)])
    s = (q.astype(np.float64).reshape(n * R, D) @ Ka.T) * SM
    sees = len(K) + (tail is not None) + np.arange(n * R) // R + 1                # itself included
    s[np.arange(len(Ka))[None, :] >= sees[:, None]] = -np.inf
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return ((p @ Va) / l[:, None]).reshape(n, R, D), (mx + np.log(l)).reshape(n, R), ((p @ np.abs(Va)) / l[:, None]).reshape(n, R, D)


def _check64(oracle, scheme, conn, b, rid, prompt, q, new, n, out, lse, what, layer=LAYER):
    """rows of request b's first n new positions against float64 at `layer`; lse None: the output only (the connector returns no lse).
    Returns the worst err / tol"""
    k, v = prompt
    even, worst = k.shape[1] & ~1, 0.0
    r = conn.requests[rid]
    for head in range(H):
        K, V = _stored64(oracle, scheme, b, k, v, head, layer)
        tail = None if not r.length & 1 else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        want, wlse, mag = _reference(K[:even], V[:even], tail, q[b, :n, head], new[0][b, :n, layer, head], new[1][b, :n, layer, head])
        err, tol = np.abs(_f32(out)[b, :n, head] - want), 2e-3 * mag + 1e-6
        lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, :n, head] - wlse)
        worst = max(worst, float((err / tol).max()), float(lerr.max() / 2e-3))
        assert np.all(err <= tol), (what, scheme, b, head, "out", float((err / tol).max()))
        assert np.all(lerr <= 2e-3), (what, scheme, b, head, "lse", float(lerr.max()))
    return worst


@pytest.mark.parametrize("rpp", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_attend_chunk_against_float64(oracle, scheme, rpp):
    """the entry over the ragged batch against float64 at layer 0 (k_first = 0) and at layer 1, and SpeckvKVConnector.attend_chunk
    gives the entry's bits (zeros for the rows of positions that are not live)"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out0, lse0 = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, layer=0)
        worst = max(_check64(oracle, scheme, conn, b, b, prompts[b], q, new, N_NEW[b], out0, lse0, "batch, layer 0", layer=0) for b in RIDS if N_NEW[b])
        print(f"attend_chunk {scheme} rows_per_pos {rpp} layer 0: worst err / tol {worst:.3f}")
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW)
        worst = max(_check64(oracle, scheme, conn, b, b, prompts[b], q, new, N_NEW[b], out, lse, "batch") for b in RIDS if N_NEW[b])
        print(f"attend_chunk {scheme} rows_per_pos {rpp}: worst err / tol {worst:.3f}")
        lengths = [conn.length(r) for r in RIDS]
        got = conn.attend_chunk(LAYER, RIDS, torch.from_numpy(q).cuda(), torch.from_numpy(new[0]).cuda(), torch.from_numpy(new[1]).cuda(), SM, N_NEW)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert [conn.length(r) for r in RIDS] == lengths                  # no state changes
        for b, n in enumerate(N_NEW):
            assert np.array_equal(got[b, :n].view(np.uint32), out[b, :n].view(np.uint32)), (scheme, rpp, b)
            assert not got[b, n:].any()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_rows_of_positions_that_are_not_live_are_not_written(scheme):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN)
        for b, n in enumerate(N_NEW):
            assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, b)
            assert np.all(np.isfinite(_f32(out)[b, :n])) and not np.any(out[b, :n] == PATTERN) and not np.any(lse[b, :n] == PATTERN)


def _causal_probe(torch, lib, conn, rids, q, new, n_new, js, what):
    """new rows behind position j replaced, for every j of js: rows <= j keep their bits, every later row changes"""
    other = np.random.default_rng(5).standard_normal((2,) + new[0].shape).astype(np.float16)
    out, lse = _entry(torch, lib, conn, rids, q, new[0], new[1], n_new)
    for j in js:
        k2, v2 = new[0].copy(), new[1].copy()
        k2[:, j + 1:], v2[:, j + 1:] = other[0][:, j + 1:], other[1][:, j + 1:]
        out2, lse2 = _entry(torch, lib, conn, rids, q, k2, v2, n_new)
        for b, n in enumerate(n_new):
            keep = min(n, j + 1)
            assert np.array_equal(out2[b, :keep], out[b, :keep]) and np.array_equal(lse2[b, :keep], lse[b, :keep]), (what, j, b)
            changed = (out2[b, keep:n] != out[b, keep:n]).any(axis=-1)
            assert changed.all(), (what, j, b, "a row that sees a replaced position kept its bits")


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_a_row_does_not_see_the_positions_behind_it(scheme):
    """new rows behind position j replaced, j on and beside the edges of query blocks (16 positions at rows_per_pos 4) and of held tiles
    (32 positions; requests with a tail are shifted by one): rows <= j keep their bits, every later row changes"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts) as (lib, conn):
        _causal_probe(torch, lib, conn, RIDS, q, new, N_NEW, (15, 16, 30, 31, 32, 63), scheme)


@pytest.mark.parametrize("rpp,js", [(16, (3, 4, 7, 31, 32)), (2, (31, 32, 63))])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_a_row_does_not_see_the_positions_behind_it_at_other_rows_per_pos(scheme, rpp, js):
    """the same probe where a wave owns ONE position and a query block is 4 (rows_per_pos 16: j on and beside the block edges, and at
    the held tile's edge), and where a query block is exactly one held tile (rows_per_pos 2: 32 positions)"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        _causal_probe(torch, lib, conn, RIDS, q, new, N_NEW, js, (scheme, rpp))


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_a_request_alone_gives_the_bits_it_gives_inside_the_batch(scheme):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW)
        for b, n in enumerate(N_NEW):
            if n == 0:
                continue
            one, one_lse = _entry(torch, lib, conn, [b], q[b:b + 1], new[0][b:b + 1], new[1][b:b + 1], [n])
            assert np.array_equal(one[0, :n], out[b, :n]) and np.array_equal(one_lse[0, :n], lse[b, :n]), (scheme, b)


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_records_behind_a_cut_are_not_seen(oracle, scheme):
    """64 positions whose last 27 are 1000 x larger, cut to 37: the pages of positions 38..63 keep their records, and the chunk's rows
    stay within the float64 bound of the 37 positions the request holds"""
    torch = torch_mod()
    _, new, q = _inputs(4)
    rng = np.random.default_rng(9)
    k, v = rng.standard_normal((L, 64, H, D)).astype(np.float16), rng.standard_normal((L, 64, H, D)).astype(np.float16)
    k[:, 37:] *= np.float16(1000); v[:, 37:] *= np.float16(1000)
    with _batch(torch, scheme, [(k, v)]) as (lib, conn):
        conn.truncate([0], [37])
        torch.cuda.synchronize()
        assert conn.length(0) == 37
        out, lse = _entry(torch, lib, conn, [0], q[:1], new[0][:1], new[1][:1], [S])
        worst = _check64(oracle, scheme, conn, 0, 0, (k[:, :36], v[:, :36]), q, new, S, out, lse, "behind a cut")
        print(f"attend_chunk {scheme} behind a cut: worst err / tol {worst:.3f}")


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_migrated_pages_give_the_same_bits(scheme):
    """two pools of the one GPU; pages of the longest request move between them (a tile's last and next first K pages, one V page):
    every row keeps its bits"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    n_new = [S] * len(RIDS)
    with _batch(torch, scheme, prompts, SPECKV_POOL_DEVICES="0,0") as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], n_new)
        h = conn.requests[5].handle
        lib.migrate(h, LAYER * T + 15, 3, 1)
        lib.migrate(h, LAYER * T + T // 2 + 2, 1, 0)
        lib.migrate(h, LAYER * T + 40, 2, 0)
        out2, lse2 = _entry(torch, lib, conn, RIDS, q, new[0], new[1], n_new)
        assert np.array_equal(out2, out) and np.array_equal(lse2, lse)


@pytest.mark.parametrize("start", ["empty", "fork"])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_chunked_prefill_end_to_end(oracle, scheme, start):
    """chunks of 33, 70 and 1 positions onto an empty request / onto a fork of a 37-position prefix, attend_chunk per layer and commit per
    chunk: the request is, bit for bit, the one write_prefill makes of the whole prompt -- kv_rows and a following attend step"""
    torch = torch_mod()
    chunks, prefix = (33, 70, 1), 37 if start == "fork" else 0
    total = prefix + sum(chunks)
    rng = np.random.default_rng(31)
    k, v = rng.standard_normal((L, total, H, D)).astype(np.float16), rng.standard_normal((L, total, H, D)).astype(np.float16)
    rpp = 4
    with _batch(torch, scheme, [(k, v)], rids=[10]) as (lib, whole):
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        if prefix:
            conn.add_request(20)
            held = conn.write_prefill(20, torch.from_numpy(k[:, :prefix]).cuda(), torch.from_numpy(v[:, :prefix]).cuda())
            conn.fork([20], [21])
        else:
            conn.add_request(21)
        at, keep = prefix, []
        for n in chunks:
            kc = torch.from_numpy(np.ascontiguousarray(k[:, at:at + n].transpose(1, 0, 2, 3))[None]).cuda()      # [1][n][L][H][D]
            vc = torch.from_numpy(np.ascontiguousarray(v[:, at:at + n].transpose(1, 0, 2, 3))[None]).cuda()
            qc = rng.standard_normal((L, 1, n, H, rpp, D)).astype(np.float16)
            for layer in range(L):
                got = conn.attend_chunk(layer, [21], torch.from_numpy(qc[layer]).cuda(), kc, vc, SM)
                if layer == LAYER and at == prefix:                                  # the first chunk against float64, as a sanity check
                    torch.cuda.synchronize()
                    o = got.cpu().numpy()
                    new = (kc.cpu().numpy(), vc.cpu().numpy())
                    for head in (0, H - 1):
                        K, V = _stored64(oracle, scheme, 0, k[:, :prefix], v[:, :prefix], head)
                        r = conn.requests[21]
                        tail = None if not r.length & 1 else (r.tail_k[LAYER, head].cpu().numpy(), r.tail_v[LAYER, head].cpu().numpy())
                        want, _, mag = _reference(K[:prefix & ~1], V[:prefix & ~1], tail, qc[layer, 0, :, head], new[0][0, :, LAYER, head], new[1][0, :, LAYER, head])
                        assert np.all(np.abs(o[0, :, head] - want) <= 2e-3 * mag + 1e-6), (scheme, start, head)
            keep += conn.commit([21], kc, vc, [range(n)])
            at += n
        torch.cuda.synchronize()
        assert conn.length(21) == whole.length(10) == total
        for layer in range(L):
            for kind in (0, 1):
                a = conn.kv_rows(21, layer, kind).cpu().numpy().view(np.uint16)
                b = whole.kv_rows(10, layer, kind).cpu().numpy().view(np.uint16)
                assert np.array_equal(a, b), (scheme, start, layer, kind)
            qd = torch.from_numpy(rng.standard_normal((1, H, rpp, D)).astype(np.float16)).cuda()
            a, b = conn.attend(layer, [21], qd, SM), whole.attend(layer, [10], qd, SM)
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)), (scheme, start, layer)


def test_attend_chunk_refuses_bad_arguments_and_launches_nothing():
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
        run = lambda **change: _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN, **change)
        before = bytes(lib.stats())
        invalid = {
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
        for what, change in invalid.items():
            with pytest.raises(SpeckvError) as e:
                out, lse = run(**change)
                pytest.fail(what)
            assert e.value.status == -4, (what, e.value.status)             # SPECKV_ERR_INVAL
        with pytest.raises(SpeckvError) as e:
            run(handles=with_handle(1, 0xDEAD))
        assert e.value.status == -1                                          # SPECKV_ERR_GENERAL: an unknown handle
        torch.cuda.synchronize()
        assert bytes(lib.stats()) == before, "a refused call counted something"
        # nothing to do: no launch, nothing written
        out, lse = run(n_q=np.zeros(len(RIDS), np.uint32))
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)
        none = lambda t: np.zeros(1, t)[:0]
        lib.attend_chunk(none(np.uint64), 0, 16, 1, 1, none(np.uint32), none(np.uint32), 16, 16, 1024, 1024, None, 0, 0, 0, 1.0, 16, 0, 1)
        assert bytes(lib.stats()) == before


# =============================================================================
# Where the flat, ordered batch above does not look: branches and index expressions of k_attend_chunk that it cannot tell from wrong
# ones.  Same helpers, reference and bound.
#   batch order    sequences without live positions first, two in a row in the middle, n_q ascending: the kernel's own search
#   peaked scores  a key c x the query row (c = 0.75: the other weights small; c = 2: they underflow in fp16) in every kind of tile, so
#                  that the running maximum jumps, alpha is tiny and a rescale that is missing or misplaced costs the whole output
#   long chunk     200 new positions: 7 held tiles, 13 / 50 query blocks, waves of one block 2 tiles apart
#   layout         255 positions (the last K and V pages of a layer's regions) at both layers; a pool striped over 3
#   K pre-scale    SpeckvKVConnector.attend_chunk with set_k_channel_scale, before and after a commit
#   never written  pages inside [0, pos_end) without a record: zeros, score 0 (not -inf)
# What no input reaches: an FP8 record shorter than 2048 bytes (the `p0 < r.len` branches of load_pool / decode_pool with 0 < len).  The
# FP8 encoders of the library and of the oracle write one byte per element of a whole block; a record is 2048 bytes or was never
# written (len 0, covered here).
# =============================================================================
ALL = ["fp8", "int4", "mxfp4"]


def _rows(rng, *shape):
    return rng.standard_normal(shape).astype(np.float16)


# ----------------------------------------------------------------------------- batch order
@pytest.mark.parametrize("n_q", [[0, 70, 0, 0, 17, 1], [1, 0, 16, 17, 0, 70]], ids=["empty-first-and-twice", "ascending"])
@pytest.mark.parametrize("scheme", ALL)
def test_sequences_without_live_positions_anywhere_in_the_batch(oracle, scheme, n_q):
    """the prompts of the ragged batch with n_q = 0 first, twice in a row in the middle and before the last, and n_q ascending: every
    live row within the float64 bound and, bit for bit, what its request gives alone in a launch; dead rows keep the fill pattern"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], n_q, fill=PATTERN)
        worst = max(_check64(oracle, scheme, conn, b, b, prompts[b], q, new, n_q[b], out, lse, "order") for b in RIDS if n_q[b])
        print(f"attend_chunk {scheme} n_q {n_q}: worst err / tol {worst:.3f}")
        for b, n in enumerate(n_q):
            assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, b, "a dead row was written")
            if n:
                one, one_lse = _entry(torch, lib, conn, [b], q[b:b + 1], new[0][b:b + 1], new[1][b:b + 1], [n])
                assert np.array_equal(one[0, :n], out[b, :n]) and np.array_equal(one_lse[0, :n], lse[b, :n]), (scheme, b)


# ----------------------------------------------------------------------------- peaked scores
J, HEAD, SUB, VCONST = 40, 5, 2, 6.0                 # the query row the needles are aligned to: position J (69 / 45 where a case says so)
# name -> (prompt length, [(where, position, c)], query position)
NEEDLES = {
    "stored-0": (98, [("stored", 0)], J), "stored-31": (98, [("stored", 31)], J), "stored-32": (98, [("stored", 32)], J),
    "stored-97": (98, [("stored", 97)], J), "tail": (99, [("stored", 98)], J), "new-0": (98, [("new", 0)], J),
    "new-33": (98, [("new", 33)], J), "itself-69": (98, [("new", 69)], 69),
}


def _peaked(name, c):
    """prompt (k, v) [L][n][H][D], new (k, v) [1][S][L][H][D], q [1][S][H][4][D], the new rows without needles, the first new position a
    needle is at (or None), the query position the needles are aligned to"""
    if name == "late-jump":                         # c = 0.75 in the first pool tile, c = 2 at new position 40: the maximum jumps late
        n, places, j = 98, [("stored", 0, 0.75), ("new", 40, 2.0)], 45
    else:
        n, places, j = NEEDLES[name][0], [p + (c,) for p in NEEDLES[name][1]], NEEDLES[name][2]
    rng = np.random.default_rng(4242)
    k, v = _rows(rng, L, n, H, D), _rows(rng, L, n, H, D)
    kn, vn, q = _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, L, H, D), _rows(rng, 1, S, H, 4, D)
    plain, first_new = (kn.copy(), vn.copy()), None
    for where, pos, cc in places:
        needle = (np.float32(cc) * q[0, j, HEAD, SUB].astype(np.float32)).astype(np.float16)
        if where == "stored":
            k[LAYER, pos, HEAD], v[LAYER, pos, HEAD] = needle, np.float16(VCONST)
        else:
            kn[0, pos, LAYER, HEAD], vn[0, pos, LAYER, HEAD] = needle, np.float16(VCONST)
            first_new = pos if first_new is None else min(first_new, pos)
    return (k, v), (kn, vn), q, plain, first_new, j


@pytest.mark.parametrize("case", [(n, c) for n in NEEDLES for c in (0.75, 2.0)] + [("late-jump", None)], ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("scheme", ALL)
def test_a_key_that_takes_nearly_all_the_weight(oracle, scheme, case):
    """one request of 98 (99) positions and 70 new ones; a key c x the query row (J, HEAD, SUB) with a V row of 6.0 at one position: the
    needle scores about 8 (c = 0.75) and 22 (c = 2) natural units above the N(0, 1) rest.  Every row against float64 under the
    project's bound: weights rounded to fp16 and the same rounded weights summed cost <= 2 x 2^-11 of sum p|v|; fp32 accumulation of
    exact fp16 products over 128 terms costs a score < 1e-4 while sum |q_d k_d| sm < 64, asserted here for the inputs used.  Rows of
    positions in front of a needle among the new positions keep the bits they have without it."""
    torch = torch_mod()
    name, c = case
    prompt, new, q, plain, first_new, j = _peaked(name, c)
    with _batch(torch, scheme, [prompt]) as (lib, conn):
        r = conn.requests[0]
        reach = 0.0
        for head in range(H):
            K, _ = _stored64(oracle, scheme, 0, prompt[0], prompt[1], head)
            keys = [np.abs(K[:r.length & ~1]), np.abs(new[0][0, :, LAYER, head].astype(np.float64))]
            if r.length & 1:
                keys.append(np.abs(r.tail_k[LAYER, head].cpu().numpy().astype(np.float64))[None])
            reach = max(reach, float((np.abs(q[0, :, head].astype(np.float64)).reshape(-1, D) @ np.concatenate(keys).T).max()) * SM)
        assert reach < 64.0, ("the inputs left the reach of the bound's argument", reach)
        out, lse = _entry(torch, lib, conn, [0], q, new[0], new[1], [S])
        worst = _check64(oracle, scheme, conn, 0, 0, prompt, q, new, S, out, lse, ("peaked", name, c))
        print(f"attend_chunk {scheme} needle {name} c {c}: worst err / tol {worst:.3f} (sum |q k| sm <= {reach:.1f})")
        # the aligned row is the needle's: its output is the needle's V row to within the weight of the rest
        if c == 2.0 or name == "late-jump":
            assert np.all(np.abs(_f32(out)[0, j, HEAD, SUB] - VCONST) < 1e-2), (scheme, name, _f32(out)[0, j, HEAD, SUB, :4])
        if first_new:
            out2, lse2 = _entry(torch, lib, conn, [0], q, plain[0], plain[1], [S])                   # the same rows without the needle
            assert np.array_equal(out2[0, :first_new], out[0, :first_new]) and np.array_equal(lse2[0, :first_new], lse[0, :first_new])
            assert (out2[0, first_new:, HEAD] != out[0, first_new:, HEAD]).any(axis=-1).all()


# ----------------------------------------------------------------------------- long chunk
S_LONG = 200


def _long_inputs(rpp):
    if "long" not in _data:
        rng = np.random.default_rng(808)
        _data["long"] = ([(_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in (0, 1)], (_rows(rng, 2, S_LONG, L, H, D), _rows(rng, 2, S_LONG, L, H, D)))
    if ("long q", rpp) not in _data:
        _data[("long q", rpp)] = _rows(np.random.default_rng(809 + rpp), 2, S_LONG, H, rpp, D)
    return _data["long"] + (_data[("long q", rpp)],)


@pytest.mark.parametrize("scheme,rpp", [("fp8", 4), ("int4", 4), ("mxfp4", 4), ("int4", 16)])
def test_a_chunk_of_200_positions(oracle, scheme, rpp):
    """an empty request and one that holds a single position (a tail only), 200 new positions each: 7 held tiles, 13 (rows_per_pos 4)
    and 50 (16) query blocks per request, blocks whose rows see 4 to 7 held tiles and whose first wave is 2 tiles behind its last.
    Every row against float64, and the causal probe on and beside the edges of the later held tiles"""
    torch = torch_mod()
    prompts, new, q = _long_inputs(rpp)
    n_new = [S_LONG, S_LONG]
    with _batch(torch, scheme, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, [0, 1], q, new[0], new[1], n_new)
        worst = max(_check64(oracle, scheme, conn, b, b, prompts[b], q, new, S_LONG, out, lse, "long") for b in (0, 1))
        print(f"attend_chunk {scheme} rows_per_pos {rpp} 200 positions: worst err / tol {worst:.3f}")
        _causal_probe(torch, lib, conn, [0, 1], q, new, n_new, (63, 64, 127, 128, 191, 199), (scheme, rpp, "long"))


# ----------------------------------------------------------------------------- layer, layout end, striped pool
@pytest.mark.parametrize("scheme", ALL)
def test_the_last_pages_of_a_layer(oracle, scheme):
    """a request of 255 positions -- pos_end 254, a tail, the last K and V pages of each layer's regions -- takes one new position
    through the entry (the connector's limit, 255 + 1 = T), at both layers"""
    torch = torch_mod()
    rng = np.random.default_rng(255)
    prompt = (_rows(rng, L, T - 1, H, D), _rows(rng, L, T - 1, H, D))
    new, q = (_rows(rng, 1, 1, L, H, D), _rows(rng, 1, 1, L, H, D)), _rows(rng, 1, 1, H, 4, D)
    with _batch(torch, scheme, [prompt]) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, [0], q, new[0], new[1], [1], layer=layer)
            worst = _check64(oracle, scheme, conn, 0, 0, prompt, q, new, 1, out, lse, ("255 positions", layer), layer=layer)
            print(f"attend_chunk {scheme} 255 positions layer {layer}: worst err / tol {worst:.3f}")


@pytest.mark.parametrize("scheme", ALL)
def test_a_pool_striped_over_three(oracle, scheme):
    """the ragged batch over three pools of the one GPU (pages striped page by page), both layers against float64"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts, SPECKV_POOL_DEVICES="0,0,0") as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, layer=layer)
            worst = max(_check64(oracle, scheme, conn, b, b, prompts[b], q, new, N_NEW[b], out, lse, ("striped", layer), layer=layer)
                        for b in RIDS if N_NEW[b])
            print(f"attend_chunk {scheme} striped over 3 layer {layer}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- K pre-scale
def _kscale():
    kscale = np.ones((L, H, D), np.float32)
    kscale[:, :, 0::8] = 4.0; kscale[:, :, 3::8] = 0.25
    return kscale


def _f16_times(x, s):
    """x (fp16) * s (powers of two), rounded once to fp16 as the connector's fp16 multiply rounds"""
    return (x.astype(np.float32) * s).astype(np.float16)


@pytest.mark.parametrize("scheme", ALL)
def test_connector_attend_chunk_with_a_k_pre_scale(oracle, scheme):
    """SpeckvKVConnector.attend_chunk of a connector with set_k_channel_scale (4.0 on channels 0::8, 0.25 on 3::8) against float64 over
    what the kernel is given: the oracle's records of k / scale, the tails as held, k_new / scale and q x scale.  Then the chunk is
    committed and a second chunk attends: its rows go against float64 over the records of the longer, pre-scaled prompt"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    ks = _kscale()
    inv = (1.0 / ks)
    dev = lambda x: torch.from_numpy(x).cuda()
    pre = [(_f16_times(k, inv[:, None]), v) for k, v in prompts]                                    # [L][n][H][D] / [L][1][H][D]
    new_pre = (_f16_times(new[0], inv[None, None]), new[1])                                          # [B][S][L][H][D]
    rng = np.random.default_rng(66)
    S2 = 20
    new2, q2 = (_rows(rng, len(RIDS), S2, L, H, D), _rows(rng, len(RIDS), S2, L, H, D)), _rows(rng, len(RIDS), S2, H, 4, D)
    new2_pre = (_f16_times(new2[0], inv[None, None]), new2[1])
    with _batch(torch, scheme, prompts, kscale=ks) as (lib, conn):
        for layer in range(L):
            qs = _f16_times(q, ks[layer][None, None, :, None, :])
            got = conn.attend_chunk(layer, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            worst = max(_check64(oracle, scheme, conn, b, b, pre[b], qs, new_pre, N_NEW[b], got, None, ("pre-scale", layer), layer=layer)
                        for b in RIDS if N_NEW[b])
            print(f"attend_chunk {scheme} K pre-scale layer {layer}: worst err / tol {worst:.3f}")
            for b, n in enumerate(N_NEW):
                assert not got[b, n:].any()
        keep = conn.commit(RIDS, dev(new[0]), dev(new[1]), [range(n) for n in N_NEW])
        torch.cuda.synchronize()
        assert [conn.length(b) for b in RIDS] == [p + n for p, n in zip(PROMPTS, N_NEW)]
        longer = [(np.concatenate([pre[b][0], new_pre[0][b, :n].transpose(1, 0, 2, 3)], axis=1),
                   np.concatenate([pre[b][1], new_pre[1][b, :n].transpose(1, 0, 2, 3)], axis=1)) for b, n in enumerate(N_NEW)]
        for layer in range(L):
            qs = _f16_times(q2, ks[layer][None, None, :, None, :])
            got = conn.attend_chunk(layer, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            worst = max(_check64(oracle, scheme, conn, b, b, longer[b], qs, new2_pre, S2, got, None, ("pre-scale, after a commit", layer),
                                 layer=layer) for b in RIDS)
            print(f"attend_chunk {scheme} K pre-scale after a commit layer {layer}: worst err / tol {worst:.3f}")
        del keep


# ----------------------------------------------------------------------------- pages never written
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("scheme", ALL)
def test_pages_never_written_count_as_zeros(oracle, scheme, layer):
    """an allocation written through speckv_write except K page 5, V page 9 and the whole second tile (pages 16..31, K and V) of
    pos_end = 64: a never-written K row scores 0, not -inf (it takes the weight exp(0 - max)), a never-written V row adds nothing,
    the output is finite and within the float64 bound of the same prompt with zeros there"""
    torch = torch_mod()
    _, new, q = _inputs(4)
    rng = np.random.default_rng(70 + layer)
    k, v = _rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D)
    k[:, 2 * 5:2 * 5 + 2] = 0; v[:, 2 * 9:2 * 9 + 2] = 0
    k[:, 32:] = 0; v[:, 32:] = 0
    with _batch(torch, scheme, []) as (lib, conn):
        lib.set_compression_scheme(SCHEMES[scheme])
        h = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(h, T, L, H, D, 2)
        page = lambda x, first, n: np.ascontiguousarray(x[layer, 2 * first:2 * (first + n)]).reshape(n, 2 * H * D)
        for x, region, skip in ((k, layer * T, 5), (v, layer * T + T // 2, 9)):
            for first, n in ((0, skip), (skip + 1, 16 - skip - 1)):
                img = page(x, first, n)
                lib.write(h, (region + first) * 4096, img.ctypes.data, img.nbytes, False)
        lib.sync()
        held = types.SimpleNamespace(requests={0: types.SimpleNamespace(handle=h, length=64, tail_k=None, tail_v=None)})
        n = 33
        out, lse = _entry(torch, lib, held, [0], q[:1], new[0][:1], new[1][:1], [n], layer=layer, fill=PATTERN)
        assert np.all(np.isfinite(_f32(out)[0, :n])) and np.all(np.isfinite(_f32(lse)[0, :n]))
        assert np.all(out[0, n:] == PATTERN) and np.all(lse[0, n:] == PATTERN)
        worst = _check64(oracle, scheme, held, 0, 0, (k, v), q, new, n, out, lse, ("never written", layer), layer=layer)
        print(f"attend_chunk {scheme} never-written pages layer {layer}: worst err / tol {worst:.3f}")
        lib.free(h)
