"""-m gpu: the split pool's decode route -- speckv_ext_attend_kv_batch (k_attend_k8v4: K from the FP8_E4M3 allocation's records, V from the
MXFP4 allocation's, one batch launch and its merge) and SpeckvSplitKVConnector.attend on top of it.

Reference: numpy float64 softmax attention where the query is what HeadChecker(oracle, FP8).q_rows gives (E4M3 x a row scale, the oracle's
own quantiser), K is HeadChecker(oracle, FP8).kv(head)[0] and V is HeadChecker(oracle, MXFP4).kv(head)[1] -- the oracle's records of the
rows that were written.  Bound: the project's for the kernels with an 8-bit query (tests/_gpu.py check_rows): |err| <= (2e-3 + 2 delta)
sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta = 3e-5 max sum |q||k| sm per (member, head); a member without positions is exactly 0
with lse -inf.  Every (member, head, row) is compared.  Geometry: L = 2, T = 256 (8 tiles a region), H = 8, D = 128; the ragged batch has
0, 2, 30, 32, 34, 64, 98 and 256 positions (nothing, one page, a ragged first tile, one whole tile, a ragged second tile, two tiles, a ragged
fourth tile, the whole region); all members are prefixes of one prompt whose two layers differ."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, decide, load_rules
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
L, T = 2, 256
LENGTHS = [0, 2, 30, 32, 34, 64, 98, 256]
RIDS = list(range(len(LENGTHS)))
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19
FP8, MX4 = 4, 5

_data, _checkers = {}, {}


def _rows(rng, *shape):
    return rng.standard_normal(shape).astype(np.float16)


def _prompt():
    """the one prompt [L][T][H][D] (K, V) every member of the ragged batch is a prefix of"""
    if "prompt" not in _data:
        rng = np.random.default_rng(2027)
        _data["prompt"] = (_rows(rng, L, T, H, D), _rows(rng, L, T, H, D))
    return _data["prompt"]


def _query(g, batch=len(LENGTHS)):
    if ("q", g, batch) not in _data:
        _data[("q", g, batch)] = _rows(np.random.default_rng(300 + g), batch, H, g, D)
    return _data[("q", g, batch)]


def _checker(oracle, tag, k, v, layer):
    """(HeadChecker over the FP8 records, HeadChecker over the MXFP4 records) of the even part of rows k, v [L][n][H][D] at `layer`; once per tag"""
    key = (tag, layer)
    if key not in _checkers:
        even = k.shape[1] & ~1
        region = _region(k[layer, :even], v[layer, :even], T)
        _checkers[key] = (HeadChecker(oracle, FP8, region, T), HeadChecker(oracle, MX4, region, T))
    return _checkers[key]


def _check(pair, out, lse, q, npos, what, tails=None):
    """out [M][H][G][D], lse [M][H][G] (fp32; None: a call that returns the rows alone) of M members over the content of `pair`, member m
    attending its first npos[m] positions (and its fp16 tail (k [H][D], v [H][D]) = tails[m] if that is not None, scored with the fp16
    query) against float64.  Returns the worst err / tol."""
    k8, v4 = pair
    M, _, G, _ = q.shape
    worst = 0.0
    for head in range(H):
        K, V = k8.kv(head)[0], v4.kv(head)[1]
        qe = k8.q_rows(q[:, head]).reshape(M, G, D)
        for m in range(M):
            n = int(npos[m])
            tail = None if tails is None else tails[m]
            if n == 0 and tail is None:
                assert not out[m, head].any() and (lse is None or np.all(lse[m, head] == -np.inf)), (what, m, head, "an empty member is exactly 0 with lse -inf")
                continue
            s = (qe[m] @ K[:n].T) * SM                                           # [G][n]
            delta = 3e-5 * float((np.abs(qe[m]) @ np.abs(K[:n]).T).max(initial=0.0)) * SM
            vals, mags = V[:n], np.abs(V[:n])
            if tail is not None:
                st = (q[m, head].astype(np.float64) @ tail[0][head].astype(np.float64)) * SM
                s = np.concatenate([s, st[:, None]], axis=1)
                vals = np.concatenate([vals, tail[1][head].astype(np.float64)[None]])
                mags = np.abs(vals)
            mx = s.max(axis=1)
            p = np.exp(s - mx[:, None])
            l = p.sum(axis=1)
            want, mag, wlse = (p @ vals) / l[:, None], (p @ mags) / l[:, None], mx + np.log(l)
            err, tol = np.abs(out[m, head].astype(np.float64) - want), (2e-3 + 2 * delta) * mag + 1e-6
            lerr, ltol = (np.zeros(G) if lse is None else np.abs(lse[m, head].astype(np.float64) - wlse)), 2e-3 + delta
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nan_to_num(err / tol, nan=np.inf).max()), float(np.nan_to_num(lerr / ltol, nan=np.inf).max()))
            assert np.all(err <= tol), (what, m, head, "out", float((err / tol).max()))
            assert np.all(lerr <= ltol), (what, m, head, "lse", float(lerr.max()), ltol)
    return worst


@contextlib.contextmanager
def _batch(torch, prompts, rids=None):
    """a split connector whose requests hold the prompts [(k, v)] of [L][n][H][D] each"""
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        keep = []
        for rid, (k, v) in zip(rids if rids is not None else range(len(prompts)), prompts):
            conn.add_request(rid)
            if k.shape[1]:
                keep += conn.write_prefill(rid, torch.from_numpy(np.ascontiguousarray(k)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda())
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
        del keep
    finally:
        lib.finalize()


def _ragged():
    k, v = _prompt()
    return [(k[:, :n], v[:, :n]) for n in LENGTHS]


def _prepare(torch, conn, rids, q, layer, fill=PATTERN, on=None, **change):
    """the arguments of speckv_ext_attend_kv_batch over what the connector holds -> (args, out, lse, stream, the query on the device)"""
    B, _, G, _ = q.shape
    reqs = [conn.requests[r] for r in rids]
    st = on if on is not None else torch.cuda.Stream()
    dq = q if hasattr(q, "data_ptr") else torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((B, H, G, D), fill, dtype=torch.int32, device="cuda")
    lse = torch.full((B, H, G), fill, dtype=torch.int32, device="cuda")
    args = dict(k_handles=np.asarray([r.k_handle for r in reqs], np.uint64), v_handles=np.asarray([r.v_handle for r in reqs], np.uint64), layer=layer,
                d_q_f16=dq.data_ptr(), g=G, pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), sm_scale=SM, d_out=out.data_ptr(),
                d_lse=lse.data_ptr(), stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    return args, out, lse, st, dq


def _entry(torch, lib, conn, rids, q, layer, **how):
    """speckv_ext_attend_kv_batch itself: (out [B][H][G][D], lse [B][H][G]) as fp32 numpy"""
    args, out, lse, st, dq = _prepare(torch, conn, rids, q, layer, **how)
    lib.attend_kv_batch(**args)
    st.synchronize()
    return out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)


def _cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- 1. the ragged batch
@pytest.mark.parametrize("g", [1, 4, 8, 16])
def test_the_ragged_batch_against_float64(oracle, g):
    """both layers (their contents differ: layer 1 proves the region addressing in both allocations); nothing keeps the fill pattern"""
    torch = torch_mod()
    k, v = _prompt()
    q = _query(g)
    with _batch(torch, _ragged()) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, RIDS, q, layer)
            assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any()
            worst = _check(_checker(oracle, "prompt", k, v, layer), out, lse, q, LENGTHS, ("ragged", g, layer))
            print(f"attend_kv_batch g {g} layer {layer}: worst err / tol {worst:.3f}")
        # and without a log-sum-exp: the same rows
        only, _ = _entry(torch, lib, conn, RIDS, q, 1, d_lse=0)
        assert np.array_equal(only.view(np.uint32), out.view(np.uint32))


# ----------------------------------------------------------------------------- 2. pieces and the merge
@pytest.mark.parametrize("tuning", [dict(attend_tiles_per_split=1), dict(attend_tiles_per_split=2), dict(attend_order_as_given=1),
                                    dict(attend_tiles_per_split=1, attend_order_as_given=1)])
def test_pieces_the_merge_and_the_dispatch_orders(oracle, tuning):
    """the ragged batch cut into pieces of one and of two tiles (the member of 256 positions: 8 and 4 pieces, partials and the merge; the
    members of one piece final from the attention kernel in the same launch), dispatched by length rows-first, and in the order given.  The
    engine's own rules (tests/_rules.py decide, for the FP8 batch shape the entry decides with) say so first."""
    torch = torch_mod()
    k, v = _prompt()
    q = _query(4)
    tps, as_given = tuning.get("attend_tiles_per_split", 0), tuning.get("attend_order_as_given", 0)
    pages = np.asarray(LENGTHS) // 2
    d = decide(load_rules(), FP8, "batch", pages, _cus(), tuning=(tps, as_given) + DEFAULT_TUNING[2:])
    tiles = (pages + 15) // 16
    assert d["fits"] == 1 and not d["table"] and not d["striped"]
    if tps:
        assert d["tps"] == tps and d["max_splits"] == 8 // tps and [int(x) for x in d["pieces"][:, 1]] == [int(-(-t // tps)) for t in tiles]
    if as_given:
        assert d["by_length"] == 0 and d["rows_first"] == 0
    else:
        assert d["by_length"] == 1 and d["rows_first"] == 1 and d["max_splits"] > 1      # several pieces, the ordered rows-first dispatch
    with _batch(torch, _ragged()) as (lib, conn):
        try:
            for key, value in tuning.items():
                set_tuning(key, value)
            for layer in range(L):
                out, lse = _entry(torch, lib, conn, RIDS, q, layer)
                worst = _check(_checker(oracle, "prompt", k, v, layer), out, lse, q, LENGTHS, ("pieces", tuning, layer))
                print(f"attend_kv_batch {tuning} layer {layer} (pieces at most {d['max_splits']}, rows first {d['rows_first']}): worst err / tol {worst:.3f}")
        finally:
            for key in tuning:
                set_tuning(key, 0)


# ----------------------------------------------------------------------------- 3. the raw entry and the chunk entry
def test_the_decode_entry_and_the_chunk_entry_each_meet_their_own_reference(oracle):
    """the same requests through speckv_ext_attend_kv_batch (E4M3 query: this file's reference) and through speckv_ext_attend_chunk_kv with one
    new position (fp16 query, the new position seen: tests/test_gpu_k8v4.py's reference).  Not compared with each other."""
    from tests.test_gpu_k8v4 import _check64, _entry as chunk_entry
    torch = torch_mod()
    k, v = _prompt()
    g, layer = 4, 1
    q = _query(g)
    rng = np.random.default_rng(31)
    new = (_rows(rng, len(RIDS), 1, L, H, D), _rows(rng, len(RIDS), 1, L, H, D))
    prompts = _ragged()
    with _batch(torch, prompts) as (lib, conn):
        out, lse = _entry(torch, lib, conn, RIDS, q, layer)
        worst = _check(_checker(oracle, "prompt", k, v, layer), out, lse, q, LENGTHS, "decode entry")
        q5 = np.ascontiguousarray(q[:, None])                               # [B][1][H][R][D]
        cout, clse = chunk_entry(torch, lib, conn, RIDS, q5, new[0], new[1], [1] * len(RIDS), layer=layer)
        cworst = max(_check64(oracle, ("decode", b), conn, b, b, prompts[b], q5, new, 1, cout, clse, ("chunk entry", b), layer=layer) for b in RIDS)
        print(f"attend_kv_batch worst err / tol {worst:.3f}; attend_chunk_kv with one new position {cworst:.3f}")


# ----------------------------------------------------------------------------- 4. hostile rows behind the cut
@pytest.mark.parametrize("hostile_from,pos_end", [(64, 64), (64, 40), (40, 40)])
def test_hostile_rows_behind_the_cut(oracle, hostile_from, pos_end):
    """98 positions stored, those from `hostile_from` on with K x 200 and V = +-1000; the raw entry with pos_end 64 (whole tiles) and 40 (a cut
    inside the second tile; with hostile rows from 40 on the masked pages of that tile are the hostile ones): float64 over the kept positions"""
    torch = torch_mod()
    rng = np.random.default_rng(98)
    k, v = _rows(rng, L, 98, H, D), _rows(rng, L, 98, H, D)
    k[:, hostile_from:] = (k[:, hostile_from:].astype(np.float32) * 200).astype(np.float16)
    v[:, hostile_from:] = np.where(rng.integers(0, 2, v[:, hostile_from:].shape) == 1, np.float16(1000), np.float16(-1000))
    q = _query(8, 1)
    with _batch(torch, [(k, v)]) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, [0], q, layer, pos_end=np.asarray([pos_end], np.uint32))
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse))
            worst = _check(_checker(oracle, ("hostile", hostile_from), k, v, layer), out, lse, q, [pos_end], ("hostile", hostile_from, pos_end, layer))
            print(f"attend_kv_batch hostile rows from {hostile_from}, pos_end {pos_end}, layer {layer}: worst err / tol {worst:.3f}")
            assert float(np.abs(out).max()) < 50.0                            # nothing of +-1000 came through


# ----------------------------------------------------------------------------- 5. pages never written
def test_pages_never_written_read_as_zeros(oracle):
    """two stored positions, pos_end = 64: positions 2 .. 63 were never written -- their scores are 0 (not -inf), their V rows zeros"""
    torch = torch_mod()
    rng = np.random.default_rng(5)
    k, v = np.zeros((L, 64, H, D), np.float16), np.zeros((L, 64, H, D), np.float16)
    k[:, :2], v[:, :2] = _rows(rng, L, 2, H, D), _rows(rng, L, 2, H, D)
    q = _query(8, 1)
    with _batch(torch, [(k[:, :2], v[:, :2])]) as (lib, conn):
        for layer in range(L):
            out, lse = _entry(torch, lib, conn, [0], q, layer, pos_end=np.asarray([64], np.uint32))
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(lse))
            worst = _check(_checker(oracle, "never", k, v, layer), out, lse, q, [64], ("never written", layer))
            print(f"attend_kv_batch never-written pages layer {layer}: worst err / tol {worst:.3f}")
            assert np.all(lse >= np.log(62.0) - 1e-3)                          # 62 positions of score 0 are in the sum


# ----------------------------------------------------------------------------- 6. a walk through the connector
def test_a_walk_through_the_connector(oracle):
    """write_prefill(37), then six rounds of (attend at both layers, commit of one position): lengths 37 .. 42, odd (one batch call and one
    fold of the fp16 tail) and even (the batch call alone) in turn; every attend against float64 over a shadow of the committed rows"""
    torch = torch_mod()
    rng = np.random.default_rng(616)
    g = 4
    shadow_k, shadow_v = _rows(rng, L, 37, H, D), _rows(rng, L, 37, H, D)
    with _batch(torch, [(shadow_k, shadow_v)], rids=[9]) as (lib, conn):
        counts = {"attend_kv_batch": 0, "attend_fold_tail": 0}
        for name in counts:
            real = getattr(lib, name)
            setattr(lib, name, (lambda real, name: lambda *a, **k: (counts.__setitem__(name, counts[name] + 1), real(*a, **k))[1])(real, name))
        keep = []
        for step in range(6):
            length = shadow_k.shape[1]
            assert conn.length(9) == length == 37 + step
            q = _rows(rng, L, 1, H, g, D)
            before = dict(counts)
            outs = [conn.attend(layer, [9], torch.from_numpy(q[layer]).cuda(), SM) for layer in range(L)]
            torch.cuda.synchronize()
            assert counts["attend_kv_batch"] == before["attend_kv_batch"] + L
            assert counts["attend_fold_tail"] == before["attend_fold_tail"] + (L if length & 1 else 0)
            even = length & ~1
            for layer in range(L):
                tails = [(shadow_k[layer, -1], shadow_v[layer, -1])] if length & 1 else None
                got = outs[layer].cpu().numpy()
                assert got.shape == (1, H, g, D) and got.dtype == np.float32
                pair = _checker(oracle, ("walk", even), shadow_k, shadow_v, layer)
                worst = _check(pair, got, None, q[layer], [even], ("walk", step, layer), tails)      # (the connector returns the rows alone)
                print(f"walk step {step} (length {length}) layer {layer}: worst err / tol {worst:.3f}")
            kn, vn = _rows(rng, 1, 1, L, H, D), _rows(rng, 1, 1, L, H, D)
            keep += conn.commit([9], torch.from_numpy(kn).cuda(), torch.from_numpy(vn).cuda(), [1])
            shadow_k = np.concatenate([shadow_k, kn[0].transpose(1, 0, 2, 3)], axis=1)
            shadow_v = np.concatenate([shadow_v, vn[0].transpose(1, 0, 2, 3)], axis=1)
        assert conn.length(9) == 43
        torch.cuda.synchronize()
        del keep


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals_launch_nothing():
    torch = torch_mod()
    q = _query(4)
    with _batch(torch, _ragged()) as (lib, conn):
        kh = np.asarray([conn.requests[r].k_handle for r in RIDS], np.uint64)
        vh = np.asarray([conn.requests[r].v_handle for r in RIDS], np.uint64)
        with_h = lambda hs, b, h: np.concatenate([hs[:b], [np.uint64(h)], hs[b + 1:]])
        pos_end = np.asarray(LENGTHS, np.uint32)
        with_pos = lambda b, p: np.concatenate([pos_end[:b], [np.uint32(p)], pos_end[b + 1:]])

        def refused(**change):
            """the status of the refused call; out and lse keep the fill pattern"""
            args, out, lse, st, dq = _prepare(torch, conn, RIDS, q, change.pop("layer", 1), **change)
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_batch(**args)
            st.synchronize(); torch.cuda.synchronize()
            assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all()), (list(change), "a refused call wrote something")
            return e.value.status
        invalid = {
            "swapped handle arrays": dict(k_handles=vh, v_handles=kh),
            "a K allocation of MXFP4": dict(k_handles=with_h(kh, 2, vh[3])), "a V allocation of FP8": dict(v_handles=with_h(vh, 2, kh[3])),
            "an odd pos_end": dict(pos_end=with_pos(4, 33)), "pos_end beyond the layout": dict(pos_end=with_pos(7, T + 2)),
            "g 0": dict(g=0), "g 17": dict(g=17),
            "NULL k_handles": dict(k_handles=None), "NULL v_handles": dict(v_handles=None), "NULL pos_end": dict(pos_end=None, k_handles=kh),
            "NULL q": dict(d_q_f16=0), "NULL out": dict(d_out=0), "a misaligned q": dict(d_q_f16=0x1008),
            "a layer beyond the regions": dict(layer=L), "a layer far beyond": dict(layer=1000),
        }
        for what, change in invalid.items():
            assert refused(**change) == -4, what                             # SPECKV_ERR_INVAL
        for change in (dict(k_handles=with_h(kh, 1, 0xDEAD)), dict(v_handles=with_h(vh, 1, 0xDEAD))):
            assert refused(**change) == -1                                   # SPECKV_ERR_GENERAL: an unknown handle
        # nothing to do: no sequence, nothing written
        args, out, lse, st, dq = _prepare(torch, conn, [], q[:0], 1)
        lib.attend_kv_batch(**args)
        st.synchronize()


def test_a_capturing_stream_is_refused():
    """the valid call on a stream that is being captured: SPECKV_ERR_INVAL, out and lse keep the fill pattern; the same arguments are
    taken once the stream captures no more"""
    torch = torch_mod()
    q = _query(4)
    with _batch(torch, _ragged()) as (lib, conn):
        st = torch.cuda.Stream()
        args, out, lse, _, dq = _prepare(torch, conn, RIDS, q, 1, on=st)
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, st):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_batch(**args)
            assert e.value.status == -4
            bump.add_(1)
        del g
        torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and bool((lse == PATTERN).all())
        lib.attend_kv_batch(**args)
        st.synchronize()
        assert not bool((out == PATTERN).any()) and not bool((lse == PATTERN).any())


# ----------------------------------------------------------------------------- 8. two streams
def test_two_calls_on_two_streams(oracle):
    """the two layers of the ragged batch issued back to back on two streams, neither waited for in between: bit for bit what each gives
    alone (the calls share the engine's scratch buffer and are ordered by the library), and within the bound"""
    torch = torch_mod()
    k, v = _prompt()
    q = _query(4)
    with _batch(torch, _ragged()) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", 2)                            # partials in the shared scratch buffer: the ordering matters
            alone = [_entry(torch, lib, conn, RIDS, q, layer) for layer in range(L)]
            dq = torch.from_numpy(q).cuda()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            torch.cuda.synchronize()
            runs = [_prepare(torch, conn, RIDS, dq, layer, on=streams[layer]) for layer in range(L)]
            for args, *_ in runs:
                lib.attend_kv_batch(**args)
            for s in streams:
                s.synchronize()
        finally:
            set_tuning("attend_tiles_per_split", 0)
        for layer, (_, out, lse, _, _) in enumerate(runs):
            out, lse = out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)
            assert np.array_equal(out.view(np.uint32), alone[layer][0].view(np.uint32)) and np.array_equal(lse.view(np.uint32), alone[layer][1].view(np.uint32)), layer
            worst = _check(_checker(oracle, "prompt", k, v, layer), out, lse, q, LENGTHS, ("streams", layer))
            print(f"attend_kv_batch two streams layer {layer}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- the example
def test_the_example_runs():
    """examples/k8v4_decode_example.py in this process, short: three requests of odd and even lengths, three decode steps, every attend
    checked inside the example against float64"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "k8v4_decode_example.py")
    spec = importlib.util.spec_from_file_location("k8v4_decode_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(steps=3, verbose=False) == 3
