"""-m gpu: the split pool's life cycle -- speckv_ext_read_pairs_kv (k_read_pairs_kv) and speckv_ext_copy_runs_kv (k_copy_records_kv), one
launch over a request's FP8_E4M3 and MXFP4 allocations each, and SpeckvSplitKVConnector.truncate / fork / commit(nodes=path) on top.

Bit-for-bit checks are against speckv_ext_fetch_range (kv_rows) on either allocation.  Attention is checked against numpy float64 softmax
attention over what the pool and the tails hold: stored K as the FP8 records (HeadChecker(oracle, FP8) over the rows that were written),
stored V as the MXFP4 records, a tail and a step's new rows as fp16; the query enters a stored part as E4M3 x a row scale where the decode
kernel reads it (attend, attend_spec, the own part of attend_shared) and as fp16 elsewhere (attend_chunk, the prefix fold).  Bound: the one
tests/test_gpu_k8v4_decode.py and tests/test_gpu_k8v4_spec.py hold -- |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6 with delta = 3e-5 max sum
|q||k| sm over the positions of a (member, head).  A row read back by truncate / fork enters the reference as the fp16 row the pool decoded,
and a pair it is committed into afterwards as the oracle's records of (that row, its new partner): the float64 shadow of the rows as the
formats decode them.

Geometry: 2 layers (4 where two layer strides must differ from one), 8 kv heads x 128, max_tokens 128; lengths out of 0, 1, 2, 31, 32, 33,
34, 63, 64, 65 -- even and odd, both sides of the 16-record MXFP4 storage tile and of the 32-position kernel tile."""
import contextlib
import os
import zlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_k8v4_decode as kd
from tests._gpu import D, H, torch_mod

pytestmark = pytest.mark.gpu
L, T, SM = 2, 128, kd.SM
REGION = T // 2
LAYER = H * D * 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, GENERAL = -4, -1
TREE = [-1, 0, 0, 1, 1, 2]                                       # node 0, two children, three grandchildren

_data = {}


def _content(tag, n=T, layers=L, scale=1.0):
    """K, V [layers][n][H][D] fp16 of a tag, made once"""
    key = (tag, n, layers, scale)
    if key not in _data:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        _data[key] = tuple((rng.standard_normal((layers, n, H, D)) * scale).astype(np.float16) for _ in range(2))
    return _data[key]


def _rng(seed):
    return np.random.default_rng(seed)


@contextlib.contextmanager
def _pool(torch, layers=L):
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        yield lib, SpeckvSplitKVConnector(lib, layers, H, D, T)
        torch.cuda.synchronize()
    finally:
        lib.finalize()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fill(torch, conn, rid, k, v):
    """a new request holding the rows k, v [layers][n][H][D]"""
    conn.add_request(rid)
    if k.shape[1]:
        conn.write_prefill(rid, _dev(torch, k), _dev(torch, v))
        torch.cuda.synchronize()


def _stored(torch, conn, rid):
    """everything kv_rows gives for a request, tail included: uint16 [layers][2][length][H][D]"""
    n = conn.length(rid)
    out = np.zeros((conn.L, 2, n, H, D), np.uint16)
    for layer in range(conn.L):
        for kind in (0, 1):
            out[layer, kind] = conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16)
    torch.cuda.synchronize()
    return out


def _tail(conn, rid):
    r = conn.requests[rid]
    return None if r.tail_k is None else (r.tail_k.cpu().numpy(), r.tail_v.cpu().numpy())


# ----------------------------------------------------------------------------- the float64 reference
class _Member:
    """What one member's query rows see.  stored: [(pair or None, lo, hi, "e4m3" | "fp16")] -- positions [lo, hi) of the content a pair of
    HeadCheckers was made of, and how the query enters; held_k / held_v [P][H][D] fp16 or None; seen[r] = the held positions row r sees."""
    def __init__(self, stored, held_k=None, held_v=None, seen=None):
        self.stored, self.held_k, self.held_v, self.seen = [s for s in stored if s[2] > s[1]], held_k, held_v, seen


def _hold(member, q, got, what):
    """q [H][G][D] fp16, got [H][G][D] fp32 of one member against float64 under the bound of the module docstring -> worst err / tol"""
    G = q.shape[1]
    worst = 0.0
    for head in range(H):
        qf = q[head].astype(np.float64)
        scores, sums, values = [], [], []
        for pair, lo, hi, mode in member.stored:
            K, V = pair[0].kv(head)[0][lo:hi], pair[1].kv(head)[1][lo:hi]
            qq = pair[0].q_rows(q[head]).reshape(G, D) if mode == "e4m3" else qf
            scores.append((qq @ K.T) * SM); sums.append((np.abs(qq) @ np.abs(K).T) * SM); values.append(V)
        P = 0 if member.held_k is None else len(member.held_k)
        if P:
            kf, vf = member.held_k[:, head].astype(np.float64), member.held_v[:, head].astype(np.float64)
            hs, ha = (qf @ kf.T) * SM, (np.abs(qf) @ np.abs(kf).T) * SM
        n_stored = sum(s.shape[1] for s in scores)
        for r in range(G):
            seen = list(member.seen[r]) if P else []
            if n_stored == 0 and not seen:
                assert not got[head, r].any(), (what, head, r, "a row that sees nothing is exactly 0")
                continue
            s = np.concatenate([x[r] for x in scores] + ([hs[r, seen]] if seen else []))
            vals = np.concatenate(values + ([vf[seen]] if seen else []))
            mags = np.concatenate([x[r] for x in sums] + ([ha[r, seen]] if seen else []))
            delta = 3e-5 * float(mags.max())
            p = np.exp(s - s.max())
            want, mag = (p @ vals) / p.sum(), (p @ np.abs(vals)) / p.sum()
            err, tol = np.abs(got[head, r].astype(np.float64) - want), (2e-3 + 2 * delta) * mag + 1e-6
            worst = max(worst, float(np.nan_to_num(err / tol, nan=np.inf).max()))
            assert np.all(err <= tol), (what, head, r, float(np.nan_to_num(err / tol, nan=np.inf).max()), n_stored, seen)
    return worst


def _pair(oracle, tag, k, v, layer):
    """the HeadCheckers over the stored (even) part of rows k, v [L][n][H][D]; None when nothing is stored"""
    return kd._checker(oracle, ("lifecycle", tag), k, v, layer) if k.shape[1] >= 2 else None


def _decode_members(pairs, lengths, tails, layer, window=None):
    """members of an attend() call: the stored positions through the E4M3 query, from the window's bound on, and the tail"""
    out = []
    for pair, n, tail in zip(pairs, lengths, tails):
        lo = max(0, n - window) if window else 0
        held = (None, None, None) if tail is None else (tail[0][layer][None], tail[1][layer][None], None)
        out.append(_Member([(pair, lo, n & ~1, "e4m3")], held[0], held[1]))
    return out


def _attend_all(torch, oracle, conn, rids, pairs_of, lengths, tails, what, g=4, window=None):
    """attend over every layer against the reference; pairs_of(layer) -> one pair per member"""
    q = kd._rows(_rng(len(what) + 11 * g), len(rids), H, g, D)
    worst = 0.0
    for layer in range(L):
        got = conn.attend(layer, rids, _dev(torch, q), SM, window=window).cpu().numpy()
        for m, member in enumerate(_decode_members(pairs_of(layer), lengths, tails, layer, window)):
            member.seen = [[0]] * g
            worst = max(worst, _hold(member, q[m], got[m], f"{what} layer {layer} member {m} length {lengths[m]}"))
    print(f"{what}: worst err / tol {worst:.3f}")
    return worst


def _step_rows(q5):
    """[S][H][R][D] of one member -> [H][S * R][D]"""
    S, _, R, _ = q5.shape
    return np.ascontiguousarray(q5.transpose(1, 0, 2, 3).reshape(H, S * R, D))


def _step_member(pair, n, tail, layer, k_new, v_new, parents, R, mode):
    """a member of a draft step (k_new, v_new [S][L][H][D]): the stored part, then tail and new rows as held positions; node j sees the
    tail, its ancestors and itself"""
    S = k_new.shape[0]
    base = 0 if tail is None else 1
    hk = np.concatenate(([tail[0][layer][None]] if base else []) + [k_new[:, layer]])
    hv = np.concatenate(([tail[1][layer][None]] if base else []) + [v_new[:, layer]])
    seen = []
    for j in range(S):
        chain, up = [], j
        while up >= 0:
            chain.append(base + up)
            up = parents[up]
        seen += [sorted(([0] if base else []) + chain)] * R
    return _Member([(pair, 0, n & ~1, mode)], hk, hv, seen)


# ----------------------------------------------------------------------------- 1. read_pairs_kv is fetch_range, bit for bit
@pytest.mark.parametrize("stride", [LAYER, LAYER + 512])
def test_read_pairs_kv_is_fetch_range_bit_for_bit(stride):
    """pairs of three requests, four layers, both rows / even only / odd only / neither wanted per kind; every byte of the destination
    that is not a wanted row keeps its canary, the gaps of the wider layer stride included"""
    torch = torch_mod()
    layers = 4
    with _pool(torch, layers) as (lib, conn):
        lengths = {0: 64, 1: 34, 2: 66}
        for rid, n in lengths.items():
            _fill(torch, conn, rid, *(x[:, :n] for x in _content(("read", rid), layers=layers)))
        whole = {}
        for rid in lengths:                                              # every page of both allocations through fetch_range
            r = conn.requests[rid]
            for kind, h in enumerate((r.k_handle, r.v_handle)):
                out = torch.empty((layers * REGION, 2, H * D), dtype=torch.float16, device="cuda")
                lib.fetch_range(h, 0, layers * REGION, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                whole[(rid, kind)] = out.cpu().numpy().view(np.uint16)
        # (request, page of layer 0, wanted halves of K, of V); page 16 of request 1 is its last written one, page 40 was never written
        pairs = [(0, 0, (1, 1), (1, 1)), (0, 15, (1, 0), (0, 1)), (1, 16, (0, 1), (1, 0)), (2, 32, (1, 0), (1, 0)), (2, 17, (0, 0), (1, 1)),
                 (1, 3, (1, 1), (0, 0)), (0, 31, (0, 0), (0, 0)), (2, 40, (1, 1), (1, 1)), (0, 16, (1, 1), (1, 1))]
        room = layers * stride + 256                                     # a row block and its guard bytes
        buf = torch.full((len(pairs) * 4 * room,), 0xA5, dtype=torch.uint8, device="cuda")
        want = np.full(len(pairs) * 4 * room, 0xA5, np.uint8)
        rows = np.zeros((len(pairs), 4), np.uint64)
        for i, (rid, page, wk, wv) in enumerate(pairs):
            for kind, wanted in enumerate((wk, wv)):
                for half in (0, 1):
                    if not wanted[half]:
                        continue
                    at = ((i * 4) + 2 * kind + half) * room + 128
                    assert (buf.data_ptr() + at) % 16 == 0
                    rows[i, 2 * kind + half] = buf.data_ptr() + at
                    for layer in range(layers):
                        want[at + layer * stride:at + layer * stride + 2048] = whole[(rid, kind)][layer * REGION + page, half].view(np.uint8)
        reqs = [conn.requests[rid] for rid, *_ in pairs]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        lib.read_pairs_kv(np.asarray([r.k_handle for r in reqs], np.uint64), np.asarray([r.v_handle for r in reqs], np.uint64),
                          np.asarray([p for _, p, *_ in pairs], np.uint64), rows, REGION, layers, stride, st.cuda_stream)
        st.synchronize()
        got = buf.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (len(bad), bad[:4] // room, bad[:4] % room)
        assert want[want != 0xA5].size > 0 and np.any(whole[(2, 1)][32])     # the rows are not all canary or zero


# ----------------------------------------------------------------------------- 2. copy_runs_kv copies records
def test_fork_copies_records_and_attends_as_its_source():
    """lengths on both sides of page 16 and of the tile, one source forked twice, one pair without a page: kv_rows of both kinds and every
    layer are the source's bits, and attend over the forks is attend over the sources bit for bit (the scale table and the code plane)"""
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        lengths = [64, 31, 32, 33, 34, 2, 0, 65]
        for rid, n in enumerate(lengths):
            _fill(torch, conn, rid, *(x[:, :n] for x in _content(("fork", rid))))
        src = list(range(len(lengths))) + [0]                            # request 0 twice in one call
        new = list(range(100, 100 + len(src)))
        before = lib.stats().copied_pages
        conn.fork(src, new)
        torch.cuda.synchronize()
        assert lib.stats().copied_pages - before == sum(2 * L * (lengths[s] // 2) for s in src)
        for s, rid in zip(src, new):
            assert conn.length(rid) == lengths[s]
            assert np.array_equal(_stored(torch, conn, rid), _stored(torch, conn, s)), (s, rid)
        q = _dev(torch, kd._rows(_rng(5), len(src), H, 4, D))
        for layer in range(L):
            for window in (None, 40):
                a, b = conn.attend(layer, src, q, SM, window=window), conn.attend(layer, new, q, SM, window=window)
                assert torch.equal(a, b), (layer, window)
        assert bool(conn.attend(0, [100], q[:1], SM).abs().sum() > 0)


def test_never_written_source_pages_zero_a_longer_destination():
    """32 pages per region copied from a source that has written 17 of them over a destination that holds 32: the destination's pages
    17 .. 31 read as never written afterwards, in both allocations, and both attend alike"""
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        _fill(torch, conn, 0, *(x[:, :34] for x in _content(("short", 0))))
        _fill(torch, conn, 1, *(x[:, :64] for x in _content(("long", 1))))
        s, d = conn.requests[0], conn.requests[1]
        u64 = lambda *v: np.asarray(v, np.uint64)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        lib.copy_runs_kv(u64(s.k_handle), u64(s.v_handle), u64(d.k_handle), u64(d.v_handle), u64(32), u64(*(l * REGION for l in range(L))), st.cuda_stream)
        st.synchronize()
        s.length = d.length = 64                                         # look at all 32 pages of either
        conn._moved()
        a, b = _stored(torch, conn, 0), _stored(torch, conn, 1)
        assert np.array_equal(a, b) and not b[:, :, 34:].any() and b[:, :, :34].any()
        q = _dev(torch, kd._rows(_rng(6), 2, H, 4, D))
        for layer in range(L):
            out = conn.attend(layer, [0, 1], q[:1].expand(2, H, 4, D), SM)
            assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out).all())


# ----------------------------------------------------------------------------- 3. refusals launch nothing
def test_refusals_launch_nothing():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        for rid in range(4):
            _fill(torch, conn, rid, *(x[:, :64] for x in _content(("refuse", rid))))
        r = [conn.requests[rid] for rid in range(4)]
        u64 = lambda *v: np.asarray(v, np.uint64)
        firsts = u64(*(l * REGION for l in range(L)))
        st = torch.cuda.Stream()
        before = {rid: _stored(torch, conn, rid) for rid in range(4)}
        copied = lib.stats().copied_pages
        k, v = (lambda i: r[i].k_handle), (lambda i: r[i].v_handle)
        cases = [("a K handle that is MXFP4", (u64(v(0)), u64(k(0)), u64(k(1)), u64(v(1)), u64(4), firsts, st.cuda_stream), INVAL),
                 ("a V destination that is FP8", (u64(k(0)), u64(v(0)), u64(k(1)), u64(k(2)), u64(4), firsts, st.cuda_stream), INVAL),
                 ("source == destination", (u64(k(0)), u64(v(0)), u64(k(0)), u64(v(1)), u64(4), firsts, st.cuda_stream), INVAL),
                 ("a destination on both sides", (u64(k(0)), u64(v(0)), u64(k(1)), u64(k(1)), u64(4), firsts, st.cuda_stream), INVAL),
                 ("a destination named twice", (u64(k(0), k(2)), u64(v(0), v(2)), u64(k(1), k(1)), u64(v(1), v(3)), u64(4, 4), firsts, st.cuda_stream), INVAL),
                 ("a destination that is a source", (u64(k(0), k(1)), u64(v(0), v(1)), u64(k(1), k(2)), u64(v(1), v(2)), u64(4, 4), firsts, st.cuda_stream), INVAL),
                 ("runs that overlap", (u64(k(0)), u64(v(0)), u64(k(1)), u64(v(1)), u64(4), u64(0, 2), st.cuda_stream), INVAL),
                 ("pages beyond the allocation", (u64(k(0)), u64(v(0)), u64(k(1)), u64(v(1)), u64(4), u64(0, L * REGION - 2), st.cuda_stream), GENERAL),
                 ("an unknown handle", (u64(k(0)), u64(v(0)), u64(k(1)), u64(0xDEAD), u64(4), firsts, st.cuda_stream), GENERAL),
                 ("a null stream", (u64(k(0)), u64(v(0)), u64(k(1)), u64(v(1)), u64(4), firsts, 0), INVAL)]
        for what, args, status in cases:
            with pytest.raises(SpeckvError) as e:
                lib.copy_runs_kv(*args)
            assert e.value.status == status, (what, e.value.status)
        torch.cuda.synchronize()
        assert lib.stats().copied_pages == copied
        for rid in range(4):
            assert np.array_equal(_stored(torch, conn, rid), before[rid]), rid          # every destination bytewise unchanged
        # the read: nothing is written into the rows
        buf = torch.full((4 * L * LAYER + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        at = buf.data_ptr() + (-buf.data_ptr()) % 16
        rows = u64(at, at + L * LAYER, at + 2 * L * LAYER, at + 3 * L * LAYER).reshape(1, 4)
        odd = rows.copy(); odd[0, 1] += 8
        done = lib.stats().total_decompressions
        for what, args, status in [("a K handle that is MXFP4", (u64(v(0)), u64(k(0)), u64(0), rows, REGION, L, LAYER, st.cuda_stream), INVAL),
                                   ("a V handle that is FP8", (u64(k(0)), u64(k(1)), u64(0), rows, REGION, L, LAYER, st.cuda_stream), INVAL),
                                   ("a row that is not aligned", (u64(k(0)), u64(v(0)), u64(0), odd, REGION, L, LAYER, st.cuda_stream), INVAL),
                                   ("a layer stride that is not", (u64(k(0)), u64(v(0)), u64(0), rows, REGION, L, LAYER + 8, st.cuda_stream), INVAL),
                                   ("a page step of 0", (u64(k(0)), u64(v(0)), u64(0), rows, 0, L, LAYER, st.cuda_stream), INVAL),
                                   ("pages beyond the allocation", (u64(k(0)), u64(v(0)), u64(REGION), rows, REGION, L, LAYER, st.cuda_stream), GENERAL),
                                   ("an unknown handle", (u64(0xDEAD), u64(v(0)), u64(0), rows, REGION, L, LAYER, st.cuda_stream), GENERAL),
                                   ("a null stream", (u64(k(0)), u64(v(0)), u64(0), rows, REGION, L, LAYER, 0), INVAL)]:
            with pytest.raises(SpeckvError) as e:
                lib.read_pairs_kv(*args)
            assert e.value.status == status, (what, e.value.status)
        torch.cuda.synchronize()
        assert lib.stats().total_decompressions == done and bool((buf == 0x5A).all())
        lib.read_pairs_kv(u64(k(0)), u64(v(0)), u64(0), rows, REGION, 0, LAYER, st.cuda_stream)           # nothing to do: SPECKV_OK
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all())
        lib.copy_runs_kv(u64(k(0)), u64(v(0)), u64(k(1)), u64(v(1)), u64(0), firsts, st.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(_stored(torch, conn, 1), before[1])


# ----------------------------------------------------------------------------- 4. truncate leaves the state of a connector that stopped there
CUTS = [(65, 33), (64, 31), (34, 34), (33, 32), (63, 1), (2, 1), (32, 0), (65, 63), (34, 33), (64, 2)]


def test_truncate_leaves_the_state_of_a_connector_that_stopped_there(oracle):
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        rids = list(range(len(CUTS)))
        k, v = _content("cut")
        for rid, (n, _) in zip(rids, CUTS):
            _fill(torch, conn, rid, k[:, :n], v[:, :n])
        new = [n for _, n in CUTS]
        rows = {rid: _stored(torch, conn, rid) for rid in rids}
        conn.truncate(rids, new)
        torch.cuda.synchronize()
        tails = []
        for rid, (n0, n) in zip(rids, CUTS):
            assert conn.length(rid) == n
            tail = _tail(conn, rid)
            tails.append(tail)
            assert (tail is not None) == bool(n & 1)
            if tail is not None and n != n0:                             # the decoded stored row, bit for bit
                for kind in (0, 1):
                    assert np.array_equal(tail[kind].view(np.uint16), rows[rid][:, kind, n - 1]), (rid, kind)
            assert np.array_equal(_stored(torch, conn, rid), rows[rid][:, :, :n]), rid
        pairs_of = lambda layer: [_pair(oracle, "cut", k, v, layer)] * len(rids)     # every member is a prefix of one prompt
        _attend_all(torch, oracle, conn, rids, pairs_of, new, tails, "attend after truncate")
        _attend_all(torch, oracle, conn, rids, pairs_of, new, tails, "attend(window=20) after truncate", g=1, window=20)
        S, R = 3, 4
        rng = _rng(44)
        q5, k_new, v_new = kd._rows(rng, len(rids), S, H, R, D), kd._rows(rng, len(rids), S, L, H, D), kd._rows(rng, len(rids), S, L, H, D)
        worst = 0.0
        for layer in range(L):
            got = conn.attend_spec(layer, rids, _dev(torch, q5), _dev(torch, k_new), _dev(torch, v_new), SM).cpu().numpy()
            for m in range(len(rids)):
                member = _step_member(pairs_of(layer)[m], new[m], tails[m], layer, k_new[m], v_new[m], list(range(-1, S - 1)), R, "e4m3")
                worst = max(worst, _hold(member, _step_rows(q5[m]), _step_rows(got[m]), f"attend_spec after truncate layer {layer} member {m}"))
        print(f"attend_spec after truncate: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- 5. stale records behind the cut
@pytest.mark.parametrize("factor", [200.0, 1000.0])
def test_stale_records_behind_the_cut_are_never_seen(oracle, factor):
    """rows of `factor` times the kept magnitude are committed behind the kept positions and cut off again: attend, attend(window=W),
    attend_spec, attend_chunk and attend_shared over a cut prefix hold the bound of a pool that never saw them"""
    torch = torch_mod()
    kept = [65, 64, 33, 32, 31, 34, 2, 1, 0, 63]
    S = 5
    with _pool(torch) as (lib, conn):
        rids = list(range(len(kept)))
        k, v = _content("kept")
        for rid, n in zip(rids, kept):
            _fill(torch, conn, rid, k[:, :n], v[:, :n])
        hk, hv = _content(("hostile", factor), n=len(kept) * S, scale=factor)
        hostile = lambda x: _dev(torch, np.ascontiguousarray(x.reshape(L, len(kept), S, H, D).transpose(1, 2, 0, 3, 4)))
        conn.commit(rids, hostile(hk), hostile(hv), [S] * len(kept))
        torch.cuda.synchronize()
        assert [conn.length(r) for r in rids] == [n + S for n in kept]
        conn.truncate(rids, kept)
        torch.cuda.synchronize()
        tails = [_tail(conn, rid) for rid in rids]
        for n, tail in zip(kept, tails):
            # an odd kept position shared its page with a hostile row: it comes back through that page's formats, far from what it was,
            # but of the kept magnitude -- the reference takes it as it is
            assert (tail is not None) == bool(n & 1) and (tail is None or float(np.abs(tail[0].astype(np.float32)).max()) < 16.0)
        # what the pool holds in front of the cut: the kept prefix's even part (a page is rewritten whole or not at all)
        pairs_of = lambda layer: [_pair(oracle, "kept", k, v, layer)] * len(rids)
        _attend_all(torch, oracle, conn, rids, pairs_of, kept, tails, f"attend x{factor:g}")
        _attend_all(torch, oracle, conn, rids, pairs_of, kept, tails, f"attend(window=24) x{factor:g}", g=2, window=24)
        R = 2
        rng = _rng(int(factor))
        q5, k_new, v_new = kd._rows(rng, len(rids), 3, H, R, D), kd._rows(rng, len(rids), 3, L, H, D), kd._rows(rng, len(rids), 3, L, H, D)
        dq, dk, dv = _dev(torch, q5), _dev(torch, k_new), _dev(torch, v_new)
        for name, mode in (("attend_spec", "e4m3"), ("attend_chunk", "fp16")):
            worst = 0.0
            for layer in range(L):
                got = getattr(conn, name)(layer, rids, dq, dk, dv, SM).cpu().numpy()
                for m in range(len(rids)):
                    member = _step_member(pairs_of(layer)[m], kept[m], tails[m], layer, k_new[m], v_new[m], [-1, 0, 1], R, mode)
                    worst = max(worst, _hold(member, _step_rows(q5[m]), _step_rows(got[m]), f"{name} x{factor:g} layer {layer} member {m}"))
            print(f"{name} x{factor:g}: worst err / tol {worst:.3f}")
        # a cut prefix: requests 1 (64 kept) and 3 (32 kept) as the prefixes of fresh members that hold a little of their own
        mk, mv = _content("members")
        members, own = [200, 201, 202], [3, 0, 34]
        for rid, n in zip(members, own):
            _fill(torch, conn, rid, mk[:, :n], mv[:, :n])
        prefixes = [1, 3, 1]
        q = kd._rows(rng, len(members), H, 4, D)
        worst = 0.0
        for layer in range(L):
            got = conn.attend_shared(layer, members, prefixes, _dev(torch, q), SM).cpu().numpy()
            for m, (rid, n, p) in enumerate(zip(members, own, prefixes)):
                tail = _tail(conn, rid)
                member = _Member([(pairs_of(layer)[0], 0, kept[p], "fp16"), (_pair(oracle, "members", mk, mv, layer), 0, n & ~1, "e4m3")],
                                 None if tail is None else tail[0][layer][None], None if tail is None else tail[1][layer][None], [[0]] * 4)
                worst = max(worst, _hold(member, q[m], got[m], f"attend_shared x{factor:g} layer {layer} member {m}"))
        print(f"attend_shared x{factor:g}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- 6. rollback, then go on
def test_rollback_then_a_tree_step_a_path_commit_and_decode(oracle):
    """truncate to an odd and to an even length, verify a draft tree, commit the accepted path, decode: every step against the float64
    shadow of the rows as the formats decode them"""
    torch = torch_mod()
    start, cut = [64, 65, 34, 33], [33, 32, 31, 2]
    paths = [[0, 2, 5], [0, 1], [0, 1, 4], [0]]
    R = 2
    S = len(TREE)
    with _pool(torch) as (lib, conn):
        rids = list(range(len(start)))
        k, v = _content("roll")
        for rid, n in zip(rids, start):
            _fill(torch, conn, rid, k[:, :n], v[:, :n])
        conn.truncate(rids, cut)
        torch.cuda.synchronize()
        # the shadow: per member the fp16 rows the encoder was given for every position -- prompt rows, and for an odd cut the DECODED row
        shadow = []
        for rid, n in zip(rids, cut):
            sk, sv = k[:, :n].copy(), v[:, :n].copy()
            if n & 1:
                sk[:, n - 1], sv[:, n - 1] = _tail(conn, rid)
            shadow.append([sk, sv])
        tails = [_tail(conn, rid) for rid in rids]
        rng = _rng(66)
        q5, k_new, v_new = kd._rows(rng, len(rids), S, H, R, D), kd._rows(rng, len(rids), S, L, H, D), kd._rows(rng, len(rids), S, L, H, D)
        dk, dv = _dev(torch, k_new), _dev(torch, v_new)
        worst = 0.0
        for layer in range(L):
            got = conn.attend_spec(layer, rids, _dev(torch, q5), dk, dv, SM, parents=TREE).cpu().numpy()
            for m in range(len(rids)):
                pair = _pair(oracle, ("roll", m, "cut"), shadow[m][0], shadow[m][1], layer)
                member = _step_member(pair, cut[m], tails[m], layer, k_new[m], v_new[m], TREE, R, "e4m3")
                worst = max(worst, _hold(member, _step_rows(q5[m]), _step_rows(got[m]), f"tree step layer {layer} member {m} length {cut[m]}"))
        print(f"tree step after rollback: worst err / tol {worst:.3f}")
        keep = conn.commit(rids, dk, dv, nodes=paths, parents=TREE)
        torch.cuda.synchronize()
        del keep
        lengths = [n + len(p) for n, p in zip(cut, paths)]
        assert [conn.length(r) for r in rids] == lengths
        for m, path in enumerate(paths):
            gather = lambda x: np.ascontiguousarray(x[m][path].transpose(1, 0, 2, 3))         # [L][len(path)][H][D]
            shadow[m] = [np.concatenate([shadow[m][0], gather(k_new)], axis=1), np.concatenate([shadow[m][1], gather(v_new)], axis=1)]
        tails = [_tail(conn, rid) for rid in rids]
        for m, n in enumerate(lengths):                                  # a new tail is the path's last row as it was given
            if n & 1:
                assert np.array_equal(tails[m][0], shadow[m][0][:, n - 1]) and np.array_equal(tails[m][1], shadow[m][1][:, n - 1])
        pairs_of = lambda layer: [_pair(oracle, ("roll", m, "after"), shadow[m][0], shadow[m][1], layer) for m in range(len(rids))]
        _attend_all(torch, oracle, conn, rids, pairs_of, lengths, tails, "decode after the path commit", g=8)


# ----------------------------------------------------------------------------- 7. commit(nodes=path) is commit(n_accept) of the gathered rows
def test_commit_of_a_path_stores_what_commit_of_the_gathered_rows_stores():
    torch = torch_mod()
    before = [33, 34, 0, 1, 63, 64]
    paths = [[0, 2, 5], [0, 1, 4], [0, 1, 3], [], [0, 2], [0]]
    S = len(TREE)
    with _pool(torch) as (lib, conn):
        k, v = _content("path")
        a, b = list(range(len(before))), list(range(50, 50 + len(before)))
        for rids in (a, b):
            for rid, n in zip(rids, before):
                _fill(torch, conn, rid, k[:, :n], v[:, :n])
        rng = _rng(77)
        k_new, v_new = kd._rows(rng, len(a), S, L, H, D), kd._rows(rng, len(a), S, L, H, D)
        longest = max(len(p) for p in paths)
        k_path, v_path = np.zeros((len(a), longest, L, H, D), np.float16), np.zeros((len(a), longest, L, H, D), np.float16)
        for m, path in enumerate(paths):
            k_path[m, :len(path)], v_path[m, :len(path)] = k_new[m][path], v_new[m][path]
        dk, dv = _dev(torch, k_new), _dev(torch, v_new)
        keep = conn.commit(a, dk, dv, nodes=paths, parents=TREE)
        keep += conn.commit(b, _dev(torch, k_path), _dev(torch, v_path), [len(p) for p in paths])
        torch.cuda.synchronize()
        for ra, rb, n, path in zip(a, b, before, paths):
            assert conn.length(ra) == conn.length(rb) == n + len(path)
            assert np.array_equal(_stored(torch, conn, ra), _stored(torch, conn, rb)), ra       # records and tails, bit for bit
            ta, tb = _tail(conn, ra), _tail(conn, rb)
            assert (ta is None) == (tb is None) and (ta is None or (np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])))
        # a path that is no chain of the tree raises and changes nothing
        state = [_stored(torch, conn, r) for r in a]
        epoch = conn._epoch
        for nodes, parents in (([[0, 3]] + [[]] * 5, TREE), ([[1]] + [[]] * 5, TREE), ([[0, S]] + [[]] * 5, None), ([[2, 1]] + [[]] * 5, None)):
            with pytest.raises(ValueError):
                conn.commit(a, dk, dv, nodes=nodes, parents=parents)
        torch.cuda.synchronize()
        assert conn._epoch == epoch
        for r, was in zip(a, state):
            assert np.array_equal(_stored(torch, conn, r), was)


# ----------------------------------------------------------------------------- 8. fork semantics
def test_source_and_fork_go_their_own_ways_and_fork_to_a_length_is_fork_and_truncate():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        lengths = [65, 64, 33, 34]
        for rid, n in enumerate(lengths):
            _fill(torch, conn, rid, *(x[:, :n] for x in _content(("own", rid))))
        src = [0, 1, 2, 3]
        conn.fork(src, [10, 11, 12, 13])
        torch.cuda.synchronize()
        rng = _rng(88)
        ka, va, kb, vb = (_dev(torch, kd._rows(rng, 4, 2, L, H, D)) for _ in range(4))
        conn.commit(src, ka, va, [2, 1, 2, 1])
        conn.commit([10, 11, 12, 13], kb, vb, [1, 2, 1, 2])
        torch.cuda.synchronize()
        for s, f, n, (na, nb) in zip(src, [10, 11, 12, 13], lengths, [(2, 1), (1, 2), (2, 1), (1, 2)]):
            assert conn.length(s) == n + na and conn.length(f) == n + nb
            x, y = _stored(torch, conn, s), _stored(torch, conn, f)
            common = n & ~1                                              # pairs stored before the fork stay equal, what came after differs
            assert np.array_equal(x[:, :, :common], y[:, :, :common]) and not np.array_equal(x[:, :, common:n + 1], y[:, :, common:n + 1])
        # fork(lengths=n) is fork() + truncate(n): rows and tails, for every kind of cut
        cuts = [33, 31, 32, 1]
        conn.fork(src, [20, 21, 22, 23], cuts)
        conn.fork(src, [30, 31, 32, 33])
        conn.truncate([30, 31, 32, 33], cuts)
        torch.cuda.synchronize()
        for x, y, n in zip([20, 21, 22, 23], [30, 31, 32, 33], cuts):
            assert conn.length(x) == conn.length(y) == n
            assert np.array_equal(_stored(torch, conn, x), _stored(torch, conn, y)), (x, y)
            tx, ty = _tail(conn, x), _tail(conn, y)
            assert (tx is None) == (ty is None) == (not n & 1)
            assert tx is None or (np.array_equal(tx[0].view(np.uint16), ty[0].view(np.uint16)) and np.array_equal(tx[1].view(np.uint16), ty[1].view(np.uint16)))
        with pytest.raises(KeyError):
            conn.fork([0], [20])
        with pytest.raises(ValueError):
            conn.fork([0], [40], [conn.length(0) + 1])
        assert 40 not in conn.requests


def test_a_fork_follows_a_commit_on_the_same_stream_without_a_host_sync():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        k, v = _content("stream")
        lengths = [33, 64, 2]
        for rid, n in enumerate(lengths):
            _fill(torch, conn, rid, k[:, :n], v[:, :n])
        rng = _rng(99)
        dk, dv = _dev(torch, kd._rows(rng, 3, 4, L, H, D)), _dev(torch, kd._rows(rng, 3, 4, L, H, D))
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        keep = conn.commit([0, 1, 2], dk, dv, [3, 4, 1], stream=st)
        keep += conn.fork([0, 1, 2, 0], [10, 11, 12, 13], [36, 67, 3, 35], stream=st)      # pairs and a row the commit has only just queued
        st.synchronize()
        for s, f, n in zip([0, 1, 2, 0], [10, 11, 12, 13], [36, 67, 3, 35]):
            assert conn.length(f) == n
            assert np.array_equal(_stored(torch, conn, f), _stored(torch, conn, s)[:, :, :n]), (s, f)


# ----------------------------------------------------------------------------- 9. launch counts
def test_one_launch_each():
    torch = torch_mod()
    with _pool(torch) as (lib, conn):
        k, v = _content("count")
        rids, lengths = [1, 2, 3, 4, 5, 6], [33, 33, 34, 64, 65, 2]
        for rid, n in zip(rids, lengths):
            _fill(torch, conn, rid, k[:, :n], v[:, :n])
        calls = []
        for name in ("read_pairs_kv", "copy_runs_kv", "read_pairs", "copy_runs"):
            def counted(first, *args, _inner=getattr(lib, name), _name=name):
                calls.append((_name, len(first)))
                return _inner(first, *args)
            setattr(lib, name, counted)
        conn.truncate(rids, [32, 31, 33, 64, 63, 1])                     # drop, read, read, nothing, read, read
        assert calls == [("read_pairs_kv", 4)]
        conn.truncate(rids, [30, 31, 32, 64, 62, 0])                     # even cuts and dropped tails only
        assert calls == [("read_pairs_kv", 4)]
        del calls[:]
        conn.fork(rids, [11, 12, 13, 14, 15, 16])                        # whole requests: a held tail is a clone, no row is read
        assert calls == [("copy_runs_kv", 6)]
        del calls[:]
        conn.fork(rids, [21, 22, 23, 24, 25, 26], [29, 31, 1, 64, 33, 0])
        assert calls == [("copy_runs_kv", 6), ("read_pairs_kv", 3)]       # 29, 1 and 33 are read from the sources; 31 is request 2's own tail
        del calls[:]
        conn.fork([6, 2], [31, 32], [0, 1])                              # nothing stored to copy; position 0 of request 2 is read
        assert calls == [("read_pairs_kv", 1)]
        torch.cuda.synchronize()
        assert not [c for c in calls if c[0] in ("read_pairs", "copy_runs")]


# ----------------------------------------------------------------------------- 10. the example
def test_the_example_runs():
    import importlib.util
    torch_mod()
    spec = importlib.util.spec_from_file_location("k8v4_fork_rollback_example", os.path.join(ROOT, "examples", "k8v4_fork_rollback_example.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(verbose=False) > 0
