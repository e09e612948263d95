"""-m gpu: the multi-position decode step -- speckv_ext_attend_fold_held (the positions a step holds outside the pool, folded
causally) and SpeckvKVConnector.attend_spec / append_tokens on top of it.  Every reference is numpy float64 in this file.

Tolerance of a fold, derived: the single-fold bound of tests/test_gpu_round2.py::test_fold_tail_adds_one_position (fp32 dot product
of 128 terms, v_exp / v_log: 2e-5 |want| + 2e-6 on out, 1e-5 max(1, |want|) on lse) times the number of positions folded into the
row -- a fold's weights are <= 1, so the errors of successive folds add at worst linearly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import HELD_MAX, SpeckvError, SpeckvLib
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = {"fp8": 4, "int4": 3, "mxfp4": 5}


def open_lib():
    return SpeckvLib(pkg.library_path(), "hip:0")


def chained_folds(out, lse, q, k, v, sm):
    """float64: rows out [G][D], lse [G], q [G][D] += the positions k / v [n][D] one after the other by the fold formula; also the
    magnitude sum p|v| carried along when `out` is a pair (out, mag)"""
    mag = None
    if isinstance(out, tuple):
        out, mag = out
        mag = np.array(mag, np.float64)
    out, lse = np.array(out, np.float64), np.array(lse, np.float64)
    for kt, vt in zip(np.asarray(k, np.float64), np.asarray(v, np.float64)):
        s = (np.asarray(q, np.float64) @ kt) * sm
        new = np.logaddexp(lse, s)
        w_old, w_new = np.exp(lse - new)[:, None], np.exp(s - new)[:, None]
        out = out * w_old + vt[None, :] * w_new
        if mag is not None:
            mag = mag * w_old + np.abs(vt)[None, :] * w_new
        lse = new
    return (out, lse) if mag is None else (out, lse, mag)


def want_fold_held(out, lse, q, kh, vh, base, n_live, rpp, sm, rows=None):
    """the definition of speckv_ext_attend_fold_held in float64.  out [n][H][g][D], lse [n][H][g], q likewise (fp16); kh / vh
    [m][P][H][D] fp16; base / n_live [m]; rows: the sequences the m held sets belong to.  Returns out, lse, folds [n][H][g]"""
    want_out, want_lse = out.astype(np.float64), lse.astype(np.float64)
    folds = np.zeros(lse.shape, np.int64)
    g = out.shape[2]
    for i in range(len(kh)):
        b = i if rows is None else rows[i]
        for j in range(min(g // rpp, int(n_live[i]))):
            n_vis = int(base[i]) + j + 1
            r0, r1 = j * rpp, (j + 1) * rpp
            for h in range(out.shape[1]):
                want_out[b, h, r0:r1], want_lse[b, h, r0:r1] = chained_folds(want_out[b, h, r0:r1], want_lse[b, h, r0:r1], q[b, h, r0:r1],
                                                                             kh[i, :n_vis, h], vh[i, :n_vis, h], sm)
            folds[b, :, r0:r1] = n_vis
    return want_out, want_lse, folds


def run_fold_held(lib, torch, q, out, lse, kh_buf, vh_buf, seq_stride, pos_stride, base, n_live, rpp, sm, rows=None, n_seq=None):
    d_q, d_out, d_lse = torch.from_numpy(q).cuda(), torch.from_numpy(out).cuda(), torch.from_numpy(lse).cuda()
    d_k, d_v = torch.from_numpy(kh_buf).cuda(), torch.from_numpy(vh_buf).cuda()
    d_base = torch.from_numpy(np.asarray(base, np.int32)).cuda()
    d_live = None if n_live is None else torch.from_numpy(np.asarray(n_live, np.int32)).cuda()
    d_rows = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lib.attend_fold_held(len(base) if n_seq is None else n_seq, 0 if rows is None else d_rows.data_ptr(), q.shape[1], q.shape[2], rpp, d_q.data_ptr(),
                         d_k.data_ptr(), d_v.data_ptr(), seq_stride, pos_stride, d_base.data_ptr(), 0 if d_live is None else d_live.data_ptr(), sm,
                         d_out.data_ptr(), d_lse.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_lse.cpu().numpy()


# rows_per_pos in {1, 4, 8} x query positions in {1, 2, 4, 16}: every pair that is a launch shape (at most 16 query rows per kv head)
SHAPES = [(rpp, n_q) for rpp in (1, 4, 8) for n_q in (1, 2, 4, 16) if rpp * n_q <= 16]


@pytest.mark.parametrize("base_kind", ["base0", "base1", "mixed"])
@pytest.mark.parametrize("rpp,n_q", SHAPES)
def test_fold_held_against_float64_chained_folds(rpp, n_q, base_kind):
    """The kernel against the fold formula applied once per visible position in float64: random incoming (out, lse), a sequence with
    nothing stored (out 0, lse -inf), scores far above and far below the stored lse, ragged live counts, a row subset through d_rows,
    strides larger than the rows need (one layer of [seq][pos][layers][heads][dim] with a gap behind every sequence).  Rows nobody
    may touch (sequences outside d_rows, positions past the live count) stay bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(1000 * rpp + 10 * n_q + len(base_kind))
        n_seq, G, Lyr, layer, sm = 7, rpp * n_q, 2, 1, 0.0884
        rows = [5, 0, 3, 6, 2]                                    # sequences 1 and 4 are not in the launch
        m = len(rows)
        base = {"base0": [0] * m, "base1": [1] * m, "mixed": [0, 1, 1, HELD_MAX - n_q, 0]}[base_kind]     # (the most the entry takes: 17 held positions)
        live = [n_q, n_q, max(n_q - 1, 1), n_q, 0]                # ragged: one sequence a position short, one without a live position
        P = HELD_MAX
        q = rng.standard_normal((n_seq, H, G, D)).astype(np.float16)
        q[3] *= 40.0                                              # scores far above the stored lse ...
        q[6] *= -40.0                                             # ... and far below (the sign flips with k: both occur)
        out = rng.standard_normal((n_seq, H, G, D)).astype(np.float32)
        lse = rng.uniform(-3, 9, (n_seq, H, G)).astype(np.float32)
        out[0] = 0.0; lse[0] = -np.inf                            # nothing stored
        pos_stride, seq_stride = Lyr * H * D, P * Lyr * H * D + 64
        kbuf = rng.standard_normal(m * seq_stride).astype(np.float16)
        vbuf = rng.standard_normal(m * seq_stride).astype(np.float16)
        view = lambda buf: np.stack([buf[i * seq_stride:i * seq_stride + P * pos_stride].reshape(P, Lyr, H, D)[:, layer] for i in range(m)])
        kh, vh = view(kbuf), view(vbuf)
        want_out, want_lse, folds = want_fold_held(out, lse, q, kh, vh, base, live, rpp, sm, rows)
        off = layer * H * D
        got_out, got_lse = run_fold_held(lib, torch, q, out, lse, kbuf[off:], vbuf[off:], seq_stride, pos_stride, base, live, rpp, sm, rows)
        touched = folds > 0
        err, lerr = np.abs(got_out - want_out), np.abs(got_lse - want_lse)
        tol = folds[..., None] * (2e-5 * np.abs(want_out) + 2e-6)
        ltol = folds * 1e-5 * np.maximum(1.0, np.abs(want_lse))
        print(f"fold_held rpp={rpp} n_q={n_q} {base_kind}: worst out err / tol {float((err[touched] / tol[touched]).max()):.3f}, "
              f"lse err / tol {float((lerr[touched] / ltol[touched]).max()):.3f}, most folds {int(folds.max())}")
        assert np.all(err[touched] <= tol[touched])
        assert np.all(lerr[touched] <= ltol[touched])
        assert np.array_equal(got_out[~touched], out[~touched]) and np.array_equal(got_lse[~touched], lse[~touched])
        assert not touched[1].any() and not touched[4].any() and not touched[2].any() and touched[0].all() and touched[6].all()
        # nothing stored: plain softmax attention over the visible held positions
        i0 = rows.index(0)
        for j in range(min(n_q, live[i0])):
            n_vis = base[i0] + j + 1
            s = np.einsum("hrd,thd->hrt", q[0, :, j * rpp:(j + 1) * rpp].astype(np.float64), kh[i0, :n_vis].astype(np.float64)) * sm
            p = np.exp(s - s.max(axis=-1, keepdims=True)); p /= p.sum(axis=-1, keepdims=True)
            plain = np.einsum("hrt,thd->hrd", p, vh[i0, :n_vis].astype(np.float64))
            assert np.all(np.abs(got_out[0, :, j * rpp:(j + 1) * rpp] - plain) <= n_vis * (2e-5 * np.abs(plain) + 2e-6))
    finally:
        lib.finalize()


def test_fold_held_refuses_bad_arguments_on_the_gpu():
    torch = torch_mod()
    lib = open_lib()
    try:
        buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
        p, s = buf.data_ptr(), torch.cuda.Stream().cuda_stream
        for heads, g, rpp, seq_stride, pos_stride, base, lse in ((8, 8, 3, 17408, 1024, p, p), (8, 32, 2, 17408, 1024, p, p), (8, 17, 1, 17408, 1024, p, p),
                                                                  (8, 8, 4, 17408, 1024, 0, p), (8, 8, 4, 17408, 1024, p, 0), (8, 8, 4, 17408, 1028, p, p),
                                                                  (8, 8, 4, 17408, 1016, p, p), (8, 8, 4, 1024, 1024, p, p)):
            with pytest.raises(SpeckvError) as e:
                lib.attend_fold_held(1, 0, heads, g, rpp, p, p, p, seq_stride, pos_stride, base, 0, 0.1, p, lse, s)
            assert e.value.status == -4
        torch.cuda.synchronize()
        assert float(buf.abs().max()) == 0.0
    finally:
        lib.finalize()


def test_fold_held_of_one_position_is_fold_tail():
    """base = 0, n_q = 1 is speckv_ext_attend_fold_tail: the two entries on the same buffers (those of
    tests/test_gpu_round2.py::test_fold_tail_adds_one_position) agree within the single-fold bound, and each meets it against float64"""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(131)
        n_seq, G, sm = 9, 5, 0.0884
        q = rng.standard_normal((n_seq, H, G, D)).astype(np.float16)
        q[3] *= 40.0; q[8] *= -40.0
        out = rng.standard_normal((n_seq, H, G, D)).astype(np.float32)
        lse = rng.uniform(-3, 9, (n_seq, H, G)).astype(np.float32)
        out[0] = 0.0; lse[0] = -np.inf
        kt = rng.standard_normal((n_seq, H, D)).astype(np.float16)
        vt = rng.standard_normal((n_seq, H, D)).astype(np.float16)
        want_out, want_lse, _ = want_fold_held(out, lse, q, kt[:, None], vt[:, None], [0] * n_seq, [1] * n_seq, G, sm)
        held_out, held_lse = run_fold_held(lib, torch, q, out, lse, kt.reshape(-1), vt.reshape(-1), H * D, H * D, [0] * n_seq, None, G, sm)
        d_q, d_out, d_lse = torch.from_numpy(q).cuda(), torch.from_numpy(out).cuda(), torch.from_numpy(lse).cuda()
        d_k, d_v = torch.from_numpy(kt).cuda(), torch.from_numpy(vt).cuda()
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        lib.attend_fold_tail(n_seq, 0, H, G, d_q.data_ptr(), d_k.data_ptr(), d_v.data_ptr(), H * D, sm, d_out.data_ptr(), d_lse.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        tail_out, tail_lse = d_out.cpu().numpy(), d_lse.cpu().numpy()
        tol, ltol = 2e-5 * np.abs(want_out) + 2e-6, 1e-5 * np.maximum(1.0, np.abs(want_lse))
        print(f"fold_held vs fold_tail: worst difference / tol {float((np.abs(held_out - tail_out) / tol).max()):.3f} (out), "
              f"{float((np.abs(held_lse - tail_lse) / ltol).max()):.3f} (lse); fold_held vs float64 {float((np.abs(held_out - want_out) / tol).max()):.3f}, "
              f"fold_tail vs float64 {float((np.abs(tail_out - want_out) / tol).max()):.3f}")
        assert np.all(np.abs(held_out - tail_out) <= tol) and np.all(np.abs(held_lse - tail_lse) <= ltol)
        assert np.all(np.abs(held_out - want_out) <= tol) and np.all(np.abs(held_lse - want_lse) <= ltol)
    finally:
        lib.finalize()


@pytest.mark.parametrize("rpp", [1, 4])
def test_fold_held_is_causal(rpp):
    """changing K / V of the draft positions behind j leaves the rows of positions <= j bit-identical"""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(91 + rpp)
        n_seq, n_q, sm = 4, 4, 0.0884
        G, P = rpp * n_q, 1 + n_q
        base = [0, 1, 1, 0]
        q = rng.standard_normal((n_seq, H, G, D)).astype(np.float16)
        out = rng.standard_normal((n_seq, H, G, D)).astype(np.float32)
        lse = rng.uniform(-3, 9, (n_seq, H, G)).astype(np.float32)
        kh = rng.standard_normal((n_seq, P, H, D)).astype(np.float16)
        vh = rng.standard_normal((n_seq, P, H, D)).astype(np.float16)
        first = run_fold_held(lib, torch, q, out, lse, kh.reshape(-1), vh.reshape(-1), P * H * D, H * D, base, None, rpp, sm)
        for j in range(n_q - 1):
            k2, v2 = kh.copy(), vh.copy()
            for i in range(n_seq):                                  # everything behind query position j of sequence i
                k2[i, base[i] + j + 1:] = rng.standard_normal(k2[i, base[i] + j + 1:].shape).astype(np.float16) * 3.0
                v2[i, base[i] + j + 1:] = rng.standard_normal(v2[i, base[i] + j + 1:].shape).astype(np.float16) * 3.0
            second = run_fold_held(lib, torch, q, out, lse, k2.reshape(-1), v2.reshape(-1), P * H * D, H * D, base, None, rpp, sm)
            upto = (j + 1) * rpp
            assert np.array_equal(first[0][:, :, :upto], second[0][:, :, :upto]) and np.array_equal(first[1][:, :, :upto], second[1][:, :, :upto])
            assert not np.array_equal(first[0][:, :, upto:], second[0][:, :, upto:])
    finally:
        lib.finalize()


def _region(k, v, T):
    """host copy of one layer's pages as HeadChecker takes them: T/2 pages of K then T/2 pages of V, positions k / v [n][H][D] (n even)"""
    pages = np.zeros((2, T, H, D), np.float16)
    pages[0, :len(k)] = k; pages[1, :len(v)] = v
    return pages.reshape(T, 2 * H * D)


@pytest.mark.parametrize("rpp", [4, 8])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_attend_spec_end_to_end(oracle, scheme, rpp):
    """SpeckvKVConnector.attend_spec over a batch of 5 requests (prompts odd, even, a single position, none, even), S = 4 new positions
    each: rows_per_pos = 4 is one group of 16 query rows, rows_per_pos = 8 two groups.  Reference in two steps: the stored part per
    (request, kv head) from HeadChecker.want with all S x rows_per_pos rows (out, lse, sum p|v|, score bound delta -- it quantises the
    query as the format's kernel does), then the float64 chained fold of the odd last position and the fp16 new rows, causally.
    Tolerance: HeadChecker.check's own ((2e-3 + 2 delta) mag + 1e-6 with mag carried through the folds, 2e-3 + delta on the scores'
    log-sum-exp) plus the derived fold bound -- fold weights are <= 1, the stored part's error carries over unamplified.  A ragged
    n_new leaves the live rows bit for bit and the others finite.  The call changes no state."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, S, layer = 2, 128, 4, 1
        conn = SpeckvKVConnector(lib, num_layers=L, num_kv_heads=H, head_dim=D, max_tokens=T, scheme=scheme)
        rng = np.random.default_rng(7 + rpp)
        dev = lambda a: torch.from_numpy(a).cuda()
        rids, prompts = [21, 22, 23, 24, 25], [37, 64, 1, 0, 22]
        data = {}
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            k, v = rng.standard_normal((L, n, H, D)).astype(np.float16), rng.standard_normal((L, n, H, D)).astype(np.float16)
            if n:
                conn.write_prefill(rid, dev(k), dev(v))
            data[rid] = (k, v)
        torch.cuda.synchronize()
        B, sm = len(rids), 1.0 / np.sqrt(D)
        q = rng.standard_normal((B, S, H, rpp, D)).astype(np.float16)
        k_new = rng.standard_normal((B, S, L, H, D)).astype(np.float16)
        v_new = rng.standard_normal((B, S, L, H, D)).astype(np.float16)
        before = {(rid, kind): conn.kv_rows(rid, layer, kind).cpu().numpy() for rid in rids for kind in (0, 1)}
        st0 = lib.stats()
        got = conn.attend_spec(layer, rids, dev(q), dev(k_new), dev(v_new), sm)
        torch.cuda.synchronize()
        n_new = [4, 3, 4, 1, 0]
        ragged = conn.attend_spec(layer, rids, dev(q), dev(k_new), dev(v_new), sm, n_new=n_new)
        torch.cuda.synchronize()
        got, ragged = got.cpu().numpy(), ragged.cpu().numpy()
        # no state changed
        st1 = lib.stats()
        for name in ("written_pages", "total_compressions", "pool_bytes_in_use", "total_allocations", "compressed_bytes"):
            assert getattr(st0, name) == getattr(st1, name), name
        for rid, n in zip(rids, prompts):
            assert conn.length(rid) == n
            for kind in (0, 1):
                assert np.array_equal(before[(rid, kind)].view(np.uint16), conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16))
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(ragged))
        for b in range(B):
            assert np.array_equal(ragged[b, :n_new[b]], got[b, :n_new[b]])
        # against the two-step reference
        worst = 0.0
        for b, (rid, n) in enumerate(zip(rids, prompts)):
            k, v = data[rid]
            even = n & ~1
            checker = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], T), T)
            for head in range(H):
                q_head = q[b, :, head].reshape(S * rpp, D)
                w_out, w_lse, w_mag, delta = checker.want(q_head, head, even, sm)
                for j in range(S):
                    r = slice(j * rpp, (j + 1) * rpp)
                    kh = np.concatenate([k[layer, even:n, head], k_new[b, :j + 1, layer, head]])      # the odd last position, then the new ones
                    vh = np.concatenate([v[layer, even:n, head], v_new[b, :j + 1, layer, head]])
                    want, _, mag = chained_folds((w_out[r], w_mag[r]), w_lse[r], q_head[r], kh, vh, sm)
                    err = np.abs(got[b, j, head] - want)
                    tol = (2e-3 + 2 * delta) * mag + 1e-6 + len(kh) * (2e-5 * np.abs(want) + 2e-6)
                    worst = max(worst, float((err / tol).max()))
                    assert np.all(err <= tol), (scheme, rpp, rid, head, j, float((err / tol).max()), delta)
        print(f"attend_spec {scheme} rows_per_pos={rpp}: worst err / tol {worst:.3f}")
        for rid in rids:
            conn.free_request(rid)
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_append_tokens_equals_single_appends(scheme):
    """Two connectors with the same seeded data: one commits ragged prefixes (0, 1, 2, 3, S accepted) with append_tokens over several
    steps, the other the same positions through append one at a time.  Afterwards the lengths, the rows of every layer and kind and
    a following attention agree bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, S, G = 2, 256, 4, 4
        a = SpeckvKVConnector(lib, L, H, D, T, scheme)
        b = SpeckvKVConnector(lib, L, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(19)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        ids_a, ids_b, prompts = [1, 2, 3, 4, 5], [101, 102, 103, 104, 105], [37, 64, 1, 0, 22]
        keep = []
        for ra, rb, n in zip(ids_a, ids_b, prompts):
            a.add_request(ra); b.add_request(rb)
            if n:
                k, v = rnd(L, n, H, D), rnd(L, n, H, D)
                keep += a.write_prefill(ra, k, v) + b.write_prefill(rb, k, v)
        B, sm = len(ids_a), 1.0 / np.sqrt(D)
        accepts = [[0, 1, 2, 3, S], [S, 0, 3, 2, 1], [1, 1, 0, S, 3], [2, 3, S, 1, 0], [3, S, 1, 0, 2]]
        for n_accept in accepts:
            k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
            keep += a.append_tokens(ids_a, k_new, v_new, n_accept)
            for t in range(S):
                members = [i for i in range(B) if n_accept[i] > t]
                if members:
                    idx = torch.tensor(members, device="cuda")
                    keep += b.append([ids_b[i] for i in members], k_new[idx, t], v_new[idx, t])
            torch.cuda.synchronize()
            qn = rnd(B, H, G, D)
            for layer in range(L):
                assert torch.equal(a.attend(layer, ids_a, qn, sm), b.attend(layer, ids_b, qn, sm)), (n_accept, layer)
        total = [sum(x[i] for x in accepts) for i in range(B)]
        for ra, rb, n, t in zip(ids_a, ids_b, prompts, total):
            assert a.length(ra) == b.length(rb) == n + t
            for layer in range(L):
                for kind in (0, 1):
                    assert torch.equal(a.kv_rows(ra, layer, kind).view(torch.int16), b.kv_rows(rb, layer, kind).view(torch.int16)), (ra, layer, kind)
        with pytest.raises(ValueError):
            a.append_tokens(ids_a, k_new, v_new, [S + 1, 0, 0, 0, 0])
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_planned_attention_and_fold_held_under_a_graph(scheme):
    """One layer's speckv_ext_attend_*_planned + speckv_ext_attend_fold_held captured once behind a first eager run, replayed with fresh
    q / held rows / d_base contents: equal to the eager calls on the same contents bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, S, rpp, layer = 2, 256, 4, 4, 1
        G, P = S * rpp, 1 + S
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, prompts = [1, 2, 3, 4], [64, 130, 22, 96]
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            conn.write_prefill(rid, rnd(L, n, H, D), rnd(L, n, H, D))
        B, sm, code = len(rids), 1.0 / np.sqrt(D), SCHEMES[scheme]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        bound = conn.plan_step(rids, s)
        plan = conn._plan
        q = rnd(B, H, G, D)
        kh, vh = rnd(B, P, L, H, D), rnd(B, P, L, H, D)
        base = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device="cuda")
        out = torch.zeros((B, H, G, D), dtype=torch.float32, device="cuda")
        lse = torch.zeros((B, H, G), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def run():
            lib.attend_planned(code, plan.data_ptr(), B, layer, q.data_ptr(), G, bound, sm, out.data_ptr(), lse.data_ptr(), s.cuda_stream)
            lib.attend_fold_held(B, 0, H, G, rpp, q.data_ptr(), kh.data_ptr() + layer * H * D * 2, vh.data_ptr() + layer * H * D * 2, P * L * H * D, L * H * D,
                                 base.data_ptr(), 0, sm, out.data_ptr(), lse.data_ptr(), s.cuda_stream)
        run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            run()
        for fresh in ([1, 0, 0, 1], [0, 0, 1, 1]):
            q.copy_(rnd(B, H, G, D)); kh.copy_(rnd(B, P, L, H, D)); vh.copy_(rnd(B, P, L, H, D))
            base.copy_(torch.tensor(fresh, dtype=torch.int32))
            torch.cuda.synchronize()
            run(); torch.cuda.synchronize()
            eager_out, eager_lse = out.clone(), lse.clone()
            out.fill_(float("nan")); lse.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager_out) and torch.equal(lse, eager_lse)
            assert bool(torch.isfinite(out).all())
        del g
        for rid in rids:
            conn.free_request(rid)
    finally:
        lib.finalize()


def test_spec_decode_example_runs():
    """examples/spec_decode_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "spec_decode_example.py"), "--steps", "5"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spec decode example ok" in out.stdout
