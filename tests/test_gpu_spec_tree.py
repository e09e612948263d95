"""-m gpu: tree-shaped drafts in the multi-position decode step -- speckv_ext_attend_fold_masked (the positions a step holds outside
the pool, folded under a per-(sequence, query position) visibility mask) and SpeckvKVConnector.attend_spec(parents=...) / append_path
on top of it.  Every reference is numpy float64 in this file.

Tolerance of a fold, as tests/test_gpu_spec_step.py derives it: the single-fold bound (2e-5 |want| + 2e-6 on out, 1e-5 max(1, |want|) on
lse) times the number of positions folded into the row -- here the popcount of the row's mask word."""
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
LOW = (1 << HELD_MAX) - 1                                     # the bits of a mask word that count


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


def bits_of(word):
    return [t for t in range(HELD_MAX) if (int(word) >> t) & 1]


def want_fold_masked(out, lse, q, kh, vh, masks, rpp, sm, rows=None):
    """the definition of speckv_ext_attend_fold_masked in float64: the fold formula applied to the visible held positions in ascending
    order.  out [n][H][g][D], lse [n][H][g], q likewise (fp16); kh / vh [m][P][H][D] fp16; masks [m][>= n_q] mask words; rows: the
    sequences the m held sets belong to.  Returns out, lse, folds [n][H][g] (the popcount of the row's word)"""
    want_out, want_lse = out.astype(np.float64), lse.astype(np.float64)
    folds = np.zeros(lse.shape, np.int64)
    g = out.shape[2]
    for i in range(len(kh)):
        b = i if rows is None else rows[i]
        for j in range(g // rpp):
            vis = bits_of(masks[i][j])
            if not vis:
                continue
            r0, r1 = j * rpp, (j + 1) * rpp
            for h in range(out.shape[1]):
                want_out[b, h, r0:r1], want_lse[b, h, r0:r1] = chained_folds(want_out[b, h, r0:r1], want_lse[b, h, r0:r1], q[b, h, r0:r1],
                                                                             kh[i, vis, h], vh[i, vis, h], sm)
            folds[b, :, r0:r1] = len(vis)
    return want_out, want_lse, folds


def run_fold_masked(lib, torch, q, out, lse, kh_buf, vh_buf, seq_stride, pos_stride, masks, rpp, sm, rows=None):
    """masks: [m][mask_stride] array of words"""
    masks = np.ascontiguousarray(np.asarray(masks, np.uint32))
    d_q, d_out, d_lse = torch.from_numpy(q).cuda(), torch.from_numpy(out).cuda(), torch.from_numpy(lse).cuda()
    d_k, d_v = torch.from_numpy(kh_buf).cuda(), torch.from_numpy(vh_buf).cuda()
    d_mask = torch.from_numpy(masks.view(np.int32)).cuda()
    d_rows = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lib.attend_fold_masked(masks.shape[0], 0 if rows is None else d_rows.data_ptr(), q.shape[1], q.shape[2], rpp, d_q.data_ptr(), d_k.data_ptr(),
                           d_v.data_ptr(), seq_stride, pos_stride, d_mask.data_ptr(), masks.shape[1], sm, d_out.data_ptr(), d_lse.data_ptr(),
                           s.cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_lse.cpu().numpy()


def run_fold_held(lib, torch, q, out, lse, kh_buf, vh_buf, seq_stride, pos_stride, base, n_live, rpp, sm, rows=None):
    d_q, d_out, d_lse = torch.from_numpy(q).cuda(), torch.from_numpy(out).cuda(), torch.from_numpy(lse).cuda()
    d_k, d_v = torch.from_numpy(kh_buf).cuda(), torch.from_numpy(vh_buf).cuda()
    d_base = torch.from_numpy(np.asarray(base, np.int32)).cuda()
    d_live = torch.from_numpy(np.asarray(n_live, np.int32)).cuda()
    d_rows = None if rows is None else torch.from_numpy(np.asarray(rows, np.int32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    lib.attend_fold_held(len(base), 0 if rows is None else d_rows.data_ptr(), q.shape[1], q.shape[2], rpp, d_q.data_ptr(), d_k.data_ptr(), d_v.data_ptr(),
                         seq_stride, pos_stride, d_base.data_ptr(), d_live.data_ptr(), sm, d_out.data_ptr(), d_lse.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_lse.cpu().numpy()


def random_tree(rng, S):
    return [int(rng.integers(-1, j)) for j in range(S)]


def mask_words(kind, rng, m, n_q):
    """[m][n_q] mask words of one kind; every word non-zero"""
    base = [0, 1, 1, HELD_MAX - n_q, 0][:m]
    if kind == "chain":
        return [[(1 << (x + j + 1)) - 1 for j in range(n_q)] for x in base]
    if kind == "star":
        return [[((1 << x) - 1) | 1 << (x + j) for j in range(n_q)] for x in base]
    if kind == "tree":
        return SpeckvKVConnector.tree_masks([random_tree(rng, n_q) for _ in range(m)], [min(x, 1) for x in base])
    if kind == "gaps":                                         # any subset of the held positions, most of them with holes
        return [[int(rng.integers(1, LOW + 1)) for _ in range(n_q)] for _ in range(m)]
    if kind == "bit16":                                        # the last held position, alone and among others
        return [[1 << 16 if (i + j) % 3 == 0 else int(rng.integers(0, LOW + 1)) | 1 << 16 for j in range(n_q)] for i in range(m)]
    raise KeyError(kind)


def fold_case(rng, rpp, n_q, n_seq=7):
    """the inputs of tests/test_gpu_spec_step.py::test_fold_held_against_float64_chained_folds: random incoming (out, lse), a sequence
    with nothing stored, scores about 40 above and below the stored lse, held rows as one layer of [seq][pos][layers][heads][dim] with
    a gap behind every sequence, a row subset"""
    G, Lyr, layer = rpp * n_q, 2, 1
    rows = [5, 0, 3, 6, 2]                                    # sequences 1 and 4 are not in the launch
    m, P = len(rows), HELD_MAX
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
    off = layer * H * D
    return dict(rows=rows, q=q, out=out, lse=lse, kbuf=kbuf[off:], vbuf=vbuf[off:], kh=view(kbuf), vh=view(vbuf), seq_stride=seq_stride,
                pos_stride=pos_stride)


# rows_per_pos in {1, 4, 8} x query positions in {1, 2, 4, 16}: every pair that is a launch shape (at most 16 query rows per kv head)
SHAPES = [(rpp, n_q) for rpp in (1, 4, 8) for n_q in (1, 2, 4, 16) if rpp * n_q <= 16]
KINDS = ["chain", "star", "tree", "gaps", "bit16"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rpp,n_q", SHAPES)
def test_fold_masked_against_float64(rpp, n_q, kind):
    """The kernel against the fold formula applied to the visible subset in ascending order, in float64: chains, stars, random trees,
    masks with gaps and masks that use bit 16; a sequence with nothing stored (out 0, lse -inf), scores +-40 from the stored lse, a row
    subset through d_rows, strides with slack (held rows and mask table).  A mask word of 0 and a sequence outside d_rows leave their
    rows bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(2000 * rpp + 20 * n_q + KINDS.index(kind))
        c = fold_case(rng, rpp, n_q)
        rows, m, sm = c["rows"], len(c["rows"]), 0.0884
        words = mask_words(kind, rng, m, n_q)
        words[4] = [0] * n_q                                   # a sequence without a live position (row 2)
        if n_q > 1:
            words[2][n_q - 1] = 0                              # ... and one a position short (row 3)
        stride = n_q + 3
        table = rng.integers(1, LOW + 1, (m, stride)).astype(np.uint32)      # (the words behind a sequence's n_q belong to nobody)
        table[:, :n_q] = np.asarray(words, np.uint32)
        want_out, want_lse, folds = want_fold_masked(c["out"], c["lse"], c["q"], c["kh"], c["vh"], words, rpp, sm, rows)
        got_out, got_lse = run_fold_masked(lib, torch, c["q"], c["out"], c["lse"], c["kbuf"], c["vbuf"], c["seq_stride"], c["pos_stride"], table,
                                           rpp, sm, rows)
        touched = folds > 0
        err, lerr = np.abs(got_out - want_out), np.abs(got_lse - want_lse)
        tol = folds[..., None] * (2e-5 * np.abs(want_out) + 2e-6)
        ltol = folds * 1e-5 * np.maximum(1.0, np.abs(want_lse))
        print(f"fold_masked rpp={rpp} n_q={n_q} {kind}: worst out err / tol {float((err[touched] / tol[touched]).max()):.3f}, "
              f"lse err / tol {float((lerr[touched] / ltol[touched]).max()):.3f}, most folds {int(folds.max())}")
        assert np.all(err[touched] <= tol[touched])
        assert np.all(lerr[touched] <= ltol[touched])
        assert np.array_equal(got_out[~touched], c["out"][~touched]) and np.array_equal(got_lse[~touched], c["lse"][~touched])
        assert not touched[1].any() and not touched[4].any() and not touched[2].any() and touched[0].all() and touched[6].all()
        if n_q > 1:
            assert not touched[3][:, (n_q - 1) * rpp:].any() and touched[3][:, :(n_q - 1) * rpp].all()
        # nothing stored: plain softmax attention over the visible held positions
        i0 = rows.index(0)
        for j in range(n_q):
            vis = bits_of(words[i0][j])
            s = np.einsum("hrd,thd->hrt", c["q"][0, :, j * rpp:(j + 1) * rpp].astype(np.float64), c["kh"][i0, vis].astype(np.float64)) * sm
            p = np.exp(s - s.max(axis=-1, keepdims=True)); p /= p.sum(axis=-1, keepdims=True)
            plain = np.einsum("hrt,thd->hrd", p, c["vh"][i0, vis].astype(np.float64))
            assert np.all(np.abs(got_out[0, :, j * rpp:(j + 1) * rpp] - plain) <= len(vis) * (2e-5 * np.abs(plain) + 2e-6))
    finally:
        lib.finalize()


@pytest.mark.parametrize("rpp,n_q", SHAPES)
def test_chain_masks_equal_fold_held(rpp, n_q):
    """chain masks (1 << (base + j + 1)) - 1, 0 for the positions past the live count, against speckv_ext_attend_fold_held with d_base /
    d_n_q on the same inputs: required within the fold tolerance (taken at the float64 result); whether the two are also bit-identical
    is printed (found on the MI355X: profiles/spec_tree_step.txt)"""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(3000 * rpp + n_q)
        c = fold_case(rng, rpp, n_q)
        rows, sm = c["rows"], 0.0884
        base = [0, 1, 1, HELD_MAX - n_q, 0]
        live = [n_q, n_q, max(n_q - 1, 1), n_q, 0]
        words = [[(1 << (x + j + 1)) - 1 if j < n else 0 for j in range(n_q)] for x, n in zip(base, live)]
        assert SpeckvKVConnector.tree_masks(list(range(-1, n_q - 1)), [0, 1, 1, 0, 0], live)[:3] == words[:3]       # what the connector would send
        args = (c["q"], c["out"], c["lse"], c["kbuf"], c["vbuf"], c["seq_stride"], c["pos_stride"])
        held_out, held_lse = run_fold_held(lib, torch, *args, base, live, rpp, sm, rows)
        mask_out, mask_lse = run_fold_masked(lib, torch, *args, words, rpp, sm, rows)
        want_out, want_lse, folds = want_fold_masked(c["out"], c["lse"], c["q"], c["kh"], c["vh"], words, rpp, sm, rows)
        tol = folds[..., None] * (2e-5 * np.abs(want_out) + 2e-6)
        ltol = folds * 1e-5 * np.maximum(1.0, np.abs(want_lse))
        same = np.array_equal(held_out.view(np.uint32), mask_out.view(np.uint32)) and np.array_equal(held_lse.view(np.uint32), mask_lse.view(np.uint32))
        touched = folds > 0
        print(f"chain masks vs fold_held rpp={rpp} n_q={n_q}: bit-identical {same}; worst difference / tol "
              f"{float((np.abs(held_out - mask_out)[touched] / tol[touched]).max()):.3f} (out), "
              f"{float((np.abs(held_lse - mask_lse)[touched] / ltol[touched]).max()):.3f} (lse)")
        assert np.all(np.abs(held_out - mask_out) <= tol) and np.all(np.abs(held_lse - mask_lse) <= ltol)      # (tol 0 where nothing is folded)
        assert np.all(np.abs(mask_out - want_out) <= tol) and np.all(np.abs(mask_lse - want_lse) <= ltol)
    finally:
        lib.finalize()


@pytest.mark.parametrize("rpp,tree", [(1, [-1, 0, 1, 2, 1, 4]), (4, [-1, 0, 0, 2])])
def test_fold_masked_isolates_a_node_from_everything_but_its_ancestors(rpp, tree):
    """changing K / V of every held position a node does not see -- siblings with a lower index among them, and whatever lies behind
    the step's positions -- leaves the node's rows bit-identical; changing any one it sees changes them; bits >= SPECKV_HELD_MAX in
    the words change nothing"""
    torch = torch_mod()
    lib = open_lib()
    try:
        rng = np.random.default_rng(77 + rpp)
        n_seq, n_q, sm, P = 4, len(tree), 0.0884, HELD_MAX
        G = rpp * n_q
        base = [0, 1, 1, 0]
        words = SpeckvKVConnector.tree_masks(tree, base)
        q = rng.standard_normal((n_seq, H, G, D)).astype(np.float16)
        out = rng.standard_normal((n_seq, H, G, D)).astype(np.float32)
        lse = rng.uniform(-3, 9, (n_seq, H, G)).astype(np.float32)
        kh = rng.standard_normal((n_seq, P, H, D)).astype(np.float16)
        vh = rng.standard_normal((n_seq, P, H, D)).astype(np.float16)
        run = lambda k, v, w: run_fold_masked(lib, torch, q, out, lse, k.reshape(-1), v.reshape(-1), P * H * D, H * D, w, rpp, sm)
        first = run(kh, vh, words)
        high = run(kh, vh, [[w | int(rng.integers(1, 1 << 15)) << HELD_MAX for w in row] for row in words])
        assert np.array_equal(first[0].view(np.uint32), high[0].view(np.uint32)) and np.array_equal(first[1].view(np.uint32), high[1].view(np.uint32))
        lower_sibling = False
        for j in range(n_q):
            r = slice(j * rpp, (j + 1) * rpp)
            k2, v2 = kh.copy(), vh.copy()
            for i in range(n_seq):                                  # everything node j of sequence i does not see
                hidden = [t for t in range(P) if not (words[i][j] >> t) & 1]
                lower_sibling |= any(base[i] <= t < base[i] + j for t in hidden)
                k2[i, hidden] = rng.standard_normal(k2[i, hidden].shape).astype(np.float16) * 3.0
                v2[i, hidden] = rng.standard_normal(v2[i, hidden].shape).astype(np.float16) * 3.0
            second = run(k2, v2, words)
            assert np.array_equal(first[0][:, :, r].view(np.uint32), second[0][:, :, r].view(np.uint32)), j
            assert np.array_equal(first[1][:, :, r].view(np.uint32), second[1][:, :, r].view(np.uint32)), j
            for pick in range(2):                                   # one position the node sees: its first ancestor (or itself), then itself
                k3, v3 = kh.copy(), vh.copy()
                for i in range(n_seq):
                    t = bits_of(words[i][j])[-pick]
                    k3[i, t] = rng.standard_normal(k3[i, t].shape).astype(np.float16) * 3.0
                    v3[i, t] = rng.standard_normal(v3[i, t].shape).astype(np.float16) * 3.0
                third = run(k3, v3, words)
                for i in range(n_seq):
                    assert not np.array_equal(first[0][i, :, r], third[0][i, :, r]), (j, pick, i)
                    assert not np.array_equal(first[1][i, :, r], third[1][i, :, r]), (j, pick, i)
        assert lower_sibling                                        # the tree has a node with a lower-numbered node it must not see
    finally:
        lib.finalize()


def test_fold_masked_refuses_bad_arguments_on_the_gpu():
    """the sets of tests/test_spec_tree_cpu.py, on the device: SPECKV_ERR_INVAL, nothing launched"""
    torch = torch_mod()
    lib = open_lib()
    try:
        buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
        p, s = buf.data_ptr(), torch.cuda.Stream().cuda_stream
        for heads, g, rpp, seq_stride, pos_stride, mask, mask_stride, lse in (
                (8, 8, 4, 17408, 1024, 0, 2, p), (8, 8, 4, 17408, 1024, p, 1, p), (8, 16, 1, 17408, 1024, p, 0, p),
                (8, 8, 3, 17408, 1024, p, 16, p), (8, 32, 2, 17408, 1024, p, 16, p), (8, 17, 1, 17408, 1024, p, 17, p), (8, 8, 0, 17408, 1024, p, 16, p),
                (8, 8, 4, 17408, 1024, p, 2, 0), (8, 8, 4, 17408, 1028, p, 2, p), (8, 8, 4, 17408, 1016, p, 2, p), (8, 8, 4, 17412, 1024, p, 2, p),
                (8, 8, 4, 1024, 1024, p, 2, p), (0, 8, 4, 17408, 1024, p, 2, p)):
            with pytest.raises(SpeckvError) as e:
                lib.attend_fold_masked(1, 0, heads, g, rpp, p, p, p, seq_stride, pos_stride, mask, mask_stride, 0.1, p, lse, s)
            assert e.value.status == -4
        torch.cuda.synchronize()
        assert float(buf.abs().max()) == 0.0
    finally:
        lib.finalize()


def _region(k, v, T):
    """host copy of one layer's pages as HeadChecker takes them: T/2 pages of K then T/2 pages of V, positions k / v [n][H][D] (n even)"""
    pages = np.zeros((2, T, H, D), np.float16)
    pages[0, :len(k)] = k; pages[1, :len(v)] = v
    return pages.reshape(T, 2 * H * D)


def _ancestors(tree, j):
    """node j's ancestors and j itself, ascending"""
    chain = []
    while j != -1:
        chain.append(j)
        j = tree[j]
    return chain[::-1]


def _leaf_paths(tree):
    return [_ancestors(tree, j) for j in range(len(tree)) if j not in tree]


# rows_per_pos 1: 16 nodes in one group; 4: 6 nodes in groups of 4 + 2; 8: 4 nodes in groups of 2 + 2 -- branches that span the groups
TREES = {1: [-1, 0, 1, 2, 1, 4, 0, 6, 7, 8, -1, 10, 10, 12, 5, 3], 4: [-1, 0, 1, 2, 1, 4], 8: [-1, 0, 0, 2]}


@pytest.mark.parametrize("rpp", [1, 4, 8])
@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_attend_spec_tree_end_to_end(oracle, scheme, rpp):
    """SpeckvKVConnector.attend_spec(parents=...) over the batch of tests/test_gpu_spec_step.py::test_attend_spec_end_to_end (prompts odd,
    even, a single position, none, even): one tree for all requests, then one tree per request with a ragged n_new.
    Reference 1, as that test builds it: the stored part per (request, kv head) from HeadChecker.want with all S x rows_per_pos rows,
    then the float64 chained fold of the odd last position and the fp16 rows of the node's ancestors and the node, ascending; that
    test's tolerance rule: (2e-3 + 2 delta) mag + 1e-6 from HeadChecker plus the fold bound per folded position.
    Reference 2: chain attend_spec calls on the same connector, one per root-to-leaf path (nothing changes state, so the same pool
    answers both): both lie within reference 1's tolerance of the float64 result, so they differ by at most twice that.
    Dead nodes' rows are finite, live nodes' rows do not depend on the dead ones.  The call changes no state."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, layer = 2, 128, 1
        tree = TREES[rpp]
        S = len(tree)
        assert len(SpeckvKVConnector.spec_groups(S, rpp)) == (1 if rpp == 1 else 2)
        conn = SpeckvKVConnector(lib, num_layers=L, num_kv_heads=H, head_dim=D, max_tokens=T, scheme=scheme)
        rng = np.random.default_rng(70 + rpp)
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
        shared = conn.attend_spec(layer, rids, dev(q), dev(k_new), dev(v_new), sm, parents=tree).cpu().numpy()
        own_trees = [tree] + [random_tree(rng, S) for _ in range(B - 1)]
        n_new = [S, S - 1, S, 1, 0]
        own = conn.attend_spec(layer, rids, dev(q), dev(k_new), dev(v_new), sm, n_new=n_new, parents=own_trees).cpu().numpy()
        own_masks = SpeckvKVConnector.tree_masks(own_trees, [n & 1 for n in prompts], n_new)
        # reference 2: the tree's root-to-leaf paths as chain steps
        by_path = {}
        for path in _leaf_paths(tree):
            got = conn.attend_spec(layer, rids, dev(np.ascontiguousarray(q[:, path])), dev(np.ascontiguousarray(k_new[:, path])),
                                   dev(np.ascontiguousarray(v_new[:, path])), sm).cpu().numpy()
            for at, j in enumerate(path):
                by_path.setdefault(j, []).append(got[:, at])
        assert sorted(by_path) == list(range(S))
        torch.cuda.synchronize()
        # no state changed
        st1 = lib.stats()
        for name in ("written_pages", "total_compressions", "pool_bytes_in_use", "total_allocations", "compressed_bytes"):
            assert getattr(st0, name) == getattr(st1, name), name
        for rid, n in zip(rids, prompts):
            assert conn.length(rid) == n
            for kind in (0, 1):
                assert np.array_equal(before[(rid, kind)].view(np.uint16), conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16))
        assert np.all(np.isfinite(shared)) and np.all(np.isfinite(own))
        assert np.array_equal(own[0], shared[0])                  # request 0: the same tree, every node live
        worst, worst_paths, identical = 0.0, 0.0, True
        for b, (rid, n) in enumerate(zip(rids, prompts)):
            k, v = data[rid]
            even = n & ~1
            checker = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], T), T)
            for head in range(H):
                q_head = q[b, :, head].reshape(S * rpp, D)
                w_out, w_lse, w_mag, delta = checker.want(q_head, head, even, sm)
                for got_all, trees, live in ((shared, [tree] * B, None), (own, own_trees, own_masks)):
                    for j in range(S):
                        if live is not None and live[b][j] == 0:
                            continue                               # a dead node: finite, otherwise unspecified
                        r = slice(j * rpp, (j + 1) * rpp)
                        nodes = _ancestors(trees[b], j)
                        kh = np.concatenate([k[layer, even:n, head], k_new[b, nodes, layer, head]])       # the odd last position, then the node's line
                        vh = np.concatenate([v[layer, even:n, head], v_new[b, nodes, layer, head]])
                        want, _, mag = chained_folds((w_out[r], w_mag[r]), w_lse[r], q_head[r], kh, vh, sm)
                        err = np.abs(got_all[b, j, head] - want)
                        tol = (2e-3 + 2 * delta) * mag + 1e-6 + len(kh) * (2e-5 * np.abs(want) + 2e-6)
                        worst = max(worst, float((err / tol).max()))
                        assert np.all(err <= tol), (scheme, rpp, rid, head, j, float((err / tol).max()), delta)
                        if live is None:
                            for chain in by_path[j]:
                                diff = np.abs(chain[b, head] - got_all[b, j, head])
                                worst_paths = max(worst_paths, float((diff / (2 * tol)).max()))
                                identical &= np.array_equal(chain[b, head], got_all[b, j, head])
                                assert np.all(diff <= 2 * tol), (scheme, rpp, rid, head, j)
        print(f"attend_spec tree {scheme} rows_per_pos={rpp} S={S}: worst err / tol {worst:.3f} against float64; against the chain call per path: "
              f"worst difference / (2 tol) {worst_paths:.4f}, bit-identical {identical}")
        for rid in rids:
            conn.free_request(rid)
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_append_path_equals_single_appends(scheme):
    """Two connectors with the same seeded data: one commits paths of a tree step (none, a lone node, a branch, the other branch, the
    trunk; then random paths of per-request trees) with append_path, the other the same rows through append one at a time.
    Afterwards the lengths, the rows of every layer and kind and a following attention agree bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, S, G = 2, 256, 6, 4
        a = SpeckvKVConnector(lib, L, H, D, T, scheme)
        b = SpeckvKVConnector(lib, L, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(29)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(29)
        ids_a, ids_b, prompts = [1, 2, 3, 4, 5], [101, 102, 103, 104, 105], [37, 64, 1, 0, 22]
        keep = []
        for ra, rb, n in zip(ids_a, ids_b, prompts):
            a.add_request(ra); b.add_request(rb)
            if n:
                k, v = rnd(L, n, H, D), rnd(L, n, H, D)
                keep += a.write_prefill(ra, k, v) + b.write_prefill(rb, k, v)
        B, sm = len(ids_a), 1.0 / np.sqrt(D)
        tree = [-1, 0, 1, 2, 1, 4]
        steps = [(tree, [[], [0], [0, 1, 4, 5], [0, 1, 2, 3], [0, 1]]), (tree, [[0, 1, 2, 3], [], [0, 1, 4], [0], [0, 1, 4, 5]])]
        for _ in range(3):
            trees = [random_tree(rng, S) for _ in range(B)]
            steps.append((trees, [_ancestors(t, int(x)) if x >= 0 else [] for t, x in zip(trees, rng.integers(-1, S, B))]))
        total = [0] * B
        for parents, paths in steps:
            k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
            keep += a.append_path(ids_a, k_new, v_new, paths, parents)
            for t in range(S):
                members = [i for i in range(B) if len(paths[i]) > t]
                if members:
                    idx = torch.tensor(members, device="cuda")
                    node = torch.tensor([paths[i][t] for i in members], device="cuda")
                    keep += b.append([ids_b[i] for i in members], k_new[idx, node], v_new[idx, node])
            torch.cuda.synchronize()
            total = [n + len(p) for n, p in zip(total, paths)]
            qn = rnd(B, H, G, D)
            for layer in range(L):
                assert torch.equal(a.attend(layer, ids_a, qn, sm), b.attend(layer, ids_b, qn, sm)), (paths, layer)
        for ra, rb, n, t in zip(ids_a, ids_b, prompts, total):
            assert a.length(ra) == b.length(rb) == n + t
            for layer in range(L):
                for kind in (0, 1):
                    assert torch.equal(a.kv_rows(ra, layer, kind).view(torch.int16), b.kv_rows(rb, layer, kind).view(torch.int16)), (ra, layer, kind)
        lengths = [a.length(r) for r in ids_a]
        with pytest.raises(ValueError):
            a.append_path(ids_a, k_new, v_new, [[0, 1, 2, 5], [], [], [], []], tree)       # node 5 hangs below node 4
        assert [a.length(r) for r in ids_a] == lengths
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_planned_attention_and_fold_masked_under_a_graph(scheme):
    """One layer's speckv_ext_attend_*_planned + speckv_ext_attend_fold_masked captured once behind a first eager run, replayed with fresh
    q / held rows / mask words: equal to the eager calls on the same contents bit for bit."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, S, rpp, layer = 2, 256, 4, 4, 1
        G, P = S * rpp, 1 + S
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(31)
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
        words = lambda trees, base, n_new=None: torch.tensor(SpeckvKVConnector.tree_masks(trees, base, n_new), dtype=torch.int32)
        masks = words([-1, 0, 0, 2], [0, 1, 1, 0]).cuda()
        out = torch.zeros((B, H, G, D), dtype=torch.float32, device="cuda")
        lse = torch.zeros((B, H, G), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def run():
            lib.attend_planned(code, plan.data_ptr(), B, layer, q.data_ptr(), G, bound, sm, out.data_ptr(), lse.data_ptr(), s.cuda_stream)
            lib.attend_fold_masked(B, 0, H, G, rpp, q.data_ptr(), kh.data_ptr() + layer * H * D * 2, vh.data_ptr() + layer * H * D * 2, P * L * H * D,
                                   L * H * D, masks.data_ptr(), S, sm, out.data_ptr(), lse.data_ptr(), s.cuda_stream)
        run(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            run()
        first = None
        for fresh in (words([-1, -1, 1, 0], [1, 0, 0, 1]), words([[-1, 0, 1, 2], [-1, -1, -1, -1], [-1, 0, 0, 0], [-1, 0, 1, 1]], [0, 0, 1, 1], [4, 3, 4, 2])):
            q.copy_(rnd(B, H, G, D)); kh.copy_(rnd(B, P, L, H, D)); vh.copy_(rnd(B, P, L, H, D))
            masks.copy_(fresh)
            torch.cuda.synchronize()
            run(); torch.cuda.synchronize()
            eager_out, eager_lse = out.clone(), lse.clone()
            out.fill_(float("nan")); lse.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager_out) and torch.equal(lse, eager_lse)
            assert bool(torch.isfinite(out).all())
            assert first is None or not torch.equal(first, out)
            first = out.clone()
        del g
        for rid in rids:
            conn.free_request(rid)
    finally:
        lib.finalize()


def test_spec_tree_example_runs():
    """examples/spec_tree_example.py end to end on the MI355X, as a child process of its own"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "spec_tree_example.py"), "--steps", "5"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spec tree example ok" in out.stdout
