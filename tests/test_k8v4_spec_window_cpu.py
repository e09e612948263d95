"""Not -m gpu: the split pool's multi-position step on a sliding-window layer -- the declaration of speckv_ext_attend_kv_spec_window, its
answer on an engine without a device and its refusals there, the walk rule (csrc/spec_window.hpp through speckv_ext_spec_window_range, and
its restatement SpeckvKVConnector.spec_window_range) against brute force, tree_masks(window=W) against a brute-force visible set, what
SpeckvSplitKVConnector.attend_spec(window=W) hands the library (against a recording library), and a numpy float64 restatement of the
kernel's scheme -- scores masked per row, V block codes dropped only where EVERY row is masked -- over hostile records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_k8v4_spec_cpu import _RecordingLib, _read_f16, _read_u32, _step
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, PLAIN, RANGE = "speckv_ext_attend_kv_spec_window", "speckv_ext_attend_kv_spec", "speckv_ext_spec_window_range"
L, H, D, T = 4, 8, 128, 64
ROW = H * D
TREES = ([-1, 0, 1, 2, 0, 4, 5], [-1, 0, 1, 0, 3])


# ------------------------------------------------------------------------------------------------------------- the declaration
def test_the_entry_is_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    mine, plain = _declared(header, ENTRY), _declared(header, PLAIN)
    # the arguments of speckv_ext_attend_kv_spec with length, d_depth, window directly behind pos_end
    assert mine == plain.replace("const uint32_t* pos_end, ", "const uint32_t* pos_end, const uint32_t* length, const uint32_t* d_depth, uint32_t window, ")
    assert mine != plain and _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]            # the binding is the declaration
    assert _declared(header, RANGE) == "uint32_t length, uint32_t window, uint32_t* out_begin, int32_t* out_rel, uint32_t* out_n_pages"
    source = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    assert ENTRY in source and RANGE in source
    assert re.search(r"global:[^}]*\bspeckv_\*;", open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read())
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("/* %s:" % ENTRY):header.index("speckv_status_t %s(" % ENTRY)])     # the comment as running text
    for said in ("lo(d) = max(0, length[i] + d + 1 - W)", "PER QUERY ROW", "begin = lo(0) & ~31", "whatever depths the call carries", "skip = max(0, rel + d) <= 46",
                 "length[i] + 16 <= window", "NOT capturable", "a NULL length or d_depth with window != 0", "{pos_end[i], pos_end[i] + 1}",
                 "SPECKV_EXT_ABI_VERSION stays"):
        assert said in text, said
    assert "There is no form under a sliding window" not in header


def test_the_library_exports_the_entry_at_version_6():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, ENTRY) and hasattr(lib, RANGE)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    assert callable(pkg.SpeckvLib.attend_kv_spec_window) and callable(pkg.SpeckvLib.spec_window_range)


def _null_call(lib, h, at, **change):
    args = dict(k_handles=[h], v_handles=[h], layer=0, d_q_f16=at, g=8, rows_per_pos=4, pos_end=[32], length=[33], d_depth=at, window=20, d_k_held=at, d_v_held=at,
                seq_stride_elems=3 * ROW, pos_stride_elems=ROW, d_mask=at, mask_stride=2, sm_scale=0.1, d_out=at, d_lse=None, stream=1)
    args.update(change)
    with pytest.raises(SpeckvError) as e:
        lib.attend_kv_spec_window(**args)
    return e.value.status


def test_the_entry_on_the_null_engine_answers_as_its_sibling_and_refuses_first():
    """a good set: SPECKV_ERR_DRIVER as speckv_ext_attend_kv_spec answers there (no data path); each refusal -- the sibling's and the new
    ones -- is judged before anything else, so it is SPECKV_ERR_INVAL on this engine too; window = 0 looks at neither length nor d_depth"""
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        with pytest.raises(SpeckvError) as e:
            lib.attend_kv_spec([h], [h], 0, at, 8, 4, [32], at, at, 3 * ROW, ROW, at, 2, 0.1, at, None, 1)
        assert _null_call(lib, h, at) == e.value.status == -2                       # SPECKV_ERR_DRIVER
        for good in (dict(length=[32]), dict(d_lse=at), dict(window=0), dict(window=0, length=None, d_depth=0), dict(window=0, length=[77]), dict(window=1),
                     dict(window=2 ** 32 - 1)):
            assert _null_call(lib, h, at, **good) == -2, good
        for change in (dict(length=None), dict(d_depth=0), dict(length=[31]), dict(length=[34]), dict(length=[0]), dict(pos_end=[34], length=[33]),
                       dict(rows_per_pos=0), dict(rows_per_pos=3), dict(g=17, rows_per_pos=1, mask_stride=17), dict(d_k_held=0), dict(d_v_held=0), dict(d_mask=0),
                       dict(mask_stride=1), dict(seq_stride_elems=3 * ROW + 4), dict(pos_stride_elems=ROW + 4), dict(pos_stride_elems=ROW - 8),
                       dict(d_k_held=at + 8), dict(d_v_held=at + 2)):
            assert _null_call(lib, h, at, **change) == -4, change                    # SPECKV_ERR_INVAL
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------- the walk rule
def _tiles_bound(W):
    return (W + 31 + 31) // 32                                                     # decode_window_tiles_bound (csrc/decode_window.hpp)


def test_the_walk_rule_against_brute_force():
    """every length in 0..200, W in 1..100, depth in 0..15: the positions the walk leaves row d are exactly [lo(d), stored); the export and
    the restatement agree; begin on a tile, skip <= 46, the tiles within decode_window_tiles_bound(W); lo(0) >= stored walks nothing"""
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        empty = 0
        for length in range(201):
            stored = length & ~1
            for W in range(1, 101):
                begin, rel, n_pages = lib.spec_window_range(length, W)
                assert (begin, rel, n_pages) == SpeckvKVConnector.spec_window_range(length, W), (length, W)
                lo0 = max(0, length + 1 - W)
                if lo0 >= stored:
                    assert n_pages == 0, (length, W)
                    empty += 1
                else:
                    assert begin % 32 == 0 and begin <= lo0 < begin + 32 and n_pages == (stored - begin) // 2 and (n_pages + 15) // 16 <= _tiles_bound(W), (length, W)
                    assert rel == length + 1 - W - begin and rel <= 31
                for d in range(16):
                    skip = SpeckvKVConnector.spec_window_skip(rel, d)
                    assert skip == max(0, rel + d)
                    walked = set(range(begin + skip, begin + 2 * n_pages))
                    assert walked == set(range(max(0, length + d + 1 - W), stored)), (length, W, d)
                    assert n_pages == 0 or skip <= 46
                assert SpeckvKVConnector.spec_window_skip(rel, 40) == SpeckvKVConnector.spec_window_skip(rel, 15)      # depths are clamped
        assert empty > 200
        assert lib.spec_window_range(4000000000, 5) == (3999999968, 28, 16) and lib.spec_window_range(0, 2 ** 32 - 1)[1] == -(2 ** 31)
        with pytest.raises(SpeckvError):
            lib.spec_window_range(10, 0)
        with pytest.raises(ValueError):
            SpeckvKVConnector.spec_window_range(10, 0)
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------------------- the mask words
def _visible(tree, base, n_new, W):
    """brute force: per node the set of held positions it sees -- itself and its ancestors while alive, the `base` positions in front,
    each only if its absolute position lies in the node's window (held position t < base sits at -(base - t), node a at depth(a))"""
    depth, alive, out = [], [], []
    for j, p in enumerate(tree):
        depth.append(0 if p < 0 else depth[p] + 1)
        alive.append(j < n_new and (p < 0 or alive[p]))
        if not alive[j]:
            out.append(set())
            continue
        path, a = [], j
        while a >= 0:
            path.append(a)
            a = tree[a]
        at = {base + a: depth[a] for a in path}
        at.update({t: t - base for t in range(base)})
        out.append({t for t, pos in at.items() if W is None or depth[j] - pos < W})
    return out


def test_tree_masks_under_a_window_against_a_brute_force_visible_set():
    chains = [list(range(-1, S - 1)) for S in (1, 2, 5, 16)]
    for tree in chains + [list(t) for t in TREES]:
        S = len(tree)
        for base in (0, 1):
            for n_new in sorted({S, S - 1, S // 2, 0}):
                if n_new < 0:
                    continue
                today = SpeckvKVConnector.tree_masks(tree, [base], [n_new])
                assert SpeckvKVConnector.tree_masks(tree, [base], [n_new], window=None) == today == SpeckvKVConnector.tree_masks(tree, [base], [n_new], window=0)
                assert today[0] == [sum(1 << t for t in seen) for seen in _visible(tree, base, n_new, None)]
                for W in range(1, 21):
                    words = SpeckvKVConnector.tree_masks(tree, [base], [n_new], window=W)
                    assert words[0] == [sum(1 << t for t in seen) for seen in _visible(tree, base, n_new, W)], (tree, base, n_new, W)
                    if W >= 17:
                        assert words == today
    # one tree per request, ragged, and the rule in the issue's words: ancestors of depth >= d + 1 - W, the tail iff d + 2 <= W
    words = SpeckvKVConnector.tree_masks([TREES[0], [-1, 0, 1, 2, 3, 4, 5]], [1, 0], [7, 4], window=3)
    assert words[0] == [0b11, 0b111, 0b1110, 0b11100, 0b100011, 0b1100010, 0b11100000] and words[1] == [0b1, 0b11, 0b111, 0b1110, 0, 0, 0]
    with pytest.raises(ValueError):
        SpeckvKVConnector.tree_masks([-1, 0], [0], window=-1)


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _Recording(_RecordingLib):
    def attend_kv_spec_window(self, k_handles, v_handles, layer, d_q, g, rpp, pos_end, length, d_depth, window, d_k, d_v, seq_stride, pos_stride, d_mask,
                              mask_stride, sm_scale, d_out, d_lse, stream):
        B = len(pos_end)
        seen = dict(q=_read_f16(d_q, B * H * g * D).reshape(B, H, g, D), k=_read_f16(d_k, B * seq_stride).reshape(B, -1, H, D),
                    v=_read_f16(d_v, B * seq_stride).reshape(B, -1, H, D), words=[_read_u32(d_mask + 4 * mask_stride * b, g // rpp) for b in range(B)],
                    depths=[_read_u32(d_depth + 4 * mask_stride * b, g // rpp) for b in range(B)])
        self.calls.append(("attend_kv_spec_window", k_handles, v_handles, layer, d_q, g, rpp, pos_end, length, d_depth, window, d_k, d_v, seq_stride, pos_stride,
                           d_mask, mask_stride, sm_scale, d_out, d_lse, stream, seen))


def _connector(torch, lengths):
    lib = _Recording()
    conn = SpeckvSplitKVConnector(lib, L, H, D, T)
    for b, n in enumerate(lengths):
        conn.add_request(10 + b)
        r = conn.requests[10 + b]
        r.length = n
        if n & 1:
            r.tail_k, r.tail_v = torch.randn((L, H, D)).to(torch.float16), torch.randn((L, H, D)).to(torch.float16)
    return lib, conn


@pytest.mark.parametrize("S,R,n_new,parents,W", [(4, 4, None, None, 33), (5, 4, None, None, 3), (3, 8, [3, 0, 2, 1, 3, 2], None, 2), (16, 1, None, None, 9),
                                                 (5, 4, [5, 2, 0, 4, 5, 1], TREES[1], 3), (7, 4, None, TREES[0], 2), (5, 2, None, TREES[1], 100)])
def test_attend_spec_under_a_window_is_one_call_per_group_and_nothing_else(monkeypatch, S, R, n_new, parents, W):
    """lengths mixing odd and even: exactly len(spec_groups(S, R)) attend_kv_spec_window calls and no other library call; the depth table and
    the words on the device equal chunk_tree_depths and tree_masks(window=W); every group reads both from + j0 with stride S; length is
    the committed length, pos_end its even part; the held rows are attend_spec's; no state moves"""
    torch, st = _cpu_torch(monkeypatch)
    lengths = (0, 1, 2, 37, 36, 5)
    lib, conn = _connector(torch, lengths)
    B, layer, sm = len(lengths), 2, 0.125
    rids = [10 + b for b in range(B)]
    q, k_new, v_new = _step(torch, B, S, R)
    out = conn.attend_spec(layer, rids, q, k_new, v_new, sm, n_new=n_new, stream=st, parents=parents, window=W)
    assert tuple(out.shape) == (B, S, H, R, D) and out.dtype == torch.float32
    groups = SpeckvKVConnector.spec_groups(S, R)
    assert [c[0] for c in lib.calls] == ["attend_kv_spec_window"] * len(groups)
    reqs = [conn.requests[r] for r in rids]
    base = [n & 1 for n in lengths]
    tree = parents if parents is not None else list(range(-1, S - 1))
    words = SpeckvKVConnector.tree_masks(tree, base, n_new, window=W)
    depths = SpeckvKVConnector.chunk_tree_depths(tree, B)
    if parents is None:
        assert depths == [list(range(S))] * B
    first = lib.calls[0]
    for (j0, n), call in zip(groups, lib.calls):
        (_, k_handles, v_handles, at_layer, d_q, g, rpp, pos_end, length, d_depth, window, d_k, d_v, seq_stride, pos_stride, d_mask, mask_stride, scale, d_out,
         d_lse, stream, seen) = call
        assert [int(h) for h in k_handles] == [r.k_handle for r in reqs] and [int(h) for h in v_handles] == [r.v_handle for r in reqs]
        assert at_layer == layer and g == n * R and rpp == R and window == W
        assert [int(p) for p in pos_end] == [x & ~1 for x in lengths] and [int(p) for p in length] == list(lengths)
        assert (seq_stride, pos_stride, mask_stride, scale, stream) == ((1 + S) * ROW, ROW, S, sm, st.cuda_stream) and not d_lse
        assert (d_k, d_v) == (first[11], first[12]) and d_mask == first[15] + 4 * j0 and d_depth == first[9] + 4 * j0      # one gather and one table of each per step
        for b, r in enumerate(reqs):
            assert seen["words"][b] == words[b][j0:j0 + n] and seen["depths"][b] == depths[b][j0:j0 + n]
            assert np.array_equal(seen["q"][b].reshape(H, n, R, D), q[b, j0:j0 + n].permute(1, 0, 2, 3).numpy())
            for got, new, tail in ((seen["k"][b], k_new, r.tail_k), (seen["v"][b], v_new, r.tail_v)):
                assert got.shape == (1 + S, H, D)
                if base[b]:
                    assert np.array_equal(got[0], tail[layer].numpy())
                assert np.array_equal(got[base[b]:base[b] + S], new[b, :, layer].numpy())
    assert [conn.length(r) for r in rids] == list(lengths)
    # the next layer of the same step: the tables and the handle arrays are reused; a global layer of the same step derives its own
    del lib.calls[:]
    conn.attend_spec(layer + 1, rids, q, k_new, v_new, sm, n_new=n_new, stream=st, parents=parents, window=W)
    assert [c[0] for c in lib.calls] == ["attend_kv_spec_window"] * len(groups) and lib.calls[0][15] == first[15] and lib.calls[0][9] == first[9]
    assert lib.calls[0][1] is first[1]


def test_no_window_issues_todays_calls(monkeypatch):
    """window=None and window=0: attend_kv_spec calls with today's arguments -- the unwindowed words, no depth table -- and nothing else"""
    torch, st = _cpu_torch(monkeypatch)
    lengths = (0, 1, 2, 37, 36, 5)
    S, R = 5, 4
    q, k_new, v_new = _step(torch, len(lengths), S, R)
    seen = []
    for how in (dict(), dict(window=None), dict(window=0)):
        lib, conn = _connector(torch, lengths)
        conn.attend_spec(1, [10 + b for b in range(len(lengths))], q, k_new, v_new, 0.25, stream=st, parents=TREES[1], **how)
        assert [c[0] for c in lib.calls] == ["attend_kv_spec"] * 2
        seen.append([(c[3], c[5], c[6], [int(p) for p in c[7]], c[10], c[11], c[13], c[14], c[17], c[18]["words"]) for c in lib.calls])
        assert [c[18]["words"][3] for c in lib.calls] == [SpeckvKVConnector.tree_masks(TREES[1], [1])[0][:4], SpeckvKVConnector.tree_masks(TREES[1], [1])[0][4:]]
    assert seen[0] == seen[1] == seen[2]


def test_bad_arguments_raise_before_any_call(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, (4, 7))
    rids = [10, 11]
    q, k_new, v_new = _step(torch, 2, 4, 4)
    bad = [dict(window=-1), dict(window=1.5), dict(window=2 ** 32), dict(window="3"), dict(q=q[0]), dict(k_new=k_new[:, :3]), dict(layer=L), dict(n_new=[5, 0]),
           dict(parents=[-1, 0, 3, 1]), dict(parents=[-1, 0, 1])]
    for change in bad:
        args = dict(layer=0, req_ids=rids, q=q, k_new=k_new, v_new=v_new, sm_scale=1.0, stream=st, window=8)
        args.update(change)
        with pytest.raises((ValueError, TypeError)):
            conn.attend_spec(**args)
    with pytest.raises(KeyError):
        conn.attend_spec(0, [10, 99], q, k_new, v_new, 1.0, stream=st, window=8)
    assert lib.calls == []

    def refuse(*a):
        raise SpeckvError(ENTRY, -4)
    lib.attend_kv_spec_window = refuse
    with pytest.raises(SpeckvError) as e:                                          # no silent fall-back to the chunk walk
        conn.attend_spec(0, rids, q, k_new, v_new, 1.0, stream=st, window=8)
    assert e.value.status == -4 and lib.calls == []


# ------------------------------------------------------------------------------------------------ the kernel's scheme, in float64
def _scheme(K, kscale, nib, code, q, depths, begin, rel, n_pages, sm, cut):
    """k_attend_k8v4<true, true> for one kv head in float64: tiles of 32 positions from `begin`; per tile the scores of all 16 rows, row r
    masked below its skip (spec_window_skip) by a select, pages past n_pages masked with their code dropped; a page's E8M0 code is
    dropped where 2 page + 2 <= cut (the kernel: cut = depth 0's bound); V = nibble value x 2^(code - 127) (code 0: x 0.0 as the bit
    pattern the kernel builds; code 255: NaN); out += P^T . V as ONE product over the tile's 32 positions for all rows, weights of
    exactly 0 included -- a NaN or inf value there poisons the row."""
    G = len(q)
    m, l, acc = np.full(G, -np.inf), np.zeros(G), np.zeros((G, D))
    skip = np.asarray([SpeckvKVConnector.spec_window_skip(rel, d) for d in depths])
    for tile in range((n_pages + 15) // 16):
        idx = np.arange(32 * tile, 32 * tile + 32)                                  # position index within the walk
        pos = begin + idx
        with np.errstate(invalid="ignore", over="ignore"):
            s = (q @ K[pos].T) * np.repeat(kscale[pos[::2] // 2], 2)[None, :] * sm     # [G][32], NaN where the record is hostile
        codes = code[pos[::2] // 2].astype(np.int64).copy()
        past = idx // 2 >= n_pages
        s[:, past] = -np.inf
        codes[past[::2]] = 0
        s = np.where(idx[None, :] < skip[:, None], -np.inf, s)
        codes[idx[::2] + 2 <= cut] = 0
        scale = np.where(codes == 0, 0.0, np.where(codes == 255, np.nan, np.exp2(codes - 127.0)))
        V = nib[pos] * np.repeat(scale, 2)[:, None]
        m_new = np.maximum(m, s.max(axis=1))
        m_use = np.where(np.isneginf(m_new), 0.0, m_new)
        f, p = np.exp(m - m_use), np.exp(s - m_use[:, None])
        l, m = l * f + p.sum(axis=1), m_new
        with np.errstate(invalid="ignore"):
            acc = acc * f[:, None] + np.einsum("gj,jd->gd", p, V)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(l[:, None] > 0, acc / l[:, None], 0.0), np.where(l > 0, m + np.log(l), -np.inf)


def test_scores_are_masked_per_row_and_codes_dropped_only_below_depth_0():
    """one kv head, 16 rows of depths 0..15, lengths whose rel is positive, negative and beyond a tile; every page wholly in front of lo(0)
    holds a hostile record (code 255, NaN key bytes, NaN key scale).  The kernel's scheme -- codes dropped below depth 0's bound only --
    gives finite rows equal to the softmax over each row's visible set.  The trap: dropping codes by a DEEPER row's bound (its own skip, as
    the single-row windowed instance does) silently zeroes stored records a shallower row still reads -- further than the tolerance."""
    rng = np.random.default_rng(4711)
    sm = 1.0 / np.sqrt(D)
    fp4 = np.asarray([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])
    depths = list(range(16))
    trapped = 0
    for length, W in ((61, 33), (60, 33), (97, 33), (20, 28), (66, 15), (100, 15), (254, 40), (33, 40)):
        stored = length & ~1
        begin, rel, n_pages = SpeckvKVConnector.spec_window_range(length, W)
        lo0 = max(0, length + 1 - W)
        n = 256
        K = rng.standard_normal((n, D))
        kscale = rng.uniform(0.5, 2.0, n // 2)
        nib = fp4[rng.integers(0, 16, (n, D))]
        code = rng.integers(124, 131, n // 2)
        for page in range(lo0 // 2):                                                 # wholly in front of every row's window
            K[2 * page:2 * page + 2], kscale[page], code[page] = np.nan, np.nan, 255
        q = rng.standard_normal((16, D))
        out, lse = _scheme(K, kscale, nib, code, q, depths, begin, rel, n_pages, sm, cut=max(0, rel))
        assert np.isfinite(out).all() and not np.isnan(lse).any(), (length, W)
        want, tol = np.zeros((16, D)), np.full((16, D), 1e-6)
        for r, d in enumerate(depths):
            lo = max(0, length + d + 1 - W)
            if lo >= stored:
                assert not out[r].any() and lse[r] == -np.inf, (length, W, r)     # a row that sees nothing
                continue
            s = (K[lo:stored] @ q[r]) * np.repeat(kscale, 2)[lo:stored] * sm
            V = nib[lo:stored] * np.repeat(np.exp2(code - 127.0), 2)[lo:stored, None]
            p = np.exp(s - s.max())
            want[r] = (p @ V) / p.sum()
            delta = 3e-5 * float((np.abs(K[lo:stored]) @ np.abs(q[r])).max()) * sm
            tol[r] = (2e-3 + 2 * delta) * ((p @ np.abs(V)) / p.sum()) + 1e-6
            assert abs(lse[r] - (s.max() + np.log(p.sum()))) < 1e-9
        assert np.allclose(out, want, rtol=1e-9, atol=1e-12), (length, W)
        # the trap: codes dropped by the deepest row's bound
        deep = SpeckvKVConnector.spec_window_skip(rel, 15)
        if deep > max(0, rel) + 1 and n_pages:
            wrong, _ = _scheme(K, kscale, nib, code, q, depths, begin, rel, n_pages, sm, cut=deep)
            assert np.isfinite(wrong).all()
            assert (np.abs(wrong[0] - want[0]) > tol[0]).any() and (np.abs(wrong[0] - want[0]) / tol[0]).max() > 10.0, (length, W)
            trapped += 1
    assert trapped >= 5
