"""Not -m gpu: the split pool's multi-position step on the decode kernel -- the declaration of speckv_ext_attend_kv_spec, its answer on an
engine without a device and its refusals there, what SpeckvSplitKVConnector.attend_spec hands the library (against a recording library),
and a numpy float64 restatement of the step against a restatement of "speckv_ext_attend_kv_batch at g = S x R, then
speckv_ext_attend_fold_masked": the same function."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_accuracy, speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import HELD_MAX, SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "speckv_ext_attend_kv_spec"
L, H, D, T = 4, 8, 128, 64
ROW = H * D


# ------------------------------------------------------------------------------------------------------------- the declaration
def test_the_entry_is_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    mine = _declared(header, ENTRY)
    assert mine == ("uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles, uint32_t layer, const void* d_q_f16, "
                    "uint32_t g, uint32_t rows_per_pos, const uint32_t* pos_end, const void* d_k_held, const void* d_v_held, "
                    "uint64_t seq_stride_elems, uint64_t pos_stride_elems, const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, "
                    "float* d_out, float* d_lse, void* stream")
    assert _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]            # the binding is the declaration
    assert ENTRY in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    assert re.search(r"global:[^}]*\bspeckv_\*;", open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "exports.map")).read())
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("/* %s:" % ENTRY):header.index("speckv_status_t %s(" % ENTRY)])     # the comment as running text
    for said in ("INSIDE the same launch", "(1 << (base + j + 1)) - 1", "NO held position above the highest bit", "FP16 query", "NOT capturable",
                 "rows_per_pos == 0", "mask_stride < g / rows_per_pos", "pos_stride_elems < 8 * 128", "16-byte aligned", "SPECKV_EXT_ABI_VERSION stays"):
        assert said in text, said


def test_the_library_exports_the_entry_at_version_6():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, ENTRY)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    assert callable(pkg.SpeckvLib.attend_kv_spec)


def _null_call(lib, h, at, **change):
    args = dict(k_handles=[h], v_handles=[h], layer=0, d_q_f16=at, g=8, rows_per_pos=4, pos_end=[32], d_k_held=at, d_v_held=at, seq_stride_elems=3 * ROW,
                pos_stride_elems=ROW, d_mask=at, mask_stride=2, sm_scale=0.1, d_out=at, d_lse=None, stream=1)
    args.update(change)
    with pytest.raises(SpeckvError) as e:
        lib.attend_kv_spec(**args)
    return e.value.status


def test_the_entry_on_the_null_engine_answers_as_the_batch_entry_and_refuses_first():
    """a good set: SPECKV_ERR_DRIVER as speckv_ext_attend_kv_batch answers there (no data path); each refusal of the held rows and the mask
    is judged before anything else, so it is SPECKV_ERR_INVAL on this engine too; nothing is written"""
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        with pytest.raises(SpeckvError) as e:
            lib.attend_kv_batch([h], [h], 0, at, 8, [32], 0.1, at, None, 1)
        assert _null_call(lib, h, at) == e.value.status == -2                       # SPECKV_ERR_DRIVER
        assert _null_call(lib, h, at, d_lse=at) == -2
        for change in (dict(rows_per_pos=0), dict(rows_per_pos=3), dict(g=17, rows_per_pos=1, mask_stride=17), dict(g=HELD_MAX * 2, rows_per_pos=2, mask_stride=HELD_MAX),
                       dict(d_k_held=0), dict(d_v_held=0), dict(d_mask=0), dict(mask_stride=1), dict(seq_stride_elems=3 * ROW + 4), dict(pos_stride_elems=ROW + 4),
                       dict(pos_stride_elems=ROW - 8), dict(d_k_held=at + 8), dict(d_v_held=at + 2)):
            assert _null_call(lib, h, at, **change) == -4, change                    # SPECKV_ERR_INVAL
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _RecordingLib:
    def __init__(self):
        self.handles, self.calls = 0, []

    def set_compression_scheme(self, scheme): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def set_layout(self, *a): pass
    def free(self, h): pass

    def attend_kv_spec(self, k_handles, v_handles, layer, d_q, g, rpp, pos_end, d_k, d_v, seq_stride, pos_stride, d_mask, mask_stride, sm_scale, d_out,
                       d_lse, stream):
        """the arguments, and what the pointers show while the call runs: the query rows, the held rows of every sequence, its mask words"""
        B = len(pos_end)
        seen = dict(q=_read_f16(d_q, B * H * g * D).reshape(B, H, g, D), k=_read_f16(d_k, B * seq_stride).reshape(B, -1, H, D),
                    v=_read_f16(d_v, B * seq_stride).reshape(B, -1, H, D), words=[_read_u32(d_mask + 4 * mask_stride * b, g // rpp) for b in range(B)])
        self.calls.append(("attend_kv_spec", k_handles, v_handles, layer, d_q, g, rpp, pos_end, d_k, d_v, seq_stride, pos_stride, d_mask, mask_stride,
                           sm_scale, d_out, d_lse, stream, seen))

    def __getattr__(self, name):                                                   # any other library call is recorded under its name
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append((name,) + tuple(a))


def _connector(torch, lengths):
    lib = _RecordingLib()
    conn = SpeckvSplitKVConnector(lib, L, H, D, T)
    for b, n in enumerate(lengths):
        conn.add_request(10 + b)
        r = conn.requests[10 + b]
        r.length = n
        if n & 1:
            r.tail_k, r.tail_v = torch.randn((L, H, D)).to(torch.float16), torch.randn((L, H, D)).to(torch.float16)
    return lib, conn


def _step(torch, B, S, R):
    return (torch.randn((B, S, H, R, D)).to(torch.float16), torch.randn((B, S, L, H, D)).to(torch.float16), torch.randn((B, S, L, H, D)).to(torch.float16))


def _read_u32(ptr, n):
    return list((C.c_uint32 * n).from_address(ptr))


def _read_f16(ptr, n):
    return np.frombuffer((C.c_uint16 * n).from_address(ptr), dtype=np.float16).copy()


TREE = [-1, 0, 1, 0, 3]


@pytest.mark.parametrize("S,R,n_new,parents", [(4, 4, None, None), (5, 4, None, None), (3, 8, [3, 0, 2, 1, 3, 2], None), (16, 1, None, None),
                                               (5, 4, [5, 2, 0, 4, 5, 1], TREE), (5, 2, None, TREE)])
def test_attend_spec_is_one_call_per_group_and_nothing_else(monkeypatch, S, R, n_new, parents):
    """lengths mixing odd and even: exactly len(spec_groups(S, R)) attend_kv_spec calls and no other library call; the mask words on the
    device equal tree_masks (a chain is the tree [-1, 0, 1, ...]), every group reads them from d_mask + j0 with stride S; the held rows
    are the tail first where the length is odd, then the new positions, (1 + S) x H x D and H x D elements apart; no state moves"""
    torch, st = _cpu_torch(monkeypatch)
    lengths = (0, 1, 2, 37, 36, 5)
    lib, conn = _connector(torch, lengths)
    B, layer, sm = len(lengths), 2, 0.125
    rids = [10 + b for b in range(B)]
    q, k_new, v_new = _step(torch, B, S, R)
    out = conn.attend_spec(layer, rids, q, k_new, v_new, sm, n_new=n_new, stream=st, parents=parents)
    assert tuple(out.shape) == (B, S, H, R, D) and out.dtype == torch.float32
    groups = SpeckvKVConnector.spec_groups(S, R)
    assert [c[0] for c in lib.calls] == ["attend_kv_spec"] * len(groups)
    reqs = [conn.requests[r] for r in rids]
    base = [n & 1 for n in lengths]
    words = SpeckvKVConnector.tree_masks(parents if parents is not None else list(range(-1, S - 1)), base, n_new)
    if parents is None and n_new is None:
        assert words == [[(1 << (x + j + 1)) - 1 for j in range(S)] for x in base]
    first = lib.calls[0]
    for (j0, n), call in zip(groups, lib.calls):
        (_, k_handles, v_handles, at_layer, d_q, g, rpp, pos_end, d_k, d_v, seq_stride, pos_stride, d_mask, mask_stride, scale, d_out, d_lse, stream, seen) = call
        assert [int(h) for h in k_handles] == [r.k_handle for r in reqs] and [int(h) for h in v_handles] == [r.v_handle for r in reqs]
        assert at_layer == layer and g == n * R and rpp == R and [int(p) for p in pos_end] == [x & ~1 for x in lengths]
        assert (seq_stride, pos_stride, mask_stride, scale, stream) == ((1 + S) * ROW, ROW, S, sm, st.cuda_stream) and not d_lse
        assert (d_k, d_v) == (first[8], first[9]) and d_mask == first[12] + 4 * j0              # one held gather and one table per step
        for b, r in enumerate(reqs):
            assert seen["words"][b] == words[b][j0:j0 + n]
            # the query rows of the group: [batch][heads][n x R][dim]
            assert np.array_equal(seen["q"][b].reshape(H, n, R, D), q[b, j0:j0 + n].permute(1, 0, 2, 3).numpy())
            # the held rows of `layer`: the tail first where the length is odd, then the new positions
            for got, new, tail in ((seen["k"][b], k_new, r.tail_k), (seen["v"][b], v_new, r.tail_v)):
                assert got.shape == (1 + S, H, D)
                if base[b]:
                    assert np.array_equal(got[0], tail[layer].numpy())
                assert np.array_equal(got[base[b]:base[b] + S], new[b, :, layer].numpy())
    assert [conn.length(r) for r in rids] == list(lengths)
    # the next layer of the same step: the table and the handle arrays are reused
    del lib.calls[:]
    conn.attend_spec(layer + 1, rids, q, k_new, v_new, sm, n_new=n_new, stream=st, parents=parents)
    assert [c[0] for c in lib.calls] == ["attend_kv_spec"] * len(groups) and lib.calls[0][12] == first[12] and lib.calls[0][1] is first[1]


def test_attend_spec_refuses_before_any_call_and_lets_a_placement_refusal_through(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, (4, 7))
    rids = [10, 11]
    q, k_new, v_new = _step(torch, 2, 4, 4)
    bad = [dict(q=q[0]), dict(q=q[:1]), dict(q=q[:, :, :4]), dict(k_new=k_new[:, :3]), dict(v_new=v_new[:, :, :2]), dict(layer=L), dict(layer=-1),
           dict(n_new=[1]), dict(n_new=[5, 0]), dict(parents=[-1, 0, 1]), dict(parents=[-1, 0, 3, 1]), dict(parents=[[-1, 0, 1, 2]]),
           dict(q=torch.zeros((2, 17, H, 1, D), dtype=torch.float16), k_new=torch.zeros((2, 17, L, H, D), dtype=torch.float16),
                v_new=torch.zeros((2, 17, L, H, D), dtype=torch.float16)),
           dict(q=torch.zeros((2, 4, H, 17, D), dtype=torch.float16))]
    for change in bad:
        args = dict(layer=0, req_ids=rids, q=q, k_new=k_new, v_new=v_new, sm_scale=1.0, stream=st)
        args.update(change)
        with pytest.raises(ValueError):
            conn.attend_spec(**args)
    with pytest.raises(KeyError):
        conn.attend_spec(0, [10, 99], q, k_new, v_new, 1.0, stream=st)
    assert lib.calls == []

    def refuse(*a):
        raise SpeckvError(ENTRY, -4)
    lib.attend_kv_spec = refuse
    with pytest.raises(SpeckvError) as e:                                          # no silent fall-back to the chunk walk
        conn.attend_spec(0, rids, q, k_new, v_new, 1.0, stream=st)
    assert e.value.status == -4 and lib.calls == []


# ------------------------------------------------------------------------------------------------ the semantics, in float64
def _softmax_fold(out, lse, s, v):
    """the fold formula of speckv_ext_attend_fold_masked for one row: (out, lse) over some positions += the positions with scores s [n]
    and values v [n][D], all at once (hi = max(lse, s); den = exp(lse - hi) + sum exp(s - hi); ...)"""
    if len(s) == 0:
        return out, lse
    hi = max(lse, s.max())
    e_old, e = (np.exp(lse - hi) if np.isfinite(lse) else 0.0), np.exp(s - hi)
    den = e_old + e.sum()
    return (out * e_old + e @ v) / den, hi + np.log(den)


def test_the_step_is_the_batch_entry_at_g_rows_followed_by_the_masked_fold():
    """one kv head in numpy float64: speckv_ext_attend_kv_spec as the header states it -- ONE softmax per row over the stored positions
    (E4M3 query) and the visible held positions (fp16 query) -- against speckv_ext_attend_kv_batch at g = S x R (softmax over the stored
    positions, lse kept; zeros and -inf where nothing is stored) followed by the fold of speckv_ext_attend_fold_masked (a word of 0
    leaves the rows as they came in).  Odd and even lengths, an empty member, a ragged tree."""
    rng = np.random.default_rng(8128)
    S, R, sm = 5, 2, 1.0 / np.sqrt(D)
    for n_stored, base, n_new in ((0, 0, 5), (0, 1, 3), (2, 0, 0), (30, 1, 5), (64, 0, 2)):
        K, V = rng.standard_normal((n_stored, D)), rng.standard_normal((n_stored, D))
        q16 = rng.standard_normal((S * R, D)).astype(np.float16)
        kh, vh = rng.standard_normal((base + S, D)).astype(np.float16), rng.standard_normal((base + S, D)).astype(np.float16)
        words = SpeckvKVConnector.tree_masks(TREE, [base], [n_new])[0]
        q8, qf = kv_accuracy.quantize_query_e4m3(q16), q16.astype(np.float64)
        for r in range(S * R):
            seen = [t for t in range(base + S) if (words[r // R] >> t) & 1]
            s_stored, s_held = (K @ q8[r]) * sm, (kh[seen].astype(np.float64) @ qf[r]) * sm
            # the step: one softmax
            s, v = np.concatenate([s_stored, s_held]), np.concatenate([V, vh[seen].astype(np.float64)])
            if len(s):
                p = np.exp(s - s.max())
                one, one_lse = (p @ v) / p.sum(), s.max() + np.log(p.sum())
            else:
                one, one_lse = np.zeros(D), -np.inf
            # the two calls: the batch entry over the stored positions, then the fold
            two, two_lse = _softmax_fold(np.zeros(D), -np.inf, s_stored, V)
            two, two_lse = _softmax_fold(two, two_lse, s_held, vh[seen].astype(np.float64))
            assert np.allclose(one, two, rtol=1e-12, atol=1e-14) and (one_lse == two_lse or abs(one_lse - two_lse) < 1e-12), (n_stored, base, r)
            if not seen:                                                               # a dead row: the stored part alone
                alone = _softmax_fold(np.zeros(D), -np.inf, s_stored, V)
                assert np.array_equal(one, alone[0]) or np.allclose(one, alone[0], rtol=1e-12, atol=1e-14)
                if n_stored == 0:
                    assert not one.any() and one_lse == -np.inf
