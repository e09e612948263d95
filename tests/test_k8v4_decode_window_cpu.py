"""Not -m gpu: the split pool's decode route under a sliding window -- the declaration of speckv_ext_attend_kv_batch_window, its export
and binding, its answer on an engine without a device, what SpeckvSplitKVConnector.attend(window=W) hands the library (against a
recording library), the walk rule of the connector against the library's over the lengths and windows of the GPU suite, and a numpy
restatement of k_attend_k8v4<true>'s masked tile 0 (csrc/attend_kv.hip) over hostile content, which shows that the kernel's scheme --
fp16 weights, the code of a page masked in both positions zeroed, the code of a page cut by an odd bound kept -- stays inside the
project's bound on such inputs, and that a mask one position off, or a cut page without its code, does not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_accuracy, speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_k8v4_decode_cpu import _RecordingLib, _connector, H, D, L, ROW
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "speckv_ext_attend_kv_batch_window"
LENGTHS = [1, 2, 33, 64, 65, 98, 131, 255, 256]          # batches A and B of tests/test_gpu_k8v4_decode_window.py
WINDOWS = [1, 2, 31, 32, 33, 64, 100, 300]


# ------------------------------------------------------------------------------------------------------------- the declaration
def test_the_entry_is_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    mine, plain = _declared(header, ENTRY), _declared(header, "speckv_ext_attend_kv_batch")
    assert mine == plain.replace("const uint32_t* pos_end, ", "const uint32_t* pos_end, const uint32_t* q_pos, uint32_t window, ")      # `q_pos, window` directly behind pos_end
    assert _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]            # the binding is the declaration
    assert ENTRY in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("/* %s:" % ENTRY):header.index("speckv_status_t %s(" % ENTRY)])     # the comment as running text
    for said in ("speckv_ext_attend_batch_window", "speckv_ext_decode_window_range", "exactly the launches of speckv_ext_attend_kv_batch",
                 "zeros and lse = -inf", "speckv_ext_attend_fold_tail", "NOT capturable", "SPECKV_ERR_INVAL", "NULL q_pos with window != 0"):
        assert said in text, said


def test_the_library_exports_the_entry_at_version_6():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, ENTRY)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    assert callable(pkg.SpeckvLib.attend_kv_batch_window)


def test_the_entry_on_the_null_engine_has_no_data_path():
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = []
        for call in (lambda: lib.attend_kv_batch_window([h], [h], 0, at, 8, [32], [31], 16, 0.1, at, None, 1),
                     lambda: lib.attend_kv_batch_window(np.asarray([h], np.uint64), np.asarray([h], np.uint64), 0, at, 8, np.asarray([32], np.uint32),
                                                        np.asarray([32], np.uint32), 1, 0.1, at, at, 1),
                     lambda: lib.attend_kv_batch_window([h], [h], 0, at, 8, [32], None, 0, 0.1, at, None, 1)):
            with pytest.raises(SpeckvError) as e:
                call()
            status.append(e.value.status)
        assert status == [-2, -2, -2]                                          # SPECKV_ERR_DRIVER: no data path
        assert not buf.any()
    finally:
        lib.finalize()


# ------------------------------------------------------------------------------------------------ what the connector hands over
class _WindowLib(_RecordingLib):
    def attend_kv_batch_window(self, k_handles, v_handles, layer, d_q, g, pos_end, q_pos, window, sm_scale, d_out, d_lse, stream):
        self.calls.append(("attend_kv_batch_window", [int(h) for h in k_handles], [int(h) for h in v_handles], layer, d_q, g, [int(p) for p in pos_end],
                           [int(p) for p in q_pos], window, sm_scale, d_out, d_lse, stream))


def _window_connector(torch, lengths):
    lib, conn = _connector(torch, lengths)
    conn.lib = win = _WindowLib()
    win.handles = lib.handles
    return win, conn


@pytest.mark.parametrize("lengths", [(0, 1, 2, 37, 36, 5), (3, 5), (7,), (64, 2, 36)])
@pytest.mark.parametrize("window", [1, 33])
def test_attend_under_a_window_is_one_window_call_and_at_most_one_fold(monkeypatch, lengths, window):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _window_connector(torch, lengths)
    B, G, layer = len(lengths), 4, 2
    rids = [10 + b for b in range(B)]
    q = torch.randn((B, H, G, D)).to(torch.float16)
    out = conn.attend(layer, rids, q, 0.125, stream=st, window=window)
    assert tuple(out.shape) == (B, H, G, D) and out.dtype == torch.float32
    odd = [b for b, n in enumerate(lengths) if n & 1]
    assert [c[0] for c in lib.calls] == ["attend_kv_batch_window"] + (["attend_fold_tail"] if odd else [])
    call = lib.calls[0]
    reqs = [conn.requests[r] for r in rids]
    assert call[1] == [r.k_handle for r in reqs] and call[2] == [r.v_handle for r in reqs]
    assert call[3] == layer and call[4] == q.data_ptr() and call[5] == G
    assert call[6] == [n & ~1 for n in lengths]                                # pos_end: the stored positions
    assert call[7] == [max(n, 1) - 1 for n in lengths]                         # q_pos = length - 1 (a request of length 0: 0 with pos_end 0)
    assert all(p - 1 <= qp <= p or (p == 0 and qp == 0) for p, qp in zip(call[6], call[7]))      # what the entry accepts
    assert call[8] == window and call[9] == 0.125 and call[10] == out.data_ptr() and call[11] not in (0, None) and call[12] == st.cuda_stream
    if odd:
        fold = lib.calls[1]
        assert fold[1] == len(odd) and fold[3:6] == (H, G, q.data_ptr()) and fold[8] == L * ROW and fold[9] == 0.125
        assert fold[10] == out.data_ptr() and fold[11] == call[11] and fold[12] == st.cuda_stream
        _, tk, tv = conn._step_tails(rids, reqs)
        assert fold[6] == tk.data_ptr() + 2 * layer * ROW and fold[7] == tv.data_ptr() + 2 * layer * ROW
    assert [conn.length(r) for r in rids] == list(lengths)                     # no state moved
    # the global layer of the same step: today's call over the same cached arrays, then the local layer again
    del lib.calls[:]
    conn.attend(layer + 1, rids, q, 0.125, stream=st)
    conn.attend(layer, rids, q, 0.125, stream=st, window=None)
    conn.attend(layer, rids, q, 0.125, stream=st, window=0)
    conn.attend(layer, rids, q, 0.125, stream=st, window=window)
    names = [c[0] for c in lib.calls if c[0] != "attend_fold_tail"]
    assert names == ["attend_kv_batch"] * 3 + ["attend_kv_batch_window"]
    assert lib.calls[0][6] == call[6] and [c for c in lib.calls if c[0] == "attend_kv_batch_window"][0][7] == call[7]


def test_attend_judges_the_window_before_any_call(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _window_connector(torch, (4, 6))
    q = torch.zeros((2, H, 4, D), dtype=torch.float16)
    for bad in (-1, 1.5, 2 ** 32, "8"):
        with pytest.raises((ValueError, TypeError)):
            conn.attend(0, [10, 11], q, 1.0, stream=st, window=bad)
    assert lib.calls == []

    def refuse(*a):
        raise SpeckvError(ENTRY, -4)
    lib.attend_kv_batch_window = refuse
    with pytest.raises(SpeckvError) as e:                                      # no silent fall-back to the chunk walk
        conn.attend(0, [10, 11], q, 1.0, stream=st, window=4)
    assert e.value.status == -4 and lib.calls == []


def test_the_class_docstring_no_longer_lists_the_window_as_not_built():
    from cxl_speckv_amd import kv_split_connector
    assert "sliding windows on attend" not in kv_split_connector.__doc__ and "speckv_ext_attend_kv_batch_window" in kv_split_connector.__doc__


# ------------------------------------------------------------------------------------------------------------- the range rule
def test_the_connectors_range_rule_is_the_librarys():
    lib = C.CDLL(pkg.build_library())
    speckv_ctypes.bind_ext(lib)
    for length in LENGTHS + [0, 3, 97]:
        for window in WINDOWS + [0]:
            b, k, n = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
            assert lib.speckv_ext_decode_window_range(length, window, C.byref(b), C.byref(k), C.byref(n)) == 0
            assert (b.value, k.value, n.value) == SpeckvKVConnector.decode_window_range(length, window), (length, window)
            assert b.value % 32 == 0 and k.value < 32 and (b.value // 2) % 16 == 0      # the descriptor starts on a storage tile of 16 records


# ------------------------------------------------------------------------------- the masked tile 0, restated in numpy
T = 256
K_HOSTILE, V_HOSTILE = 200.0, 1000.0
SM = 1.0 / np.sqrt(D)
G = 8
MUTATIONS = ("none", "skip + 1", "skip - 1", "a cut page loses its code")
CASES = [(length, window) for length in (33, 64, 65, 98, 131, 255, 256) for window in (2, 31, 33, 100)]


def _content(lo, stored, needle, seed, front=True):
    """q [G][D], k, v [T][H][D] fp16: ordinary rows (randn x U(0.2, 3) per position) in [lo, stored), hostile rows (K x 200, V = +-1000: the
    content of the GPU suite) below lo and at or behind stored; needle: position lo's K lies along the queries, nearly all the weight;
    front = False: the rows below lo are ordinary ones, as in a served request -- a page cut by an odd lo then holds its kept position at
    full precision (beside V = +-1000 the block's step is 64 and an ordinary kept value is stored as 0: the page's code carries nothing)"""
    rng = np.random.default_rng(seed)
    k = rng.standard_normal((T, H, D)) * rng.uniform(0.2, 3.0, (T, 1, 1))
    v = rng.standard_normal((T, H, D)) * rng.uniform(0.2, 3.0, (T, 1, 1))
    out = np.ones(T, bool)
    out[lo:stored] = False
    if not front:
        out[:lo] = False
    k[out] *= K_HOSTILE
    v[out] = np.sign(v[out]) * V_HOSTILE
    u = np.sign(rng.standard_normal(D))
    q = rng.standard_normal((G, D)) * 1.5
    if needle and lo < stored:
        k[lo, 0] = 1.2 * u
        q = u + 0.3 * rng.standard_normal((G, D))
    return q.astype(np.float16), k.astype(np.float16), v.astype(np.float16)


def _restate(q16, k16, v16, length, window, mutation):
    """k_attend_k8v4<true> over kv head 0 of one member: the query as E4M3 x a row scale, K as the FP8 pool holds it, V as the MXFP4 pool
    holds it (elements x 2^(code - 127), one code per page and block of 16 channels); tiles of 32 positions from `begin`; the first
    `skip` positions of tile 0 and the pages at or beyond `stored` score -inf; a page masked in BOTH positions takes code 0 (its
    elements x 2^-127), a page CUT by an odd skip keeps its code; online softmax, the weights rounded to fp16 in front of the V
    product, their sum taken unrounded."""
    begin, skip, n_pages = SpeckvKVConnector.decode_window_range(length, window)
    if mutation == "skip + 1": skip += 1
    elif mutation == "skip - 1": skip -= 1
    qe = kv_accuracy.quantize_query_e4m3(q16)
    K = kv_accuracy.quantize_fp8_e4m3(k16)[:, 0]                                # [T][D] float64
    V = kv_accuracy.quantize_mxfp4(v16)[:, 0]
    code = np.repeat(np.repeat(kv_accuracy.mxfp4_codes(v16)[:, :D // 16], 16, axis=1), 2, axis=0)      # [T][D]: the code a position's channel is stored under
    m, l, acc = np.full(G, -np.inf), np.zeros(G), np.zeros((G, D))
    for tile in range((n_pages + 15) // 16):
        pos = begin + 32 * tile + np.arange(32)
        page = (pos - begin) // 2
        masked = page >= n_pages
        if tile == 0:
            masked = masked | (pos - begin < skip)
        dead = np.repeat(masked.reshape(16, 2).all(axis=1), 2)                   # both positions of the page masked
        if mutation == "a cut page loses its code":
            dead = np.repeat(masked.reshape(16, 2).any(axis=1), 2)
        s = np.where(masked[None], -np.inf, ((qe @ K[pos].T) * SM).astype(np.float32).astype(np.float64))
        vt = np.where(dead[:, None], np.ldexp(V[pos], -code[pos]), V[pos])       # code 0: the elements x 2^-127 -- small and finite
        assert np.isfinite(vt).all()
        m_new = np.maximum(m, s.max(axis=1))
        if not np.isfinite(m_new).all():                                         # a tile masked throughout (a mutation's doing): no row comes of it
            return np.full((G, D), np.nan), np.full(G, np.nan)
        f = np.where(np.isfinite(m), np.exp(m - m_new), 0.0)
        p = np.exp(s - m_new[:, None])
        l = l * f + p.sum(axis=1)
        acc = acc * f[:, None] + p.astype(np.float16).astype(np.float64) @ vt
        m = m_new
    if n_pages == 0:
        return np.zeros((G, D)), np.full(G, -np.inf)
    return acc / l[:, None], m + np.log(l)


def _reference(q16, k16, v16, lo, stored):
    """float64 attention over the records of exactly [lo, stored): out, lse, sum p|v|, delta"""
    qe = kv_accuracy.quantize_query_e4m3(q16)
    K, V = kv_accuracy.quantize_fp8_e4m3(k16)[lo:stored, 0], kv_accuracy.quantize_mxfp4(v16)[lo:stored, 0]
    s = (qe @ K.T) * SM
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return (p @ V) / l[:, None], mx + np.log(l), (p @ np.abs(V)) / l[:, None], 3e-5 * float((np.abs(qe) @ np.abs(K).T).max()) * SM


def test_the_masked_tile_0_restated_in_numpy_keeps_the_bound_over_hostile_content():
    """The kernel's scheme holds |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6 and lse within 2e-3 + delta on every case -- the inputs, not the
    kernel, keep the reference within tolerance -- and each mutation of the mask leaves the bound on some case.  The cases hold odd and
    even skips, cut pages, a first tile that is the last one, and ragged last tiles."""
    caught = {mu: 0 for mu in MUTATIONS}
    worst, odd_skips = 0.0, 0
    for needle, front in ((False, True), (True, True), (True, False)):
        for length, window in CASES:
            lo, stored = max(0, length - window), length & ~1
            odd_skips += SpeckvKVConnector.decode_window_range(length, window)[1] & 1
            q, k, v = _content(lo, stored, needle, 7100 + 13 * length + window, front)
            want, wlse, mag, delta = _reference(q, k, v, lo, stored)
            tol = (2e-3 + 2 * delta) * mag + 1e-6
            for mu in MUTATIONS:
                got, lse = _restate(q, k, v, length, window, mu)
                ok = bool(np.all(np.abs(got - want) <= tol)) and bool(np.all(np.abs(lse - wlse) <= 2e-3 + delta))
                if mu == "none":
                    worst = max(worst, float((np.abs(got - want) / tol).max()), float((np.abs(lse - wlse) / (2e-3 + delta)).max()))
                    assert ok, ("the scheme as it stands", length, window, needle, float((np.abs(got - want) / tol).max()), front)
                elif not ok:
                    caught[mu] += 1
    print(f"masked tile 0 restated: worst err / tol {worst:.3f} over {3 * len(CASES)} cases ({odd_skips} with an odd skip); "
          + ", ".join(f"'{mu}' leaves the bound on {caught[mu]}" for mu in MUTATIONS[1:]))
    assert odd_skips >= 12
    for mu in MUTATIONS[1:]:
        assert caught[mu] > 0, (mu, "no case of the data tells it from the scheme")
