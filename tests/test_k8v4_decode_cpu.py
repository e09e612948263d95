"""Not -m gpu: the split pool's decode route -- the declaration of speckv_ext_attend_kv_batch and its answer on an engine without a
device, the numpy restatement of the decode kernels' query quantisation against the oracle's, what the E4M3 query costs on KV-like data
(kv_accuracy.format_accuracy_cpu(query="e4m3")), and what SpeckvSplitKVConnector.attend hands the library, against a recording library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_accuracy, speckv_ctypes
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "speckv_ext_attend_kv_batch"


# ------------------------------------------------------------------------------------------------------------- the declaration
def test_the_entry_is_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    mine = _declared(header, ENTRY)
    assert mine == ("uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles, uint32_t layer, const void* d_q_f16, "
                    "uint32_t g, const uint32_t* pos_end, float sm_scale, float* d_out, float* d_lse, void* stream")
    assert _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]            # the binding is the declaration
    assert ENTRY in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    text = re.sub(r"\s*\n \*\s*", " ", header[header.index("/* %s:" % ENTRY):header.index("speckv_status_t %s(" % ENTRY)])     # the comment as running text
    for said in ("region `layer`", "E4M3 x a row scale", "block scale multiplies the score in fp32", "speckv_ext_fetch_range",
                 "NOT capturable", "SPECKV_ERR_INVAL", "SPECKV_ERR_GENERAL", "do not lie in one run"):
        assert said in text, said


def test_the_library_exports_the_entry_at_version_6():
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, ENTRY)
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert lib.speckv_ext_abi_version() == 6
    assert callable(pkg.SpeckvLib.attend_kv_batch)


def test_the_entry_on_the_null_engine_answers_as_the_fp8_batch_entry():
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = []
        for call in (lambda: lib.attend_fp8_batch([h], 0, at, 8, [32], 0.1, at, None, 1),
                     lambda: lib.attend_kv_batch([h], [h], 0, at, 8, [32], 0.1, at, None, 1),
                     lambda: lib.attend_kv_batch(np.asarray([h], np.uint64), np.asarray([h], np.uint64), 0, at, 8, np.asarray([32], np.uint32), 0.1, at, at, 1)):
            with pytest.raises(SpeckvError) as e:
                call()
            status.append(e.value.status)
        assert status == [-2, -2, -2]                                          # SPECKV_ERR_DRIVER: no data path
        assert not buf.any()
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------------------------------- the query in numpy
def _oracle_rows(oracle, q16):
    """the oracle's orc_quantize_rows_e4m3 of fp16 rows [R][D]: bytes and scales -> float64 values"""
    from oracle.bindings import _ptr, u8p, u16p, f32p
    q16 = np.ascontiguousarray(q16, np.float16)
    R, Dm = q16.shape
    q8, qs = np.zeros((R, Dm), np.uint8), np.zeros(R, np.float32)
    oracle.lib.orc_quantize_rows_e4m3(_ptr(q16.view(np.uint16).reshape(-1), u16p), R, Dm, _ptr(q8, u8p), _ptr(qs, f32p))
    lut = np.array([oracle.lib.orc_e4m3_to_f32(b) for b in range(256)], np.float64)
    assert not np.isnan(lut[q8]).any()
    return lut[q8] * qs.astype(np.float64)[:, None], q8, qs


def test_the_numpy_query_restatement_is_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(20262)
    rows = [rng.standard_normal((64, 128)).astype(np.float16), np.zeros((1, 128), np.float16)]
    big = (rng.standard_normal((1, 128)) * 0.01).astype(np.float16)
    big[0, 77] = 65504
    rows.append(big)
    for seed in (7001, 7002):
        _, _, qs, _ = kv_accuracy.synth_kv(64, 8, seed)
        rows += [qs[r].reshape(-1, 128) for r in kv_accuracy.REGIMES]
    q16 = np.concatenate(rows)
    want, q8, scales = _oracle_rows(oracle, q16)
    got = kv_accuracy.quantize_query_e4m3(q16)
    assert got.dtype == np.float64 and got.shape == q16.shape
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])] if len(bad) else None)
    assert scales[64] == 1.0 and not got[64].any()                             # the zero row: scale 1, values 0
    assert q8[65, 77] == 0x7E and got[65, 77] == 448.0 * float(scales[65])      # the row's maximum is 448 x the scale (fp32(65504 / 448))
    assert (got != q16.astype(np.float64)).any()                               # and no copy of the input
    # any leading shape
    again = kv_accuracy.quantize_query_e4m3(q16[:64].reshape(2, 4, 8, 128))
    assert np.array_equal(again.reshape(64, 128), got[:64])


# today's six numbers of format_accuracy_cpu("fp8_e4m3", "mxfp4") (fp16 query), per seed: peaky, decode, flat
PINNED = {7001: (0.13909761856604705, 0.21573484432981613, 0.13503974591695958),
          7002: (0.14515157704517942, 0.18779154995882907, 0.14064746585158078)}


@pytest.mark.parametrize("seed", [7001, 7002])
def test_the_e4m3_query_keeps_the_split_pool_under_the_bar(seed):
    """decode-regime rel. L2 <= 0.25 with the query as the decode kernel restates it (computed in numpy: 0.2162 / 0.1895; with the fp16
    query 0.2157 / 0.1878); without the keyword the function returns what it returned before"""
    plain = kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed)
    e4m3 = kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed, query="e4m3")
    print(f"seed {seed}: fp16 query {plain}, e4m3 query {e4m3}")
    assert tuple(plain[r] for r in ("peaky", "decode", "flat")) == pytest.approx(PINNED[seed], rel=1e-9)
    assert kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed, query="fp16") == plain
    assert set(e4m3) == set(kv_accuracy.REGIMES)
    assert e4m3["decode"] <= 0.25, e4m3
    assert e4m3 != plain                                                        # the keyword does something
    with pytest.raises(ValueError):
        kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed, query="int8")


# ------------------------------------------------------------------------------------------------ what the connector hands over
L, H, D, T = 4, 8, 128, 64
ROW = H * D


class _RecordingLib:
    def __init__(self):
        self.handles, self.calls, self.scheme = 0, [], None

    def set_compression_scheme(self, scheme): self.scheme = scheme

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def set_layout(self, *a): pass
    def free(self, h): pass

    def attend_kv_batch(self, k_handles, v_handles, layer, d_q, g, pos_end, sm_scale, d_out, d_lse, stream):
        self.calls.append(("attend_kv_batch", [int(h) for h in k_handles], [int(h) for h in v_handles], layer, d_q, g, [int(p) for p in pos_end],
                           sm_scale, d_out, d_lse, stream))

    def attend_fold_tail(self, n_rows, d_rows, heads, g, d_q, d_k_tail, d_v_tail, tail_stride, sm_scale, d_out, d_lse, stream):
        self.calls.append(("attend_fold_tail", n_rows, d_rows, heads, g, d_q, d_k_tail, d_v_tail, tail_stride, sm_scale, d_out, d_lse, stream))


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


@pytest.mark.parametrize("lengths", [(0, 1, 2, 37, 36, 5), (3, 5), (7,)])
def test_attend_is_one_batch_call_and_one_fold_over_the_odd_members(monkeypatch, lengths):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, lengths)
    B, G, layer = len(lengths), 4, 2
    rids = [10 + b for b in range(B)]
    q = torch.randn((B, H, G, D)).to(torch.float16)
    index = {}
    real_index = __import__("cxl_speckv_amd.kv_connector", fromlist=["x"])._device_index
    monkeypatch.setattr("cxl_speckv_amd.kv_connector._device_index", lambda v: index.setdefault("rows", real_index(v)))
    out = conn.attend(layer, rids, q, 0.125, stream=st)
    assert tuple(out.shape) == (B, H, G, D) and out.dtype == torch.float32
    assert [c[0] for c in lib.calls] == ["attend_kv_batch", "attend_fold_tail"]
    batch, fold = lib.calls
    reqs = [conn.requests[r] for r in rids]
    assert batch[1] == [r.k_handle for r in reqs] and batch[2] == [r.v_handle for r in reqs]
    assert batch[3] == layer and batch[4] == q.data_ptr() and batch[5] == G and batch[6] == [n & ~1 for n in lengths]
    assert batch[7] == 0.125 and batch[8] == out.data_ptr() and batch[9] not in (0, None) and batch[10] == st.cuda_stream
    odd = [b for b, n in enumerate(lengths) if n & 1]
    assert fold[1] == len(odd) and index["rows"].tolist() == odd and fold[2] == index["rows"].data_ptr()
    assert fold[3:6] == (H, G, q.data_ptr()) and fold[8] == L * ROW and fold[9] == 0.125
    assert fold[10] == out.data_ptr() and fold[11] == batch[9] and fold[12] == st.cuda_stream
    # the tail rows: the i-th odd member's rows of `layer`, L * H * D elements apart
    _, tk, tv = conn._step_tails(rids, reqs)
    assert fold[6] == tk.data_ptr() + 2 * layer * ROW and fold[7] == tv.data_ptr() + 2 * layer * ROW
    for i, b in enumerate(odd):
        assert torch.equal(tk[i], reqs[b].tail_k) and torch.equal(tv[i], reqs[b].tail_v)
    assert [conn.length(r) for r in rids] == list(lengths)                     # no state moved
    # the next layer of the same step: the same two calls, the index tensor reused
    del lib.calls[:]
    conn.attend(layer + 1, rids, q, 0.125, stream=st)
    assert [c[0] for c in lib.calls] == ["attend_kv_batch", "attend_fold_tail"] and lib.calls[1][2] == index["rows"].data_ptr()


def test_attend_without_an_odd_member_makes_no_fold_call(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, (0, 2, 36, 64))
    q = torch.randn((4, H, 1, D)).to(torch.float16)
    conn.attend(0, [10, 11, 12, 13], q, 0.5, stream=st)
    assert [c[0] for c in lib.calls] == ["attend_kv_batch"]
    assert lib.calls[0][6] == [0, 2, 36, 64]


def test_attend_refuses_shapes_before_any_call_and_lets_a_placement_refusal_through(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, (4, 6))
    ok = torch.zeros((2, H, 4, D), dtype=torch.float16)
    for bad in (torch.zeros((2, H, 17, D), dtype=torch.float16), torch.zeros((1, H, 4, D), dtype=torch.float16),
                torch.zeros((2, 4, 4, D), dtype=torch.float16), torch.zeros((2, 1, H, 4, D), dtype=torch.float16)):
        with pytest.raises(ValueError):
            conn.attend(0, [10, 11], bad, 1.0, stream=st)
    with pytest.raises(ValueError):
        conn.attend(L, [10, 11], ok, 1.0, stream=st)
    assert lib.calls == []

    def refuse(*a):
        raise SpeckvError("speckv_ext_attend_kv_batch", -4)
    lib.attend_kv_batch = refuse
    with pytest.raises(SpeckvError) as e:                                      # no silent fall-back to the chunk walk
        conn.attend(0, [10, 11], ok, 1.0, stream=st)
    assert e.value.status == -4 and lib.calls == []
