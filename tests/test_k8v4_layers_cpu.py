"""Not -m gpu: the split pool's decode step of several layers in one launch -- the declaration of speckv_ext_attend_kv_layers, its answer on an
engine without a device and the refusals the arguments alone decide, and what SpeckvSplitKVConnector.attend_layers hands the library
(against the recording library of tests/test_k8v4_spec_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_k8v4_spec_cpu import D, H, L, ROW, _connector, _read_f16
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "speckv_ext_attend_kv_layers"


def test_the_entry_is_declared_bound_exported_and_additive():
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in header
    mine = _declared(header, ENTRY)
    assert mine == ("uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles, uint32_t layer_begin, uint32_t n_layers, "
                    "const void* d_q_f16, uint32_t g, const uint32_t* pos_end, uint32_t n_tail, const int32_t* d_tail_idx, const void* d_k_tail, "
                    "const void* d_v_tail, uint64_t tail_stride_elems, float sm_scale, float* d_out, float* d_lse, void* stream")
    assert _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]            # the binding is the declaration
    assert ENTRY in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()
    lib = C.CDLL(pkg.build_library())
    lib.speckv_ext_abi_version.restype = C.c_uint32
    assert hasattr(lib, ENTRY) and lib.speckv_ext_abi_version() == 6


def test_the_null_engine_answers_as_the_batch_entry_and_the_arguments_are_judged_first():
    """a good set: SPECKV_ERR_DRIVER as speckv_ext_attend_kv_batch answers there; what the arguments alone decide is SPECKV_ERR_INVAL on this
    engine too; nothing is written"""
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h = lib.alloc(64 * 4096)
        buf = np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16

        def status(**change):
            args = dict(k_handles=[h], v_handles=[h], layer_begin=1, n_layers=2, d_q_f16=at, g=8, pos_end=[32], n_tail=1, d_tail_idx=at, d_k_tail=at,
                        d_v_tail=at, tail_stride_elems=4 * ROW, sm_scale=0.1, d_out=at, d_lse=None, stream=1)
            args.update(change)
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_layers(**args)
            return e.value.status
        with pytest.raises(SpeckvError) as e:
            lib.attend_kv_batch([h], [h], 0, at, 8, [32], 0.1, at, None, 1)
        assert status() == e.value.status == -2                                   # SPECKV_ERR_DRIVER
        assert status(n_tail=0, d_tail_idx=0, d_k_tail=0, d_v_tail=0, tail_stride_elems=0) == -2
        for change in (dict(g=0), dict(g=17), dict(n_layers=0), dict(pos_end=[33]), dict(d_q_f16=at + 8), dict(d_out=at + 4), dict(d_tail_idx=0),
                       dict(d_k_tail=0), dict(d_v_tail=0), dict(d_k_tail=at + 8), dict(d_v_tail=at + 2), dict(tail_stride_elems=4 * ROW + 4),
                       dict(tail_stride_elems=3 * ROW - 8)):
            assert status(**change) == -4, change                                  # SPECKV_ERR_INVAL
        assert not buf.any()
    finally:
        lib.finalize()


@pytest.mark.parametrize("lengths", [(0, 1, 2, 37, 36, 5), (4, 36)])
def test_attend_layers_is_one_call_with_the_step_derived_once(monkeypatch, lengths):
    """odd and even lengths, and even ones alone: exactly one attend_kv_layers call and no other; the handles, the stored lengths, the tail
    index and the stacked tails [tail][layers][heads][dim] as the connector keeps them; a second call of the step reuses them; no state moves"""
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, lengths)
    rids = [10 + b for b in range(len(lengths))]
    reqs = [conn.requests[r] for r in rids]
    q = torch.randn((3, len(rids), H, 4, D)).to(torch.float16)
    out = conn.attend_layers(1, 3, rids, q, 0.125, stream=st)
    assert tuple(out.shape) == tuple(q.shape) and out.dtype == torch.float32
    assert [c[0] for c in lib.calls] == ["attend_kv_layers"]
    _, kh, vh, begin, n_layers, d_q, g, pos_end, n_tail, d_idx, d_k, d_v, stride, sm, d_out, d_lse, stream = lib.calls[0]
    odd = [r for r in reqs if r.length & 1]
    assert [int(x) for x in kh] == [r.k_handle for r in reqs] and [int(x) for x in vh] == [r.v_handle for r in reqs]
    assert (begin, n_layers, g, n_tail, sm, d_out, stream) == (1, 3, 4, len(odd), 0.125, out.data_ptr(), st.cuda_stream) and not d_lse
    assert [int(p) for p in pos_end] == [n & ~1 for n in lengths]
    assert np.array_equal(_read_f16(d_q, q.numel()).reshape(q.shape), q.numpy())
    if odd:
        assert stride == L * ROW
        ranks = iter(range(len(odd)))
        assert list((C.c_int32 * len(reqs)).from_address(d_idx)) == [next(ranks) if r.length & 1 else -1 for r in reqs]
        for got, rows in ((d_k, [r.tail_k for r in odd]), (d_v, [r.tail_v for r in odd])):
            assert np.array_equal(_read_f16(got, len(odd) * L * ROW).reshape(len(odd), L, H, D), torch.stack(rows).numpy())
    else:
        assert (d_idx, d_k, d_v) == (0, 0, 0)
    conn.attend_layers(0, 1, rids, q[:1], 0.125, stream=st)
    assert len(lib.calls) == 2 and lib.calls[1][1] is kh and lib.calls[1][9] == d_idx and lib.calls[1][10] == d_k
    assert [conn.length(r) for r in rids] == list(lengths)


def test_attend_layers_refuses_a_bad_query_before_any_call(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    lib, conn = _connector(torch, (4, 7))
    q = torch.zeros((2, 2, H, 4, D), dtype=torch.float16)
    for change in (dict(q=q[0]), dict(q=q[:1]), dict(n_layers=3), dict(n_layers=0, q=q[:0]), dict(q=q[:, :1]), dict(q=q[:, :, :4]),
                   dict(q=torch.zeros((2, 2, H, 17, D), dtype=torch.float16)), dict(layer_begin=L - 1), dict(layer_begin=-1)):
        args = dict(layer_begin=0, n_layers=2, req_ids=[10, 11], q=q, sm_scale=1.0, stream=st)
        args.update(change)
        with pytest.raises(ValueError):
            conn.attend_layers(**args)
    with pytest.raises(KeyError):
        conn.attend_layers(0, 2, [10, 99], q, 1.0, stream=st)
    assert lib.calls == []
