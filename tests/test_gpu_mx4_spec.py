"""-m gpu: speckv_ext_attend_spec_mx4 (k_attend_mx4_spec: up to 16 query rows per kv head over ONE MXFP4 allocation in one pass over the records, the
held rows folded inside the launch) and SpeckvKVConnector.attend_spec(row_block=16) on top of it.  The step, the held rows, the float64 reference, the
bound and the lengths are tests/test_gpu_k8v4_spec.py's, imported; the pair is HeadChecker(oracle, MXFP4) for K and V alike, so the stored scores take the
query as its q_rows give it for this scheme (MXFP8 per 16 channels), the held scores the fp16 query.  Every (member, head, row) is compared, out and lse;
worst err / tol is printed before it is asserted.  L = 2, T = 256: the members are prefixes of one prompt, each in its own allocation."""
import contextlib
import ctypes

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_k8v4_decode as kd
from tests._gpu import D, H, HeadChecker, _hip_runtime, graph_capture, torch_mod
from tests.test_gpu_hostile_ranges import drop_engine, tuned
from tests.test_gpu_k8v4_spec import LENGTHS, TREE, _compare, _held, _rows_of, _step, _want
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
L, T, SM, PATTERN, MX4 = kd.L, kd.T, kd.SM, kd.PATTERN, 5
B, RIDS, EVEN = len(LENGTHS), list(range(len(LENGTHS))), [n & ~1 for n in LENGTHS]
_pairs = {}


@contextlib.contextmanager
def _pool(scheme="mxfp4", lengths=LENGTHS, prompt=None):
    """an engine and a connector of `scheme` whose request i holds the first lengths[i] positions of the prompt"""
    torch = torch_mod()
    drop_engine()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn, keep = SpeckvKVConnector(lib, L, H, D, T, scheme), []
        k, v = prompt if prompt is not None else kd._prompt()
        for rid, n in enumerate(lengths):
            conn.add_request(rid)
            if n:
                keep += conn.write_prefill(rid, *(torch.from_numpy(np.ascontiguousarray(a[:, :n])).cuda() for a in (k, v)))
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
    finally:
        lib.finalize()


def _pair(oracle, layer, tag="prompt", prompt=None):
    """HeadChecker over the MXFP4 records of the prompt's layer, as K and as V"""
    if (tag, layer) not in _pairs:
        k, v = prompt if prompt is not None else kd._prompt()
        even = k.shape[1] & ~1
        _pairs[tag, layer] = (HeadChecker(oracle, MX4, _region(k[layer, :even], v[layer, :even], T), T),) * 2
    return _pairs[tag, layer]


def _entry(lib, conn, layer, qg, R, kh, vh, words, out=None, rids=RIDS, **change):
    """speckv_ext_attend_spec_mx4 over what the connector holds -> (out, lse) as fp32 numpy; both start as the fill pattern"""
    torch = torch_mod()
    Bq, _, G, _ = qg.shape
    reqs = [conn.requests[r] for r in rids]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dk, dv, dm = dev(qg), dev(kh), dev(vh), dev(np.asarray(words, np.uint32).view(np.int32))
    out = torch.full((Bq, H, G, D), PATTERN, dtype=torch.int32, device="cuda") if out is None else out
    lse = torch.full((Bq, H, G), PATTERN, dtype=torch.int32, device="cuda")
    args = dict(handles=np.asarray([r.handle for r in reqs], np.uint64), layer=layer, d_q_f16=dq.data_ptr(), g=G, rows_per_pos=R,
                pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), d_k_held=dk.data_ptr(), d_v_held=dv.data_ptr(), seq_stride_elems=kh.shape[1] * H * D,
                pos_stride_elems=H * D, d_mask=dm.data_ptr(), mask_stride=dm.shape[1], sm_scale=SM, d_out=out.data_ptr(), d_lse=lse.data_ptr(),
                stream=torch.cuda.Stream().cuda_stream)
    _entry.last = dict(args)                                             # (the capture case of the refusals repeats the good set on a capturing stream)
    args.update(change)
    torch.cuda.synchronize()
    try:
        lib.attend_spec_mx4(**args)
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)


def _chain(S):
    return list(range(-1, S - 1))


def _chains(oracle, S, R, what, tuning=()):
    q5, k_new, v_new = _step(S, R)
    with _pool() as (lib, conn), tuned(tuning):
        for layer in range(L):
            kh, vh, base = _held(layer, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(_chain(S), base)
            out, lse = _entry(lib, conn, layer, _rows_of(q5), R, kh, vh, words)
            assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any()
            _compare(_want(_pair(oracle, layer), _rows_of(q5), R, EVEN, kh, vh, words), out, lse, f"attend_spec_mx4 {what} S {S} R {R} layer {layer}")


@pytest.mark.parametrize("S,R", [(4, 4), (2, 8), (16, 1), (3, 3), (1, 8)])
def test_chains_through_the_entry(oracle, S, R):
    """g = 16 full, g = 9 (rows 9..15 are zero columns), g = 8; nothing stored, odd tails, a ragged last tile, exactly one tile, 8 tiles"""
    _chains(oracle, S, R, "chain")


def test_a_tree_and_a_ragged_step_through_the_connector(oracle):
    """TREE at 4 rows per position (two groups) through attend_spec(row_block=16); layer 1 ragged: zeros and partial counts; no state moves"""
    torch = torch_mod()
    S, R, n_new = len(TREE), 4, (None, [7, 0, 5, 2, 7, 1, 6, 0, 3])
    q5, k_new, v_new = _step(S, R)
    with _pool() as (lib, conn):
        for layer in range(L):
            got = conn.attend_spec(layer, RIDS, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, n_new=n_new[layer], parents=TREE, row_block=16)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert got.shape == (B, S, H, R, D) and np.isfinite(got).all() and [conn.length(r) for r in RIDS] == LENGTHS
            kh, vh, base = _held(layer, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(TREE, base, n_new[layer])
            _compare(_want(_pair(oracle, layer), _rows_of(q5), R, EVEN, kh, vh, words), _rows_of(got), None, f"attend_spec(row_block=16) tree layer {layer}")


@pytest.mark.parametrize("as_given", [0, 1])
def test_the_fold_lands_in_a_partial_and_survives_the_merge(oracle, as_given):
    """pieces of one tile: 254 positions are 8 pieces, 97 are 4; the fold goes into split 0's partial, members with one piece or none stay final"""
    _chains(oracle, 16, 1, f"pieces, as given {as_given}", tuning=(("attend_tiles_per_split", 1), ("attend_order_as_given", as_given)))


def test_hostile_records_behind_pos_end(oracle):
    """98 positions stored; the K and V records of pages 17 on get the E8M0 code 255 (NaN) in every block; pos_end = 34 is a ragged second tile"""
    rng = np.random.default_rng(3434)
    prompt, S, R = (kd._rows(rng, L, 98, H, D), kd._rows(rng, L, 98, H, D)), 4, 4
    q5, k_new, v_new = (a[:1] for a in _step(S, R))
    with _pool(lengths=[98], prompt=prompt) as (lib, conn):
        nan_codes = np.full(64, 255, np.uint8)
        for page in [(layer * 2 + kind) * T // 2 + j for layer in range(L) for kind in (0, 1) for j in range(17, 49)]:
            info = lib.translate(conn.requests[0].handle, page * 4096)
            assert info.aux_offset and _hip_runtime().hipMemcpy(ctypes.c_void_p(info.pool_addr + info.aux_offset), nan_codes.ctypes.data, 64, 1) == 0
        for layer in range(L):
            kh, vh, base = _held(layer, k_new, v_new, [34], prompt)
            words = SpeckvKVConnector.tree_masks(_chain(S), base)
            out, lse = _entry(lib, conn, layer, _rows_of(q5), R, kh, vh, words, rids=[0], pos_end=np.asarray([34], np.uint32))
            assert np.isfinite(out).all() and np.isfinite(lse).all()
            _compare(_want(_pair(oracle, layer, "hostile", prompt), _rows_of(q5), R, [34], kh, vh, words), out, lse, f"attend_spec_mx4 hostile codes layer {layer}")


def test_refusals_launch_nothing():
    """g = 0 and 17, an odd pos_end, a NULL mask, a capturing stream, FP8 and INT4 pools: INVAL, the fill pattern kept; then the good call writes every row"""
    torch = torch_mod()
    S, R = 2, 4
    q5, k_new, v_new = _step(S, R)
    kh, vh, base = _held(0, k_new, v_new)
    kh, vh, words = np.nan_to_num(kh), np.nan_to_num(vh), SpeckvKVConnector.tree_masks(_chain(S), base)
    bad = dict(mxfp4=[dict(g=0), dict(g=17, rows_per_pos=1, mask_stride=17), dict(pos_end=np.asarray(EVEN, np.uint32) | (np.arange(B) == 4)), dict(d_mask=0)],
               fp8=[{}], int4=[{}])
    for scheme, changes in bad.items():
        with _pool(scheme) as (lib, conn):
            out = torch.full((B, H, S * R, D), PATTERN, dtype=torch.int32, device="cuda")
            call = lambda **change: _entry(lib, conn, 0, _rows_of(q5), R, kh, vh, words, out=out, **change)
            for change in changes:
                assert pytest.raises(SpeckvError, call, **change).value.status == -4, (scheme, change)
            if scheme == "mxfp4":
                capturing, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                with graph_capture(graph, capturing):
                    assert pytest.raises(SpeckvError, lib.attend_spec_mx4, **dict(_entry.last, stream=capturing.cuda_stream)).value.status == -4
                    out.add_(0)
                del graph
            torch.cuda.synchronize()
            assert (out.cpu().numpy().view(np.uint32) == PATTERN).all()
            if scheme == "mxfp4":
                assert not (call()[0].view(np.uint32) == PATTERN).any()
