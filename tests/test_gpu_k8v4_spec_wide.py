"""-m gpu: the split pool's multi-position step with 17..32 query rows per kv head in ONE pass -- speckv_ext_attend_kv_spec_wide
(k_attend_k8v4_wide: two blocks of 16 rows per wave over each tile's K bytes and widened V operand) and
SpeckvSplitKVConnector.attend_spec(rows_per_pass=32) on top of it.

Reference and bound: tests/test_gpu_k8v4_spec.py's _want / _compare (numpy float64 over the oracle's decoded records and the held rows;
|err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta), under a window tests/test_gpu_k8v4_spec_window.py's Members.want
(the same bound per row over [lo(depth), stored), words from tree_masks(window=W)).  Every (member, head, row) of out and lse is compared.
Members of one call: length 1 (nothing stored, the tail and the held rows only), 38 (a whole tile and a ragged one), 97 (3 tiles + a
tail); both layers.  The helpers call the 16-row entries by name: _Wide puts the wide entry in their place."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_k8v4_decode as kd
from tests import test_gpu_k8v4_spec_window as kw
from tests._gpu import D, H, graph_capture, set_tuning, torch_mod
from tests.test_gpu_k8v4_spec import _compare, _entry, _held, _pair, _rows_of, _step, _want

pytestmark = pytest.mark.gpu
L, SM, PATTERN = kd.L, kd.SM, kd.PATTERN
LENGTHS = [1, 38, 97]
RIDS, B, EVEN = [0, 1, 2], 3, [n & ~1 for n in LENGTHS]
TREE = [-1, 0, 1, 2, 0, 4, 5, 6]             # node 0, then a branch of three and a branch of four


class _Wide:
    """the library with speckv_ext_attend_kv_spec_wide where the helpers of the 16-row tests call their entries"""

    def __init__(self, lib):
        self._lib, self.attend_kv_spec_window = lib, lib.attend_kv_spec_wide
        self.attend_kv_spec = lambda **args: lib.attend_kv_spec_wide(length=None, d_depth=0, window=0, **args)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _members():
    return [(kd._prompt()[0][:, :n], kd._prompt()[1][:, :n]) for n in LENGTHS]


def _data(S, R):
    return tuple(a[:B] for a in _step(S, R))


@pytest.mark.parametrize("S,R,tiles_per_split", [(4, 8, 0), (3, 8, 0), (9, 2, 0), (16, 2, 0), (4, 8, 1), (3, 8, 1)])
def test_row_blocks_against_float64(oracle, S, R, tiles_per_split):
    """g = 32 (both blocks full), 24 (the second half empty), 18 (two rows in it, position 8 straddles the seam), 32 of 16 positions (17
    held rows with the tail).  tiles_per_split = 1: the member of 3 tiles leaves a partial per block and piece, the fold lands in split
    0's two, and both survive the merge (a half-empty second block too)."""
    torch = torch_mod()
    q5, k_new, v_new = _data(S, R)
    with kd._batch(torch, _members()) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", tiles_per_split)
            for layer in range(L):
                kh, vh, base = _held(layer, k_new, v_new, LENGTHS)
                words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base)
                out, lse, _ = _entry(torch, _Wide(lib), conn, layer, _rows_of(q5), R, kh, vh, words, rids=RIDS)
                assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any()
                _compare(_want(_pair(oracle, layer), _rows_of(q5), R, EVEN, kh, vh, words), out, lse, f"attend_kv_spec_wide S {S} R {R} tps {tiles_per_split} layer {layer}")
        finally:
            set_tuning("attend_tiles_per_split", 0)


def test_a_tree_and_a_ragged_step(oracle):
    """8 nodes at R = 4, g = 32: the second branch lies in block 1 and sees node 0 of block 0, none of its siblings -- the reference with
    chain visibility is further than the tolerance from the tree's (tests/test_gpu_k8v4_spec.py's argument).  n_new < S for two members: a
    dead node's rows are the stored part alone, finite."""
    torch = torch_mod()
    S, R = len(TREE), 4
    q5, k_new, v_new = _data(S, R)
    v_new = v_new.copy()
    v_new[:, 4:] += np.float16(6.0)                                                  # the second branch's values stand apart
    with kd._batch(torch, _members()) as (lib, conn):
        for layer in range(L):
            kh, vh, base = _held(layer, k_new, v_new, LENGTHS)
            pair, qg = _pair(oracle, layer), _rows_of(q5)
            for n_new in (None, [8, 5, 3]):
                words = SpeckvKVConnector.tree_masks(TREE, base, n_new)
                want = _want(pair, qg, R, EVEN, kh, vh, words)
                if n_new is None:
                    chain = _want(pair, qg, R, EVEN, kh, vh, SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base))
                    assert (np.abs(chain[0] - want[0])[:, :, 4 * R:] / want[2][:, :, 4 * R:]).reshape(B, -1).max(axis=1).min() > 10.0
                out, lse, _ = _entry(torch, _Wide(lib), conn, layer, qg, R, kh, vh, words, rids=RIDS)
                assert np.isfinite(out).all()
                _compare(want, out, lse, f"attend_kv_spec_wide tree n_new {n_new} layer {layer}")


@pytest.mark.parametrize("S,R,window", [(4, 8, 40), (4, 8, 32), (16, 2, 12)])
def test_under_a_window(oracle, S, R, window):
    """length 70: W = 40 is rel = 31 -- depths 0..3 skip 31..34, block 1's rows (depths 2, 3) lose all of tile 0 and positions of tile 1
    that block 0's rows see; W = 32 is rel = 7, skips 7..10 inside tile 0.  W = 12 with 16 positions: deep rows see no stored position and
    lose held ones.  Positions in front of every window are hostile (Members)."""
    torch = torch_mod()
    lengths = [70, 71, 1, 200]
    q5, k_new, v_new = kw._step(len(lengths), S, R)
    assert SpeckvKVConnector.spec_window_range(70, 40)[1] == 31 and SpeckvKVConnector.spec_window_range(70, 32)[:2] == (32, 7)
    with kw._pool(torch) as (lib, conn):
        conn.lib = _Wide(lib)                                                       # (Members.entry calls conn.lib.attend_kv_spec_window)
        m = kw.Members(conn, lengths, window, 8100 + window)
        for layer in range(kw.L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = kw._tables(kw._chain(S), base, len(lengths), window)
            out, lse = m.entry(layer, kw._rows_of(q5), R, kh, vh, words, depths)
            kw._compare(m.want(oracle, layer, kw._rows_of(q5), R, kh, vh, words, depths), out, lse, f"attend_kv_spec_wide S {S} R {R} W {window} layer {layer}")


@pytest.mark.parametrize("S,R", [(4, 8), (5, 8)])
def test_the_connector_at_32_rows_per_pass(oracle, S, R):
    """(4, 8): one wide group; (5, 8): a wide group, then a 16-row group of one position that sees the first group's positions through its
    mask columns.  rows_per_pass=16 is attend_spec() without the argument, bit for bit."""
    torch = torch_mod()
    q5, k_new, v_new = _data(S, R)
    assert [n * R for _, n in SpeckvKVConnector.spec_groups(S, R, 32)] == ([32] if S == 4 else [32, 8])
    with kd._batch(torch, _members()) as (lib, conn):
        dq, dk, dv = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q5, k_new, v_new))
        for layer in range(L):
            got = conn.attend_spec(layer, RIDS, dq, dk, dv, SM, rows_per_pass=32)
            plain, same = conn.attend_spec(layer, RIDS, dq, dk, dv, SM), conn.attend_spec(layer, RIDS, dq, dk, dv, SM, rows_per_pass=16)
            torch.cuda.synchronize()
            assert np.array_equal(plain.cpu().numpy().view(np.uint32), same.cpu().numpy().view(np.uint32))
            kh, vh, base = _held(layer, k_new, v_new, LENGTHS)
            words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base)
            _compare(_want(_pair(oracle, layer), _rows_of(q5), R, EVEN, kh, vh, words), _rows_of(got.cpu().numpy()), None, f"attend_spec(rows_per_pass=32) S {S} layer {layer}")


def test_refusals_launch_nothing():
    """g = 16 and g = 33, g = 24 at one row per position and a capturing stream: SPECKV_ERR_INVAL, d_out keeps its fill pattern"""
    torch = torch_mod()
    S, R = 4, 8
    q5, k_new, v_new = _data(S, R)
    with kd._batch(torch, _members()) as (lib, conn):
        kh, vh, base = _held(0, k_new, v_new, LENGTHS)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dk, dv = dev(_rows_of(q5)), dev(np.nan_to_num(kh)), dev(np.nan_to_num(vh))
        dm = dev(np.asarray(SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base), np.uint32).view(np.int32))
        out = torch.full((B, H, 33, D), PATTERN, dtype=torch.int32, device="cuda")
        st, capturing = torch.cuda.Stream(), torch.cuda.Stream()
        good = dict(k_handles=[conn.requests[r].k_handle for r in RIDS], v_handles=[conn.requests[r].v_handle for r in RIDS], layer=0, d_q_f16=dq.data_ptr(), g=S * R,
                    rows_per_pos=R, pos_end=EVEN, length=None, d_depth=0, window=0, d_k_held=dk.data_ptr(), d_v_held=dv.data_ptr(), seq_stride_elems=(1 + S) * H * D,
                    pos_stride_elems=H * D, d_mask=dm.data_ptr(), mask_stride=S, sm_scale=SM, d_out=out.data_ptr(), d_lse=0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for change in (dict(g=16), dict(g=33, rows_per_pos=1, mask_stride=33), dict(g=24, rows_per_pos=1, mask_stride=24)):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec_wide(**dict(good, **change))
            assert e.value.status == -4, change
        bump, graph = torch.zeros(4, device="cuda"), torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with graph_capture(graph, capturing):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec_wide(**dict(good, stream=capturing.cuda_stream))
            assert e.value.status == -4
            bump.add_(1)
        del graph
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == PATTERN).all()                  # (33 rows per head: room for the refused g)
