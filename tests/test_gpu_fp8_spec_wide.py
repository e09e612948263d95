"""-m gpu: the FP8 pool's multi-position step with 17..32 query rows per kv head in ONE pass -- speckv_ext_attend_spec_wide
(k_attend_fp8_wide: two blocks of 16 rows per wave over each tile's K bytes, f16 V operand and V reference scale), on a global layer
(window 0) and under a window, and SpeckvKVConnector.attend_spec(rows_per_pass=32) on top of it.

Conventions, content (hostile in front of lo(0)), float64 reference and bound are tests/test_gpu_k8v4_spec_window.py's through
tests/test_gpu_fp8_spec_window.py's Members (ONE FP8 allocation, K and V from HeadChecker(oracle, FP8)): |err| <= (2e-3 + 2 delta)
sum p|v| + 1e-6, |lse err| <= 2e-3 + delta over every (member, head, row); rows that see nothing exactly 0 / -inf; no NaN; the worst
err / tol printed before it is asserted (MI355X: 0.133 at worst over all cases; the wide rows equal two 16-row calls bit for bit at
every member).  The helpers call the 16-row entry by name: _Entry puts the wide entry in its place."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_fp8_spec_window as fw
from tests import test_gpu_k8v4_spec_window as kw
from tests._gpu import D, H, graph_capture, torch_mod
from tests.test_gpu_hostile_ranges import tuned
from tests.test_gpu_k8v4_spec_wide import TREE

pytestmark = pytest.mark.gpu
L, SM = kw.L, kw.SM
_compare, _rows_of, _step, _tables, _chain = kw._compare, kw._rows_of, kw._step, kw._tables, kw._chain
PLAIN, WINDOWED = [0, 1, 38, 97], [70, 71, 1, 200]


class _Entry(fw._AsSplit):
    """fw._AsSplit with speckv_ext_attend_spec_wide where kw.Members calls its entry (wide = False: the 16-row entry again)"""
    wide = True

    def _entry(self, k_handles, v_handles, **args):
        self.last = dict(handles=k_handles, **args)
        return (self._conn.lib.attend_spec_wide if self.wide else self._conn.lib.attend_spec_window)(**self.last)


@pytest.mark.parametrize("S,R,tiles_per_split", [(4, 8, 0), (3, 8, 0), (9, 2, 0), (16, 2, 0), (4, 8, 1), (3, 8, 1)])
def test_row_blocks_without_a_window(oracle, S, R, tiles_per_split):
    """g = 32 (both blocks full), 24 (half of block 1 empty), 18 (position 8 straddles the seam), 32 of 16 positions (17 held rows with
    the tail).  Members: nothing stored, a tail alone, a whole plus a ragged tile, three tiles plus a tail.  tiles_per_split = 1: two
    partials per piece, the fold lands in split 0's, and both survive the merge."""
    torch = torch_mod()
    q5, k_new, v_new = _step(len(PLAIN), S, R)
    with kw._pool(torch) as (lib, _), tuned((("attend_tiles_per_split", tiles_per_split),)):
        m = fw.Members(_Entry(lib), PLAIN, 0, 9100)
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(_chain(S), base, m.n, 0)
            out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths, length=None, d_depth=0)      # (a global layer reads neither)
            _compare(m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths), out, lse, f"attend_spec_wide S {S} R {R} tps {tiles_per_split} layer {layer}")


@pytest.mark.parametrize("S,R,window", [(4, 8, 40), (4, 8, 32), (16, 2, 12)])
def test_under_a_window(oracle, S, R, window):
    """length 70: W = 40 is rel = 31 -- block 1's rows (depths 2, 3) lose all of tile 0 and positions of tile 1 that block 0's rows see;
    W = 32 is rel = 7, inside tile 0; W = 12 with 16 positions: deep rows see no stored position and lose held ones.  Positions in front
    of every window are hostile.  (4, 8, 40) again with pieces of one tile: rows 0..15 and 16..31 against two 16-row calls on the same
    tables, bit for bit -- the per-row arithmetic and cut_pos are the same, the forced split length pins the pieces."""
    torch = torch_mod()
    q5, k_new, v_new = _step(len(WINDOWED), S, R)
    qg = _rows_of(q5)
    with kw._pool(torch) as (lib, _):
        m = fw.Members(_Entry(lib), WINDOWED, window, 9200 + window)
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(_chain(S), base, m.n, window)
            out, lse = m.entry(layer, qg, R, kh, vh, words, depths)
            _compare(m.want(oracle, layer, qg, R, kh, vh, words, depths), out, lse, f"attend_spec_wide S {S} R {R} W {window} layer {layer}")
            if (S, R, window) != (4, 8, 40):
                continue
            with tuned((("attend_tiles_per_split", 1),)):
                out, lse = m.entry(layer, qg, R, kh, vh, words, depths)
                m.conn.wide = False
                for b in range(2):
                    o16, l16 = m.entry(layer, qg[:, :, 16 * b:16 * b + 16], R, kh, vh, [w[2 * b:2 * b + 2] for w in words], [d[2 * b:2 * b + 2] for d in depths])
                    assert np.array_equal(o16.view(np.uint32), out[:, :, 16 * b:16 * b + 16].view(np.uint32)), (layer, b)
                    assert np.array_equal(l16.view(np.uint32), lse[:, :, 16 * b:16 * b + 16].view(np.uint32)), (layer, b)
                m.conn.wide = True


@pytest.mark.parametrize("window", [0, 33])
@pytest.mark.parametrize("S,R,parents,n_new", [(8, 4, TREE, (None, [8, 5, 3, 6])), (4, 8, None, (None, None)), (5, 8, None, (None, None))])
def test_the_connector_at_32_rows_per_pass(oracle, S, R, parents, n_new, window):
    """TREE: 8 nodes at R = 4, g = 32, the second branch in block 1; layer 1 ragged.  Chains of (4, 8) and (5, 8): [32] and [32, 8]
    rows -- the trailing group takes the 16-row route and sees the first group's positions through its mask columns.  Output finite
    and within the bound, lengths unchanged; rows_per_pass=16 is the call without the argument, bit for bit."""
    torch = torch_mod()
    lengths = WINDOWED if window else PLAIN
    q5, k_new, v_new = _step(len(lengths), S, R)
    assert [n * R for _, n in SpeckvKVConnector.spec_groups(S, R, 32)] == ([32, 8] if S == 5 else [32])
    with kw._pool(torch) as (lib, _):
        m = fw.Members(_Entry(lib), lengths, window, 9300 + window)
        dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
        for layer in range(L):
            step = lambda **how: m.conn.attend_spec(layer, m.rids, dq, dk, dv, SM, n_new=n_new[layer], parents=parents, window=window, **how).cpu().numpy()
            got, plain, same = step(rows_per_pass=32), step(), step(rows_per_pass=16)
            assert np.isfinite(got).all() and [m.conn.length(r) for r in m.rids] == list(lengths)
            assert np.array_equal(plain.view(np.uint32), same.view(np.uint32))
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(parents or _chain(S), base, m.n, window, n_new[layer])
            _compare(m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths), _rows_of(got), None, f"attend_spec(rows_per_pass=32) S {S} R {R} W {window} layer {layer}")


def test_refusals_launch_nothing():
    """g = 16, g = 33, g = 24 at one row per position, W >= 1 with a NULL length, a capturing stream, INT4 / MXFP4 pools: INVAL and the
    fill pattern kept; then the good call overwrites all of it"""
    torch = torch_mod()
    S, R = 4, 8
    q5, k_new, v_new = _step(len(PLAIN), S, R)
    bad = dict(fp8=[dict(g=16), dict(g=33, rows_per_pos=1, mask_stride=33), dict(g=24, rows_per_pos=1, mask_stride=24), dict(window=33, length=None)],
               int4=[{}], mxfp4=[{}])
    for scheme in bad:
        with kw._pool(torch) as (lib, _):
            m = fw.Members(_Entry(lib, scheme), PLAIN, 0, 9400)
            kh, vh, base = m.held(0, k_new, v_new)
            words, depths = _tables(_chain(S), base, m.n, 0)
            out = torch.full((m.n, H, 33, D), kw.PATTERN, dtype=torch.int32, device="cuda")          # (33 rows per head: room for the refused g)
            call = lambda **change: m.entry(0, _rows_of(q5), R, np.nan_to_num(kh), np.nan_to_num(vh), words, depths, d_out=out.data_ptr(), **change)
            for change in bad[scheme]:
                assert pytest.raises(SpeckvError, call, **change).value.status == -4, (scheme, change)
            if scheme == "fp8":
                capturing, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                with graph_capture(graph, capturing):
                    assert pytest.raises(SpeckvError, lib.attend_spec_wide, **dict(m.conn.last, window=0, stream=capturing.cuda_stream)).value.status == -4
                    out.add_(0)
                del graph
                torch.cuda.synchronize()
            assert (out.cpu().numpy().view(np.uint32) == kw.PATTERN).all()
            if scheme == "fp8":
                call()
                assert not (out.cpu().numpy().view(np.uint32).reshape(-1)[:m.n * H * S * R * D] == kw.PATTERN).any()      # (rows [member][head][32])
