"""-m gpu: speckv_ext_attend_spec_window (k_attend_fp8_spec) and SpeckvKVConnector.attend_spec(window=W).  Conventions, content (hostile in front of
lo(0)), float64 reference and bound are tests/test_gpu_k8v4_spec_window.py's, imported: its Members over ONE FP8 allocation, K and V both from
HeadChecker(oracle, FP8); every (member, head, row), rows that see nothing exactly 0 / -inf, no NaN; worst err / tol printed before it is asserted."""
import types

import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_k8v4_spec_window as kw
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_decode_window import checker, content
from tests.test_gpu_hostile_ranges import tuned

pytestmark = pytest.mark.gpu
L, T, SM, FP8, LENGTHS = kw.L, kw.T, kw.SM, kw.FP8, [0, 1, 2, 31, 33, 64, 65, 97, 200]
_compare, _rows_of, _step, _tables, _chain, lo_of = kw._compare, kw._rows_of, kw._step, kw._tables, kw._chain, kw.lo_of


class _AsSplit:
    """the FP8 connector where kw.Members expects a split one: the one handle under both names, the entry with one handle array"""

    def __init__(self, lib, scheme="fp8"):
        self._conn, self.lib = SpeckvKVConnector(lib, L, H, D, T, scheme), types.SimpleNamespace(attend_kv_spec_window=self._entry)

    def _entry(self, k_handles, v_handles, **args):
        self.last = dict(handles=k_handles, **args)                                     # (the capture case of the refusals repeats it on a capturing stream)
        return self._conn.lib.attend_spec_window(**self.last)

    def __getattr__(self, name):
        if name == "requests":
            return {rid: types.SimpleNamespace(length=r.length, k_handle=r.handle, v_handle=r.handle) for rid, r in self._conn.requests.items()}
        return getattr(self._conn, name)


class Members(kw.Members):
    def pair(self, oracle, layer, i):
        c = checker(oracle, FP8, layer, *self.spans[i]) if self.own is None else HeadChecker(oracle, FP8, self.own[i][layer * T:(layer + 1) * T], T)
        return c, c


def _case(oracle, lengths, window, S, R, what, rows=None, tuning=(), parents=None, n_new=(None, None)):
    """per layer against float64: a chain of S through the entry (out, lse), or `parents` with the layer's n_new through attend_spec(window=W) (out)"""
    torch = torch_mod()
    q5, k_new, v_new = _step(len(lengths), S, R)
    with kw._pool(torch) as (lib, _), tuned(tuning):                                       # (kw's engine and pool; its split connector goes unused)
        m = Members(_AsSplit(lib), lengths, window, 8000 + window, rows)
        for layer in range(L):
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(parents or _chain(S), base, m.n, window, n_new[layer])
            if parents is None:
                out, lse = m.entry(layer, _rows_of(q5), R, kh, vh, words, depths)
            else:
                got = m.conn.attend_spec(layer, m.rids, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, n_new=n_new[layer], parents=parents, window=window)
                torch.cuda.synchronize()
                out, lse = _rows_of(got.cpu().numpy()), None
                assert np.isfinite(out).all() and [m.conn.length(r) for r in m.rids] == list(lengths)
            _compare(m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths), out, lse, f"attend_spec_window {what} layer {layer}")


@pytest.mark.parametrize("S,R", [(4, 4), (2, 8), (16, 1)])
@pytest.mark.parametrize("window", [1, 2, 3, 17, 33, 48, 64, 100])
def test_chains_under_windows(oracle, window, S, R):
    """odd tails, a bound inside tile 0 and (W = 48, 16 depths on 65 and 97: skip 33) inside tile 1, deep rows blind to tile 0, rel < 0 (W >= 48), members blind to the pool"""
    _case(oracle, LENGTHS, window, S, R, f"W {window} S {S} R {R}")


@pytest.mark.parametrize("as_given", [0, 1])
def test_rows_masked_throughout_a_piece_survive_the_merge(oracle, as_given):
    """pieces of one tile, S = 16 under W = 15 (kw.MERGE_LENGTHS, see there): 100 has rows masked throughout piece 0, 66 throughout piece 1"""
    _case(oracle, kw.MERGE_LENGTHS, kw.MERGE_W, 16, 1, f"pieces, as given {as_given}", tuning=(("attend_tiles_per_split", 1), ("attend_order_as_given", as_given)))


def test_hostile_records_in_front_of_every_window(oracle):
    """every whole page in front of begin + cut_pos (positions < lo(0) & ~1) has a K scale of inf and a V scale of NaN; the reference never reads them"""
    lengths, made = [97, 60, 61, 200], []
    for n in lengths:
        made.append(content(lo_of(n, 0, 33), n & ~1).copy())
        x = made[-1].reshape(L, 2, T, H, D)
        x[:, 0, :lo_of(n, 0, 33) & ~1, :, 5], x[:, 1, :lo_of(n, 0, 33) & ~1, :, 9] = np.inf, np.nan
    _case(oracle, lengths, 33, 16, 1, "hostile scales", rows=made)


@pytest.mark.parametrize("window", [33, 3])
def test_a_tree_and_a_ragged_step_through_the_connector(oracle, window):
    """kw.TREE: 7 nodes, two branches, rows_per_pos 4 (two groups); node 4 has depth 1 -- its bound is depth 1's, not index 4's; layer 1 ragged"""
    assert SpeckvKVConnector.chunk_tree_depths(kw.TREE, 1)[0] == [0, 1, 2, 3, 1, 2, 3]
    _case(oracle, LENGTHS, window, len(kw.TREE), 4, f"tree W {window}", parents=kw.TREE, n_new=(None, [7, 0, 5, 2, 7, 1, 6, 0, 3]))


def test_refusals_launch_nothing():
    """g = 0 and 17, a length off {pos_end, pos_end + 1}, W = 0, a capturing stream, INT4 / MXFP4 pools: INVAL, the fill pattern kept; then the good set"""
    torch = torch_mod()
    S, R, lengths = 2, 4, [64, 33, 0, 97]
    q5, k_new, v_new = _step(len(lengths), S, R)
    bad = dict(fp8=[dict(g=0), dict(g=17, rows_per_pos=1, mask_stride=17), dict(length=np.asarray(lengths, np.uint32) + 2), dict(window=0)], int4=[{}], mxfp4=[{}])
    for scheme in bad:
        with kw._pool(torch) as (lib, _):
            m = Members(_AsSplit(lib, scheme), lengths, 33, 8700)
            kh, vh, base = m.held(0, k_new, v_new)
            words, depths = _tables(_chain(S), base, len(lengths), 33)
            out = torch.full((len(lengths), H, S * R, D), kw.PATTERN, dtype=torch.int32, device="cuda")
            call = lambda **change: m.entry(0, _rows_of(q5), R, np.nan_to_num(kh), np.nan_to_num(vh), words, depths, d_out=out.data_ptr(), **change)
            for change in bad[scheme]:
                assert pytest.raises(SpeckvError, call, **change).value.status == -4, (scheme, change)
            if scheme == "fp8":
                capturing, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
                with graph_capture(graph, capturing):
                    last = dict(m.conn.last, window=33, stream=capturing.cuda_stream)     # (refused before anything is read: the arguments of the last call)
                    assert pytest.raises(SpeckvError, lib.attend_spec_window, **last).value.status == -4
                    out.add_(0)
                del graph
                torch.cuda.synchronize()
            assert (out.cpu().numpy().view(np.uint32) == kw.PATTERN).all()
            if scheme == "fp8":
                call()
                assert not (out.cpu().numpy().view(np.uint32) == kw.PATTERN).any()


def test_a_connector_walk_on_a_local_and_a_global_layer(oracle):
    """layer 0 local (W = 33), layer 1 global: attend_spec against attend_tree, then commit.  The queries are +-2^-k with a 1 in every row: exact as E4M3 x
    a row scale and as fp16.  Each route is within the bound of the one float64 reference, so they differ by 2 x the layer's bound at most, per element."""
    torch = torch_mod()
    S, R, W, lengths, rng = 3, 4, 33, [59, 6, 98], np.random.default_rng(8900)
    with kw._pool(torch) as (lib, _):
        m = Members(_AsSplit(lib), lengths, W, 8900, rows=[content(0, T)] * len(lengths))
        _, k_new, v_new = _step(m.n, S, R)
        q5 = (rng.choice([-1.0, 1.0], (m.n, S, H, R, D)) * np.exp2(-rng.integers(0, 4, (m.n, S, H, R, D)))).astype(np.float16)
        q5[..., 0] = 1.0
        dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
        for layer, window in ((0, W), (1, None)):
            spec = _rows_of(m.conn.attend_spec(layer, m.rids, dq, dk, dv, SM, window=window).cpu().numpy())
            tree = _rows_of(m.conn.attend_tree(layer, m.rids, dq, dk, dv, SM, _chain(S), window=window).cpu().numpy())
            kh, vh, base = m.held(layer, k_new, v_new)
            words, depths = _tables(_chain(S), base, m.n, window)
            tol = m.want(oracle, layer, _rows_of(q5), R, kh, vh, words, depths, window=window or 0)[2]
            worst = float((np.abs(spec.astype(np.float64) - tree) / (2.0 * tol)).max())
            print(f"connector walk layer {layer} window {window}: attend_spec against attend_tree, worst |diff| / (2 tol) {worst:.3f}")
            assert worst <= 1.0                                                         # (a NaN in either fails here too)
        m.conn.commit(m.rids, dk, dv, [[0, 1], [0], [0, 1, 2]])
        assert [m.conn.length(r) for r in m.rids] == [61, 7, 101]
