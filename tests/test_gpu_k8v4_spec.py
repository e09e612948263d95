"""-m gpu: the split pool's multi-position step on the decode kernel -- speckv_ext_attend_kv_spec (k_attend_k8v4<false, true>: the stored
positions walked once for g = n_q x rows_per_pos query rows, the rows held outside the pool folded in by split 0 inside the launch) and
SpeckvSplitKVConnector.attend_spec on top of it.

Reference: numpy float64 softmax attention.  Stored part as tests/test_gpu_k8v4_decode.py: the query is HeadChecker(oracle, FP8).q_rows
(E4M3 x a row scale), K the FP8 records, V the MXFP4 records.  Held part: the fp16 query, the fp16 rows, visibility from the mask words.
Bound: the project's for 8-bit-query kernels (tests/_gpu.py check_rows): |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 +
delta, delta = 3e-5 max sum |q||k| sm over the stored and held positions of a (member, head).  Every (member, head, row) is compared; a row
that sees nothing anywhere is exactly 0 with lse -inf.  Geometry: L = 2, T = 256, H = 8, D = 128, both layers; the members are prefixes of
one prompt with 0, 1, 2, 31, 32, 33, 64, 97 and 254 positions (nothing stored; the tail only; one page; a ragged tile with a tail; a whole
tile; a tile and a tail; two tiles; a ragged fourth tile with a tail; nearly the region)."""
import os

import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_k8v4_decode as kd
from tests._gpu import D, H, graph_capture, set_tuning, torch_mod

pytestmark = pytest.mark.gpu
L, T, SM, PATTERN = kd.L, kd.T, kd.SM, kd.PATTERN
LENGTHS = [0, 1, 2, 31, 32, 33, 64, 97, 254]
RIDS = list(range(len(LENGTHS)))
B = len(LENGTHS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_data = {}


def _members():
    k, v = kd._prompt()
    return [(k[:, :n], v[:, :n]) for n in LENGTHS]


def _step(S, R, seed=0):
    """the step's query [B][S][H][R][D] and new rows [B][S][L][H][D] (K, V), once per shape"""
    key = (S, R, seed)
    if key not in _data:
        rng = np.random.default_rng(4100 + 100 * S + R + 7 * seed)
        _data[key] = (kd._rows(rng, B, S, H, R, D), kd._rows(rng, B, S, L, H, D), kd._rows(rng, B, S, L, H, D))
    return _data[key]


def _held(layer, k_new, v_new, lengths=LENGTHS, prompt=None):
    """the held rows of `layer` as the entry takes them: [B][1 + S][H][D] fp16 per kind -- the odd last position first where there is one,
    then the new positions; the slots behind them are NaN (nothing may read them) -- and base [B]"""
    k, v = prompt if prompt is not None else kd._prompt()
    S = k_new.shape[1]
    kh = np.full((len(lengths), 1 + S, H, D), np.nan, np.float16)
    vh = np.full((len(lengths), 1 + S, H, D), np.nan, np.float16)
    base = [n & 1 for n in lengths]
    for b, n in enumerate(lengths):
        if n & 1:
            kh[b, 0], vh[b, 0] = k[layer, n - 1], v[layer, n - 1]
        kh[b, base[b]:base[b] + S], vh[b, base[b]:base[b] + S] = k_new[b, :, layer], v_new[b, :, layer]
    return kh, vh, base


def _rows_of(q5):
    """[B][S][H][R][D] -> the entry's [B][H][S * R][D]"""
    Bq, S, _, R, _ = q5.shape
    return np.ascontiguousarray(q5.transpose(0, 2, 1, 3, 4).reshape(Bq, H, S * R, D))


def _want(pair, qg, R, npos, kh, vh, words):
    """float64: out [M][H][G][D], lse [M][H][G], tol, ltol of qg [M][H][G][D] over the stored positions [0, npos[m]) of `pair` and the held
    positions the words [M][G // R] show"""
    k8, v4 = pair
    M, _, G, _ = qg.shape
    out, lse = np.zeros((M, H, G, D)), np.full((M, H, G), -np.inf)
    tol, ltol = np.full((M, H, G, D), 1e-6), np.full((M, H, G), 2e-3)
    for head in range(H):
        K, V = k8.kv(head)[0], v4.kv(head)[1]
        qe = k8.q_rows(qg[:, head]).reshape(M, G, D)
        for m in range(M):
            n = int(npos[m])
            qf = qg[m, head].astype(np.float64)
            top = max((int(w).bit_length() for w in words[m]), default=0)
            kf, vf = kh[m, :top, head].astype(np.float64), vh[m, :top, head].astype(np.float64)
            sums = [np.abs(qe[m]) @ np.abs(K[:n]).T] + ([np.abs(qf) @ np.abs(kf).T] if top else [])
            delta = 3e-5 * float(np.concatenate(sums, axis=1).max(initial=0.0)) * SM
            for r in range(G):
                seen = [t for t in range(top) if (int(words[m][r // R]) >> t) & 1]
                s = np.concatenate([(K[:n] @ qe[m, r]) * SM, (kf[seen] @ qf[r]) * SM])
                if len(s) == 0:
                    continue
                vals = np.concatenate([V[:n], vf[seen]])
                mx = s.max()
                p = np.exp(s - mx)
                out[m, head, r], lse[m, head, r] = (p @ vals) / p.sum(), mx + np.log(p.sum())
                tol[m, head, r] = (2e-3 + 2 * delta) * ((p @ np.abs(vals)) / p.sum()) + 1e-6
                ltol[m, head, r] = 2e-3 + delta
    return out, lse, tol, ltol


def _compare(want, out, lse, what):
    """-> worst err / tol over every (member, head, row); rows that see nothing are exactly 0 / -inf"""
    w_out, w_lse, tol, ltol = want
    nothing = np.isneginf(w_lse)
    assert not out[nothing].any(), (what, "a row that sees nothing is exactly 0")
    err = np.abs(out.astype(np.float64) - w_out)
    worst = float(np.nan_to_num(err / tol, nan=np.inf).max())
    if lse is not None:
        assert np.all(np.isneginf(lse[nothing])), (what, "a row that sees nothing has lse -inf")
        with np.errstate(invalid="ignore"):
            lerr = np.where(nothing, 0.0, np.abs(lse.astype(np.float64) - w_lse))
        worst = max(worst, float(np.nan_to_num(lerr / ltol, nan=np.inf).max()))
    print(f"{what}: worst err / tol {worst:.3f}")
    assert worst <= 1.0, (what, worst, np.argwhere(np.nan_to_num(err / tol, nan=np.inf) > 1.0)[:4])
    return worst


def _entry(torch, lib, conn, layer, qg, R, kh, vh, words, rids=RIDS, with_lse=True, on=None, **change):
    """speckv_ext_attend_kv_spec itself over what the connector holds -> (out, lse or None) as fp32 numpy; both start as the fill pattern"""
    Bq, _, G, _ = qg.shape
    reqs = [conn.requests[r] for r in rids]
    st = on if on is not None else torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, dk, dv = dev(qg), dev(kh), dev(vh)
    dm = dev(np.asarray(words, np.uint32).view(np.int32))
    out = torch.full((Bq, H, G, D), PATTERN, dtype=torch.int32, device="cuda")
    lse = torch.full((Bq, H, G), PATTERN, dtype=torch.int32, device="cuda")
    P = kh.shape[1]
    args = dict(k_handles=np.asarray([r.k_handle for r in reqs], np.uint64), v_handles=np.asarray([r.v_handle for r in reqs], np.uint64), layer=layer,
                d_q_f16=dq.data_ptr(), g=G, rows_per_pos=R, pos_end=np.asarray([r.length & ~1 for r in reqs], np.uint32), d_k_held=dk.data_ptr(),
                d_v_held=dv.data_ptr(), seq_stride_elems=P * H * D, pos_stride_elems=H * D, d_mask=dm.data_ptr(), mask_stride=dm.shape[1],
                sm_scale=SM, d_out=out.data_ptr(), d_lse=lse.data_ptr() if with_lse else 0, stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    try:
        lib.attend_kv_spec(**args)
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy().view(np.float32), (lse.cpu().numpy().view(np.float32) if with_lse else None), lse.cpu().numpy()


def _pair(oracle, layer):
    k, v = kd._prompt()
    return kd._checker(oracle, "prompt", k, v, layer)


def _even(lengths=LENGTHS):
    return [n & ~1 for n in lengths]


# ----------------------------------------------------------------------------- 1. chains through the connector: one group and two
@pytest.mark.parametrize("S,R", [(1, 1), (4, 4), (2, 8), (16, 1), (5, 4), (3, 8)])
def test_chains_against_float64(oracle, S, R):
    """attend_spec of a causal chain, both layers: (1, 1), (4, 4), (2, 8), (16, 1) are one group, (5, 4) and (3, 8) two -- the second
    group sees the first group's positions as held positions through its mask columns"""
    torch = torch_mod()
    q5, k_new, v_new = _step(S, R)
    assert len(SpeckvKVConnector.spec_groups(S, R)) == (2 if S * R > 16 else 1)
    with kd._batch(torch, _members()) as (lib, conn):
        dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
        for layer in range(L):
            got = conn.attend_spec(layer, RIDS, dq, dk, dv, SM)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (B, S, H, R, D) and got.dtype == torch.float32
            kh, vh, base = _held(layer, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base)
            want = _want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, words)
            _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec chain S {S} R {R} layer {layer}")
        assert [conn.length(r) for r in RIDS] == LENGTHS                           # no state moved


# ----------------------------------------------------------------------------- 2. a ragged step: dead rows are the stored part alone
def test_a_ragged_step_and_its_dead_rows(oracle):
    """n_new 0..S mixed over the members: a dead position's rows equal the stored-only reference (what speckv_ext_attend_kv_batch writes there),
    and the empty member's dead rows are exactly 0 with lse -inf (through the entry, which returns the lse)"""
    torch = torch_mod()
    S, R = 4, 4
    q5, k_new, v_new = _step(S, R)
    n_new = [0, 2, 4, 0, 1, 3, 4, 0, 2]
    with kd._batch(torch, _members()) as (lib, conn):
        for layer in range(L):
            kh, vh, base = _held(layer, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base, n_new)
            assert words[0] == [0] * S and words[3] == [0] * S and words[4][1:] == [0] * (S - 1)
            want = _want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, words)
            got = conn.attend_spec(layer, RIDS, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, n_new=n_new)
            torch.cuda.synchronize()
            assert np.isfinite(got.cpu().numpy()).all()
            _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec ragged layer {layer}")
            out, lse, _ = _entry(torch, lib, conn, layer, _rows_of(q5), R, kh, vh, words)
            _compare(want, out, lse, f"attend_kv_spec ragged layer {layer}")
            assert not out[0].any() and np.all(np.isneginf(lse[0]))                 # nothing stored, nothing seen
            assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any()
            # the dead rows of a member with stored positions: what the batch entry writes (the same walk, no fold)
            plain, plain_lse = kd._entry(torch, lib, conn, RIDS, _rows_of(q5), layer)
            dead = np.asarray(words) == 0
            for b in range(B):
                for j in np.flatnonzero(dead[b]):
                    assert np.array_equal(out[b, :, j * R:(j + 1) * R].view(np.uint32), plain[b, :, j * R:(j + 1) * R].view(np.uint32)), (b, j)
                    assert np.array_equal(lse[b, :, j * R:(j + 1) * R].view(np.uint32), plain_lse[b, :, j * R:(j + 1) * R].view(np.uint32)), (b, j)


# ----------------------------------------------------------------------------- 3. a tree
TREE = [-1, 0, 1, 2, 0, 4, 5]                # node 0, then two branches of three


def test_a_tree_of_two_branches(oracle):
    """7 nodes, rows_per_pos 4: two groups (nodes 0..3, nodes 4..6) -- the second branch sees node 0 of the first group and none of its
    siblings.  The branches' rows differ enough that a node which saw a sibling would miss the bound: the reference with chain visibility
    is further than the tolerance from the tree's."""
    torch = torch_mod()
    S, R = len(TREE), 4
    q5, k_new, v_new = _step(S, R)
    v_new = v_new.copy()
    v_new[:, 4:] += np.float16(6.0)                                                  # the second branch's values stand apart
    with kd._batch(torch, _members()) as (lib, conn):
        for layer in range(L):
            kh, vh, base = _held(layer, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(TREE, base)
            want = _want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, words)
            chain = _want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base))
            apart = np.abs(chain[0] - want[0])[:, :, 4 * R:] / want[2][:, :, 4 * R:]
            assert apart.reshape(B, -1).max(axis=1).min() > 10.0                      # in every member some row of the second branch
            got = conn.attend_spec(layer, RIDS, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, parents=TREE)
            torch.cuda.synchronize()
            _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec tree layer {layer}")
            # and a ragged tree: the members' live counts differ, a dead node takes its subtree with it
            n_new = [7, 0, 5, 2, 7, 1, 6, 4, 3]
            words = SpeckvKVConnector.tree_masks(TREE, base, n_new)
            want = _want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, words)
            got = conn.attend_spec(layer, RIDS, *(torch.from_numpy(a).cuda() for a in (q5, k_new, v_new)), SM, n_new=n_new, parents=TREE)
            torch.cuda.synchronize()
            _compare(want, _rows_of(got.cpu().numpy()), None, f"attend_spec ragged tree layer {layer}")


# ----------------------------------------------------------------------------- 4. pieces and the merge
@pytest.mark.parametrize("tuning", [dict(attend_tiles_per_split=1), dict(attend_tiles_per_split=2), dict(attend_order_as_given=1), dict()])
def test_the_fold_lands_in_a_partial_and_survives_the_merge(oracle, tuning):
    """pieces of one and of two tiles (the member of 254 positions: 8 and 4 pieces -- the fold goes into split 0's partial, the merge
    runs as ever), the order as given, and the library's own rule (rows-first dispatch by length)"""
    torch = torch_mod()
    S, R = 4, 4
    q5, k_new, v_new = _step(S, R)
    with kd._batch(torch, _members()) as (lib, conn):
        try:
            for key, value in tuning.items():
                set_tuning(key, value)
            for layer in range(L):
                kh, vh, base = _held(layer, k_new, v_new)
                words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base, [4, 4, 4, 4, 2, 4, 0, 4, 3])
                out, lse, _ = _entry(torch, lib, conn, layer, _rows_of(q5), R, kh, vh, words)
                _compare(_want(_pair(oracle, layer), _rows_of(q5), R, _even(), kh, vh, words), out, lse, f"attend_kv_spec {tuning} layer {layer}")
        finally:
            for key in tuning:
                set_tuning(key, 0)


# ----------------------------------------------------------------------------- 5. nothing above the highest bit is read; no lse
def test_hostile_rows_above_the_highest_bit_and_a_null_lse(oracle):
    """the held positions above every word's highest bit hold NaN / inf patterns, varied: results stay bit for bit, and the bound holds.
    d_lse NULL: the same rows."""
    torch = torch_mod()
    S, R = 3, 4
    q5, k_new, v_new = _step(S, R)
    n_new = [1, 3, 2, 0, 3, 1, 2, 3, 0]
    with kd._batch(torch, _members()) as (lib, conn):
        kh, vh, base = _held(1, k_new, v_new)
        words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base, n_new)
        want = _want(_pair(oracle, 1), _rows_of(q5), R, _even(), kh, vh, words)
        runs = []
        for bits in (0x7E00, 0x7C00, 0xFC00, 0xFFFF):                              # NaN, +inf, -inf, a NaN of all ones
            k2, v2 = kh.copy(), vh.copy()
            for b in range(B):
                top = max(int(w).bit_length() for w in words[b])
                k2.view(np.uint16)[b, top:] = bits
                v2.view(np.uint16)[b, top:] = bits
            out, lse, _ = _entry(torch, lib, conn, 1, _rows_of(q5), R, k2, v2, words)
            runs.append((out, lse))
        _compare(want, runs[0][0], runs[0][1], "attend_kv_spec hostile rows above the highest bit")
        for out, lse in runs[1:]:
            assert np.array_equal(out.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(lse.view(np.uint32), runs[0][1].view(np.uint32))
        only, none, raw = _entry(torch, lib, conn, 1, _rows_of(q5), R, kh, vh, words, with_lse=False)
        assert none is None and np.array_equal(only.view(np.uint32), runs[0][0].view(np.uint32)) and (raw.view(np.uint32) == PATTERN).all()


# ----------------------------------------------------------------------------- 6. refusals, streams
def test_refusals_launch_nothing():
    """every refusal of the entry on the GPU engine is SPECKV_ERR_INVAL, a capturing stream included, and d_out keeps its fill pattern"""
    torch = torch_mod()
    S, R = 2, 4
    q5, k_new, v_new = _step(S, R)
    with kd._batch(torch, _members()) as (lib, conn):
        kh, vh, base = _held(0, k_new, v_new)
        words = SpeckvKVConnector.tree_masks([-1, 0], base)
        row = H * D
        reqs = [conn.requests[r] for r in RIDS]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dk, dv, dm = dev(_rows_of(q5)), dev(np.nan_to_num(kh)), dev(np.nan_to_num(vh)), dev(np.asarray(words, np.uint32).view(np.int32))
        off = dev(np.zeros(kh.size + 8, np.float16))
        out = torch.full((B, H, S * R, D), PATTERN, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        good = dict(k_handles=np.asarray([r.k_handle for r in reqs], np.uint64), v_handles=np.asarray([r.v_handle for r in reqs], np.uint64), layer=0,
                    d_q_f16=dq.data_ptr(), g=S * R, rows_per_pos=R, pos_end=np.asarray(_even(), np.uint32), d_k_held=dk.data_ptr(), d_v_held=dv.data_ptr(),
                    seq_stride_elems=(1 + S) * row, pos_stride_elems=row, d_mask=dm.data_ptr(), mask_stride=S, sm_scale=SM, d_out=out.data_ptr(), d_lse=0,
                    stream=st.cuda_stream)
        torch.cuda.synchronize()
        bad = [dict(rows_per_pos=0), dict(rows_per_pos=3), dict(g=17, rows_per_pos=1, mask_stride=17), dict(d_k_held=0), dict(d_v_held=0), dict(d_mask=0),
               dict(mask_stride=1), dict(seq_stride_elems=3 * row + 4), dict(pos_stride_elems=row + 4), dict(pos_stride_elems=row - 8),
               dict(d_k_held=off.data_ptr() + 8), dict(d_v_held=off.data_ptr() + 8), dict(g=0), dict(g=20), dict(layer=L)]
        for change in bad:
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec(**dict(good, **change))
            assert e.value.status == -4, change
        capturing = torch.cuda.Stream()
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with graph_capture(graph, capturing):
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec(**dict(good, stream=capturing.cuda_stream))
            assert e.value.status == -4
            bump.add_(1)
        del graph
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == PATTERN).all()
        lib.attend_kv_spec(**good)                                                    # and the good set goes through
        torch.cuda.synchronize()
        assert not (out.cpu().numpy().view(np.uint32) == PATTERN).any()


def test_two_calls_on_two_streams(oracle):
    torch = torch_mod()
    S, R = 4, 4
    q5, k_new, v_new = _step(S, R)
    q5b = _step(S, R, seed=1)[0]
    with kd._batch(torch, _members()) as (lib, conn):
        try:
            set_tuning("attend_tiles_per_split", 1)                                  # both calls leave partials in the one scratch buffer
            kh, vh, base = _held(1, k_new, v_new)
            words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base)
            reqs = [conn.requests[r] for r in RIDS]
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            dk, dv, dm = dev(kh), dev(vh), dev(np.asarray(words, np.uint32).view(np.int32))
            streams, qs, outs = [torch.cuda.Stream(), torch.cuda.Stream()], [dev(_rows_of(q5)), dev(_rows_of(q5b))], []
            torch.cuda.synchronize()
            for st, dq in zip(streams, qs):
                out = torch.full((B, H, S * R, D), PATTERN, dtype=torch.int32, device="cuda")
                lse = torch.full((B, H, S * R), PATTERN, dtype=torch.int32, device="cuda")
                outs.append((out, lse))
                lib.attend_kv_spec(np.asarray([r.k_handle for r in reqs], np.uint64), np.asarray([r.v_handle for r in reqs], np.uint64), 1, dq.data_ptr(),
                                   S * R, R, np.asarray(_even(), np.uint32), dk.data_ptr(), dv.data_ptr(), (1 + S) * H * D, H * D, dm.data_ptr(), S, SM,
                                   out.data_ptr(), lse.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            for q, (out, lse), name in zip((q5, q5b), outs, "ab"):
                want = _want(_pair(oracle, 1), _rows_of(q), R, _even(), kh, vh, words)
                _compare(want, out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32), f"attend_kv_spec two streams, call {name}")
        finally:
            set_tuning("attend_tiles_per_split", 0)


# ----------------------------------------------------------------------------- 7. the example, and a walk over several steps
def test_the_example_runs():
    """examples/k8v4_spec_example.py in this process, short: a chain step and a tree step per round, every layer checked inside the example
    against attend_chunk"""
    import importlib.util
    torch_mod()
    spec = importlib.util.spec_from_file_location("k8v4_spec_example", os.path.join(ROOT, "examples", "k8v4_spec_example.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(rounds=2, verbose=False) == 2


def test_a_walk_of_steps_and_commits_across_the_seams(oracle):
    """prefill, then attend_spec and commit of a varying accepted count, four steps: lengths cross odd and even seams and tile edges; every
    step is checked against float64 over what the pool then holds (the oracle's records of the rows written so far)"""
    torch = torch_mod()
    S, R = 3, 4
    rng = np.random.default_rng(977)
    starts = [0, 1, 31]
    accepts = [[1, 3, 2], [2, 0, 3], [3, 1, 1], [1, 2, 0]]
    Bw = len(starts)
    rows_k = [kd._rows(rng, L, 96, H, D) for _ in starts]                              # every member's own sequence of positions
    rows_v = [kd._rows(rng, L, 96, H, D) for _ in starts]
    with kd._batch(torch, [(k[:, :n], v[:, :n]) for k, v, n in zip(rows_k, rows_v, starts)]) as (lib, conn):
        lengths, parities = list(starts), set()
        rids = list(range(Bw))
        for step, accept in enumerate(accepts):
            q5 = kd._rows(rng, Bw, S, H, R, D)
            # the drafts: the true next positions up to the accepted count, then rows that will be thrown away
            k_new, v_new = kd._rows(rng, Bw, S, L, H, D), kd._rows(rng, Bw, S, L, H, D)
            for b in range(Bw):
                for t in range(accept[b]):
                    k_new[b, t], v_new[b, t] = rows_k[b][:, lengths[b] + t], rows_v[b][:, lengths[b] + t]
            dq, dk, dv = (torch.from_numpy(a).cuda() for a in (q5, k_new, v_new))
            layer = step % L
            got = conn.attend_spec(layer, rids, dq, dk, dv, SM)
            torch.cuda.synchronize()
            base = [n & 1 for n in lengths]
            parities.update(base)
            words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), base)
            worst = 0.0
            for b in range(Bw):                                                       # every member over its own content
                pair = kd._checker(oracle, ("walk", b, lengths[b] & ~1), rows_k[b][:, :lengths[b] & ~1], rows_v[b][:, :lengths[b] & ~1], layer) \
                    if lengths[b] >= 2 else _pair(oracle, layer)
                kh, vh, _ = _held(layer, k_new[b:b + 1], v_new[b:b + 1], [lengths[b]], (rows_k[b], rows_v[b]))
                want = _want(pair, _rows_of(q5[b:b + 1]), R, [lengths[b] & ~1], kh, vh, words[b:b + 1])
                worst = max(worst, _compare(want, _rows_of(got[b:b + 1].cpu().numpy()), None, f"walk step {step} member {b} length {lengths[b]}"))
            keep = conn.commit(rids, dk, dv, accept)
            torch.cuda.synchronize()
            del keep
            lengths = [n + a for n, a in zip(lengths, accept)]
            assert [conn.length(r) for r in rids] == lengths
        assert parities == {0, 1}                                                     # steps began on odd and on even lengths
