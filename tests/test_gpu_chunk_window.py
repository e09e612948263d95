"""-m gpu: chunk attention under a sliding window -- speckv_ext_attend_chunk_window (k_attend_chunk's WINDOW form, whole and split) and
SpeckvKVConnector.attend_chunk(window=...) on top of it.

Reference and bound are those of tests/test_gpu_chunk.py, unchanged but for the lower bound: numpy float64 softmax attention with the
fp16 query as given, the oracle's records (HeadChecker.kv) for the stored part, the fp16 held rows for the rest; row j at the absolute
position P sees the absolute positions [max(0, P + 1 - W), P].  |err| <= 2e-3 sum p|v| + 1e-6 and |lse err| <= 2e-3; the bound scales
with what a row sees, so it needs no change under a window.

Shapes: L = 2, T = 256, 8 x 128 heads, the ragged batch of tests/test_gpu_chunk.py (prompts of 0, 1, 2, 37, 64, 98 positions, S = 70
with 70, 33, 17, 16, 1, 0 live); the split form at T = 512 over the prompts of tests/test_gpu_chunk_split.py (up to 481 positions)."""
import numpy as np
import pytest

from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import test_gpu_chunk_split as split
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_chunk import (L, LAYER, N_NEW, PATTERN, PROMPTS, RIDS, S, SM, T, _batch, _f16_times, _f32, _inputs, _kscale, _rows,
                                  _stored64)
from tests.test_gpu_chunk import _entry as _causal_entry
from tests.test_gpu_spec_step import SCHEMES, _region

pytestmark = pytest.mark.gpu
ALL = ["fp8", "int4", "mxfp4"]
WINDOWS = [1, 2, 31, 32, 33, 40, 64, 100]


def _entry(torch, lib, conn, rids, q, k_new, v_new, n_new, window, n_splits=1, **kw):
    """speckv_ext_attend_chunk_window over what the connector holds: (out, lse) as numpy int32 bit patterns"""
    _, args, out, lse, st, held = split._stage(torch, conn, rids, q, k_new, v_new, n_new, None, entry="causal", **kw)
    args.setdefault("window", window)
    args.setdefault("n_splits", n_splits)
    torch.cuda.synchronize()
    lib.attend_chunk_window(**args)
    st.synchronize()
    del held
    return out.cpu().numpy(), lse.cpu().numpy()


def _scores(K, V, tail, q, kn, vn):
    """float64 scores of q [n][R][D] against everything the request holds and the new rows, by absolute position: (s [n R][P], V [P][D])"""
    n, R, _ = q.shape
    parts_k, parts_v = [K], [V]
    if tail is not None:
        parts_k.append(tail[0][None].astype(np.float64)); parts_v.append(tail[1][None].astype(np.float64))
    Ka, Va = np.concatenate(parts_k + [kn.astype(np.float64)]), np.concatenate(parts_v + [vn.astype(np.float64)])
    return (q.astype(np.float64).reshape(n * R, D) @ Ka.T) * SM, Va, len(K) + (tail is not None)


def _windowed(s, Va, held_from, n, R, window):
    """the reference of tests/test_gpu_chunk.py with the lower bound: row j sees the absolute positions [max(0, P + 1 - W), P],
    P = held_from + j -> out [n][R][D], lse [n][R], mag = sum p|v|"""
    s = s.copy()
    sees = held_from + np.arange(n * R) // R + 1                             # P + 1: itself included
    at = np.arange(Va.shape[0])[None, :]
    s[(at >= sees[:, None]) | (at < np.maximum(0, sees - window)[:, None])] = -np.inf
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return ((p @ Va) / l[:, None]).reshape(n, R, D), (mx + np.log(l)).reshape(n, R), ((p @ np.abs(Va)) / l[:, None]).reshape(n, R, D)


def _check(stored, conn, b, rid, prompt, q, new, n, outs, what, layer=LAYER):
    """rows of request b's first n new positions against float64 at `layer` for every (window, out, lse) of outs -- the scores are
    computed once per head and shared by the windows; stored(k, v, head) gives the float64 rows of the oracle's records; lse None:
    the output only.  Returns the worst err / tol per window"""
    k, v = prompt
    even = k.shape[1] & ~1
    r = conn.requests[rid]
    worst = {w: 0.0 for w, _, _ in outs}
    for head in range(H):
        K, V = stored(k, v, head)
        tail = None if not r.length & 1 else (r.tail_k[layer, head].cpu().numpy(), r.tail_v[layer, head].cpu().numpy())
        s, Va, held_from = _scores(K[:even], V[:even], tail, q[b, :n, head], new[0][b, :n, layer, head], new[1][b, :n, layer, head])
        for w, out, lse in outs:
            want, wlse, mag = _windowed(s, Va, held_from, n, q.shape[3], w)
            got = _f32(out)[b, :n, head]
            assert np.all(np.isfinite(got)), (what, w, b, head, "not finite")
            err, tol = np.abs(got - want), 2e-3 * mag + 1e-6
            lerr = np.zeros(1) if lse is None else np.abs(_f32(lse)[b, :n, head] - wlse)
            worst[w] = max(worst[w], float((err / tol).max()), float(lerr.max() / 2e-3))
            assert np.all(err <= tol), (what, w, b, head, "out", float((err / tol).max()))
            assert np.all(lerr <= 2e-3), (what, w, b, head, "lse", float(lerr.max()))
    return worst


def _stored256(oracle, scheme, b, layer=LAYER):
    return lambda k, v, head: _stored64(oracle, scheme, b, k, v, head, layer)


def _merge_worst(into, worst):
    for w, x in worst.items():
        into[w] = max(into.get(w, 0.0), x)


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_windows_against_float64(oracle, scheme, rpp):
    """the ragged batch at both layers under windows of 1 (itself only), 2 (an odd bound: one position of a page), 31 / 32 / 33
    (around a tile), 40, 64 and 100 (beyond the short prompts, inside the long one): the bound falls inside a pool tile and on its
    edge, inside the last partial pool tile, on the pool / held seam and on the tail, and inside held tiles, where later query blocks
    read no pool tile at all"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        for layer in range(L):
            outs = [(w,) + _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, w, layer=layer) for w in WINDOWS]
            worst = {}
            for b in RIDS:
                if N_NEW[b]:
                    _merge_worst(worst, _check(_stored256(oracle, scheme, b, layer), conn, b, b, prompts[b], q, new, N_NEW[b], outs,
                                               ("window", scheme, rpp, layer), layer=layer))
            print(f"attend_chunk_window {scheme} rows_per_pos {rpp} layer {layer}: worst err / tol " +
                  ", ".join(f"W {w}: {x:.3f}" for w, x in worst.items()))


# ----------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_a_window_that_cuts_nothing_gives_the_unwindowed_bits_and_one_position_less_moves_one_row(scheme, rpp):
    """window >= everything every request holds (and window 0): out / lse are speckv_ext_attend_chunk's, bit for bit -- the engine
    issues that launch.  window = 69, one less than what the longest request's last row sees (request 0: 70 positions): the call
    runs on the WINDOW instances, that one position's rows differ, and every other row -- all of them in blocks that start at tile
    0 -- keeps the unwindowed call's bits: the same arithmetic in the same order"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    with _batch(torch, scheme, prompts) as (lib, conn):
        want = _causal_entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, fill=PATTERN)
        assert not np.all(want[0] == PATTERN)
        reach = max(p + n for p, n in zip(PROMPTS, N_NEW) if n)
        assert reach == 70
        for window, n_splits in ((0, 1), (reach, 1), (reach, 0), (reach, 5), (10 ** 6, 1), (0xFFFFFFFF, 0)):
            got = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, window, n_splits, fill=PATTERN)
            if n_splits == 5:                               # forced pieces without a window: the split entry's bits
                want5 = split._entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, 5, fill=PATTERN)
                assert np.array_equal(got[0], want5[0]) and np.array_equal(got[1], want5[1]), (scheme, rpp, window, "forced 5")
            else:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (scheme, rpp, window, n_splits)
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, reach - 1, fill=PATTERN)
        assert (out[0, 69] != want[0][0, 69]).any(axis=-1).all() and (lse[0, 69] != want[1][0, 69]).all()
        same_out, same_lse = out == want[0], lse == want[1]
        same_out[0, 69], same_lse[0, 69] = True, True
        assert same_out.all() and same_lse.all(), (scheme, rpp, "a row that loses no position changed its bits")


# ----------------------------------------------------------------------------- 3. not written
@pytest.mark.parametrize("scheme", ALL)
def test_rows_of_positions_that_are_not_live_are_not_written(scheme):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts) as (lib, conn):
        for window, n_splits in ((33, 1), (1, 1), (33, 3)):
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, window, n_splits, fill=PATTERN)
            for b, n in enumerate(N_NEW):
                assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, window, b)
                assert np.all(np.isfinite(_f32(out)[b, :n])) and np.all(np.isfinite(_f32(lse)[b, :n])), (scheme, window, b)
                assert not np.any(lse[b, :n] == PATTERN) and not np.any(np.all(out[b, :n] == PATTERN, axis=-1))


# ----------------------------------------------------------------------------- 4. the window probe
PROBE_NEW = {1: (0, 1, 15, 16, 69), 33: (0, 3, 4, 31, 32, 36, 37), 64: (0, 5, 6, 31, 32)}
# stored positions of the 98-position prompt on both sides of lo(0) = 99 - W and of tile and page edges: W = 33 -> lo(j) = 66 + j,
# W = 64 -> lo(j) = 35 + j, W = 1 -> no stored position is seen
PROBE_STORED = {1: (97,), 33: (64, 65, 66, 67, 97), 64: (31, 34, 35, 36, 63, 64)}


@pytest.mark.parametrize("scheme", ALL)
def test_the_window_probe_on_new_rows(scheme):
    """new row a replaced by other values: exactly the rows a <= j < a + W change, every other row keeps its bits -- a on both sides
    of query-block edges (16 positions at rows_per_pos 4), of held tiles (32; requests with a tail are shifted by one) and of the
    bound itself"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    other = np.random.default_rng(5).standard_normal((2,) + new[0].shape).astype(np.float16)
    with _batch(torch, scheme, prompts) as (lib, conn):
        for window, places in PROBE_NEW.items():
            out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, window)
            for a in places:
                k2, v2 = new[0].copy(), new[1].copy()
                k2[:, a], v2[:, a] = other[0][:, a], other[1][:, a]
                out2, lse2 = _entry(torch, lib, conn, RIDS, q, k2, v2, N_NEW, window)
                for b, n in enumerate(N_NEW):
                    if n == 0:
                        continue
                    sees = np.asarray([a <= j < a + window for j in range(n)], bool)
                    changed = (out2[b, :n] != out[b, :n]).any(axis=-1).reshape(n, -1)
                    assert changed[sees].all(), (scheme, window, a, b, "a row that sees the replaced position kept its bits")
                    assert not changed[~sees].any() and np.array_equal(lse2[b, :n][~sees], lse[b, :n][~sees]), (scheme, window, a, b)


@pytest.mark.parametrize("scheme", ALL)
def test_the_window_probe_on_stored_positions(scheme):
    """stored position t of the 98-position prompt negated (a record's scales stay: the other position of its page keeps its bits):
    exactly the rows with lo(j) <= t change, every other row keeps its bits; t on both sides of lo(0), of a page and of a tile"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    k, v = prompts[5]
    places = sorted({t for ts in PROBE_STORED.values() for t in ts})
    variants = []
    for t in places:
        k2, v2 = k.copy(), v.copy()
        k2[:, t], v2[:, t] = -k2[:, t], -v2[:, t]
        variants.append((k2, v2))
    n = S
    with _batch(torch, scheme, [prompts[5]] + variants) as (lib, conn):
        one = lambda rid, window: _entry(torch, lib, conn, [rid], q[5:6], new[0][5:6], new[1][5:6], [n], window)
        for window, ts in PROBE_STORED.items():
            out, lse = one(0, window)
            for t in ts:
                out2, lse2 = one(1 + places.index(t), window)
                sees = np.asarray([max(0, 98 + j + 1 - window) <= t for j in range(n)], bool)
                changed = (out2[0] != out[0]).any(axis=-1).reshape(n, -1)
                assert changed[sees].all(), (scheme, window, t, "a row that sees the replaced position kept its bits")
                assert not changed[~sees].any() and np.array_equal(lse2[0][~sees], lse[0][~sees]), (scheme, window, t)
            assert sees.any() == (window != 1)


# ----------------------------------------------------------------------------- 5. hostile rows below the window
def _hostile(x, rows, kind):
    x = x.copy()
    if kind == "k":
        x[rows] = (x[rows].astype(np.float32) * 200).astype(np.float16)
    else:
        x[rows] = np.where(x[rows] < 0, np.float16(-1000), np.float16(1000))
    return x


@pytest.mark.parametrize("rpp", [1, 4])
@pytest.mark.parametrize("scheme", ALL)
def test_hostile_rows_below_the_window_stay_out(oracle, scheme, rpp):
    """a prompt of 98 positions whose positions [0, 48) are K x 200, V = +-1000 under W = 40, S = 16 (lo(0) = 59: no row sees them),
    and new positions 0..20 of a 70-position step with V = +-1000 under W = 8 (rows j >= 28 see none of them): every row within the
    float64 bound, whose sum p|v| runs over what the row sees"""
    torch = torch_mod()
    prompts, new, q = _inputs(rpp)
    k, v = prompts[5]
    below = np.arange(48)
    hk = np.stack([_hostile(k[layer], below, "k") for layer in range(L)])
    hv = np.stack([_hostile(v[layer], below, "v") for layer in range(L)])
    new_v = new[1].copy()
    new_v[:, :21] = np.where(new_v[:, :21] < 0, np.float16(-1000), np.float16(1000))
    with _batch(torch, scheme, [(hk, hv), prompts[5]]) as (lib, conn):
        out, lse = _entry(torch, lib, conn, [0], q[5:6], new[0][5:6], new[1][5:6], [16], 40)
        stored = lambda kk, vv, head: _stored64(oracle, scheme, 5, kk, vv, head)
        worst = _check(stored, conn, 0, 0, (hk, hv), q[5:6], (new[0][5:6], new[1][5:6]), 16, [(40, out, lse)], ("hostile prompt", scheme, rpp))
        print(f"attend_chunk_window {scheme} rows_per_pos {rpp} hostile stored rows below W 40: worst err / tol {worst[40]:.3f}")
        for n_splits in (1, 3):
            out, lse = _entry(torch, lib, conn, [1], q[5:6], new[0][5:6], new_v[5:6], [S], 8, n_splits)
            worst = _check(stored, conn, 0, 1, prompts[5], q[5:6], (new[0][5:6], new_v[5:6]), S, [(8, out, lse)], ("hostile new rows", scheme, rpp))
            print(f"attend_chunk_window {scheme} rows_per_pos {rpp} hostile new rows below W 8, n_splits {n_splits}: worst err / tol {worst[8]:.3f}")


# ----------------------------------------------------------------------------- 6. split
N_SPLIT = [70, 33, 0, 16, 1, 70, 70]                # over split.PROMPTS = 0, 1, 2, 37, 98, 255, 481


@pytest.mark.parametrize("n_splits", [2, 3, 5, 0])
@pytest.mark.parametrize("scheme", ALL)
def test_pieces_under_a_window_against_float64(oracle, scheme, n_splits):
    """T = 512, prompts up to 481 positions, forced 2, 3, 5 pieces and the rule, W in {33, 100, 300}: whole sequences start at a
    first tile > 0, and later query blocks have EMPTY pieces (rows_per_pos 8: 9 blocks of 8 positions; 1: 2 blocks).  Every live row
    finite and within the float64 bound, dead rows keep the fill pattern"""
    torch = torch_mod()
    t = split.T
    with split._batch(torch, scheme, split._inputs(8)[0]) as (lib, conn):
        for rpp in (8, 1):
            prompts, new, q = split._inputs(rpp)
            outs = [(w,) + _entry(torch, lib, conn, split.RIDS, q, new[0], new[1], N_SPLIT, w, n_splits, fill=PATTERN) for w in (33, 100, 300)]
            if n_splits:
                # the plan the engine makes: empty pieces and late first tiles do occur
                plans = [type(conn).chunk_pieces(N_SPLIT, split.PROMPTS, rpp, n_splits, 256, window=w) for w, _, _ in outs]
                assert any(f > 0 and p > 1 for plan in plans for p, f in zip(plan[0], plan[3]))
            worst = {}
            for b in split.RIDS:
                n = N_SPLIT[b]
                for w, out, lse in outs:
                    assert np.all(out[b, n:] == PATTERN) and np.all(lse[b, n:] == PATTERN), (scheme, n_splits, w, b)
                    assert np.all(np.isfinite(_f32(out)[b, :n])) and np.all(np.isfinite(_f32(lse)[b, :n])), (scheme, n_splits, w, b)
                if n:
                    stored = lambda k, v, head: split._stored64(oracle, scheme, k, v, head, LAYER, t)
                    _merge_worst(worst, _check(stored, conn, b, b, prompts[b], q, new, n, outs, ("pieces", scheme, n_splits, rpp)))
            print(f"attend_chunk_window {scheme} n_splits {n_splits} rows_per_pos {rpp}: worst err / tol " +
                  ", ".join(f"W {w}: {x:.3f}" for w, x in worst.items()))


# ----------------------------------------------------------------------------- 7. placement
@pytest.mark.parametrize("scheme", ALL)
def test_a_window_over_a_pool_striped_over_three(oracle, scheme):
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, scheme, prompts, SPECKV_POOL_DEVICES="0,0,0") as (lib, conn):
        outs = [(w,) + _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, w) for w in (40,)]
        worst = {}
        for b in RIDS:
            if N_NEW[b]:
                _merge_worst(worst, _check(_stored256(oracle, scheme, b), conn, b, b, prompts[b], q, new, N_NEW[b], outs, ("striped", scheme)))
        print(f"attend_chunk_window {scheme} striped over 3, W 40: worst err / tol {worst[40]:.3f}")


@pytest.mark.parametrize("scheme", ALL)
def test_pages_never_written_inside_the_window_count_as_zeros(oracle, scheme):
    """an allocation written through speckv_write except K page 13, V page 14 (positions 26..29) and the whole second tile of
    pos_end = 64, under W = 40 with 33 new positions (lo(0) = 25): all of them inside the window of some row.  A never-written K row
    scores 0, not -inf, a never-written V row adds nothing: within the float64 bound of the same prompt with zeros there"""
    import types
    torch = torch_mod()
    _, new, q = _inputs(4)
    rng = np.random.default_rng(71)
    k, v = _rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D)
    k[:, 26:28] = 0; v[:, 28:30] = 0
    k[:, 32:] = 0; v[:, 32:] = 0
    with _batch(torch, scheme, []) as (lib, conn):
        lib.set_compression_scheme(SCHEMES[scheme])
        h = lib.alloc(2 * T * L * H * D * 2)
        lib.set_layout(h, T, L, H, D, 2)
        page = lambda x, first, n: np.ascontiguousarray(x[LAYER, 2 * first:2 * (first + n)]).reshape(n, 2 * H * D)
        for x, region, skip in ((k, LAYER * T, 13), (v, LAYER * T + T // 2, 14)):
            for first, n in ((0, skip), (skip + 1, 16 - skip - 1)):
                img = page(x, first, n)
                lib.write(h, (region + first) * 4096, img.ctypes.data, img.nbytes, False)
        lib.sync()
        held = types.SimpleNamespace(requests={0: types.SimpleNamespace(handle=h, length=64, tail_k=None, tail_v=None)})
        n = 33
        out, lse = _entry(torch, lib, held, [0], q[:1], new[0][:1], new[1][:1], [n], 40, fill=PATTERN)
        assert np.all(out[0, n:] == PATTERN) and np.all(lse[0, n:] == PATTERN)
        stored = lambda kk, vv, head: _stored64(oracle, scheme, 0, kk, vv, head)
        worst = _check(stored, held, 0, 0, (k, v), q, new, n, [(40, out, lse)], ("never written", scheme))
        print(f"attend_chunk_window {scheme} never-written pages inside W 40: worst err / tol {worst[40]:.3f}")
        lib.free(h)


# ----------------------------------------------------------------------------- 8. through the connector
@pytest.mark.parametrize("scheme", ALL)
def test_connector_attend_chunk_with_a_window(scheme):
    """attend_chunk(window=W) gives the entry's bits and zeros for the rows that are not live, with splits=0 and a forced count too;
    window=None / 0 gives the bits of the call without the argument; no state changes"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    dev = lambda x: torch.from_numpy(x).cuda()
    with _batch(torch, scheme, prompts) as (lib, conn):
        lengths = [conn.length(r) for r in RIDS]
        plain = conn.attend_chunk(LAYER, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW).cpu().numpy()
        for window in (None, 0):
            got = conn.attend_chunk(LAYER, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW, window=window).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
        for window, splits in ((33, 1), (33, 0), (8, 3), (1, 1)):
            out, _ = _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, window, splits)
            got = conn.attend_chunk(LAYER, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW, splits=splits, window=window)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            for b, n in enumerate(N_NEW):
                assert np.array_equal(got[b, :n].view(np.uint32), out[b, :n].view(np.uint32)), (scheme, window, splits, b)
                assert not got[b, n:].any()
        assert [conn.length(r) for r in RIDS] == lengths                  # no state changes
        with pytest.raises(ValueError, match="window"):
            conn.attend_chunk(LAYER, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW, parents=[-1] + list(range(S - 1)), window=8)


@pytest.mark.parametrize("scheme", ALL)
def test_windowed_decode_steps_through_the_connector(oracle, scheme):
    """S = 1 with a window -- the windowed DECODE step -- over requests of 0, 1, 2, 37, 64 and 98 positions (odd and even lengths, an
    empty request, a tail only) against float64, with splits=0"""
    torch = torch_mod()
    prompts, new, q = _inputs(8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q1, new1 = q[:, :1], (new[0][:, :1], new[1][:, :1])
    with _batch(torch, scheme, prompts) as (lib, conn):
        for layer in range(L):
            outs = []
            for w in (1, 2, 33, 40):
                got = conn.attend_chunk(layer, RIDS, dev(q1), dev(new1[0]), dev(new1[1]), SM, splits=0, window=w)
                torch.cuda.synchronize()
                outs.append((w, got.cpu().numpy(), None))
            worst = {}
            for b in RIDS:
                _merge_worst(worst, _check(_stored256(oracle, scheme, b, layer), conn, b, b, prompts[b], q1, new1, 1, outs, ("decode", scheme, layer),
                                           layer=layer))
            print(f"attend_chunk(window) {scheme} S = 1 layer {layer}: worst err / tol " + ", ".join(f"W {w}: {x:.3f}" for w, x in worst.items()))


@pytest.mark.parametrize("scheme", ALL)
def test_connector_window_with_a_k_pre_scale_before_and_after_a_commit(oracle, scheme):
    """attend_chunk(window=40) of a connector with set_k_channel_scale against float64 over what the kernel is given (the oracle's
    records of k / scale, k_new / scale and q x scale); then the chunk is committed and a second chunk attends over the longer
    requests"""
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    ks = _kscale()
    inv = 1.0 / ks
    dev = lambda x: torch.from_numpy(x).cuda()
    pre = [(_f16_times(k, inv[:, None]), v) for k, v in prompts]
    new_pre = (_f16_times(new[0], inv[None, None]), new[1])
    rng = np.random.default_rng(66)
    S2 = 20
    new2, q2 = (_rows(rng, len(RIDS), S2, L, H, D), _rows(rng, len(RIDS), S2, L, H, D)), _rows(rng, len(RIDS), S2, H, 4, D)
    new2_pre = (_f16_times(new2[0], inv[None, None]), new2[1])
    with _batch(torch, scheme, prompts, kscale=ks) as (lib, conn):
        qs = _f16_times(q, ks[LAYER][None, None, :, None, :])
        got = conn.attend_chunk(LAYER, RIDS, dev(q), dev(new[0]), dev(new[1]), SM, N_NEW, window=40)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        worst = {}
        for b in RIDS:
            if N_NEW[b]:
                _merge_worst(worst, _check(_stored256(oracle, scheme, b), conn, b, b, pre[b], qs, new_pre, N_NEW[b], [(40, got, None)], ("pre-scale", scheme)))
        keep = conn.commit(RIDS, dev(new[0]), dev(new[1]), [range(n) for n in N_NEW])
        torch.cuda.synchronize()
        longer = [(np.concatenate([pre[b][0], new_pre[0][b, :n].transpose(1, 0, 2, 3)], axis=1),
                   np.concatenate([pre[b][1], new_pre[1][b, :n].transpose(1, 0, 2, 3)], axis=1)) for b, n in enumerate(N_NEW)]
        qs2 = _f16_times(q2, ks[LAYER][None, None, :, None, :])
        got = conn.attend_chunk(LAYER, RIDS, dev(q2), dev(new2[0]), dev(new2[1]), SM, window=40)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        after = {}
        for b in RIDS:
            _merge_worst(after, _check(_stored256(oracle, scheme, b), conn, b, b, longer[b], qs2, new2_pre, S2, [(40, got, None)], ("pre-scale, committed", scheme)))
        print(f"attend_chunk(window=40) {scheme} K pre-scale: worst err / tol {worst[40]:.3f}, after a commit {after[40]:.3f}")
        del keep


# ----------------------------------------------------------------------------- 9. refusals at the entry
def test_the_window_entry_refuses_bad_arguments_and_capture():
    torch = torch_mod()
    prompts, new, q = _inputs(4)
    with _batch(torch, "fp8", prompts) as (lib, conn):
        pos_end = np.asarray([p & ~1 for p in PROMPTS], np.uint32)
        odd = pos_end.copy(); odd[3] = 35
        before = bytes(lib.stats())
        invalid = {"rows_per_pos 3": dict(rows_per_pos=3), "n_q > C": dict(n_q=np.asarray([S + 1] + N_NEW[1:], np.uint32)),
                   "an odd pos_end": dict(pos_end=odd), "n_splits 65": dict(n_splits=65), "NULL stream": dict(stream=0)}
        for what, change in invalid.items():
            for window in (0, 33):
                with pytest.raises(SpeckvError) as e:
                    _entry(torch, lib, conn, RIDS, q, new[0], new[1], N_NEW, window, fill=PATTERN, **change)
                    pytest.fail(what)
                assert e.value.status == -4, (what, window, e.value.status)     # SPECKV_ERR_INVAL
        torch.cuda.synchronize()
        assert bytes(lib.stats()) == before, "a refused call counted something"
        out, lse = _entry(torch, lib, conn, RIDS, q, new[0], new[1], [0] * len(RIDS), 33, fill=PATTERN)      # nothing to do
        assert np.all(out == PATTERN) and np.all(lse == PATTERN)
        # capture: refused, nothing launched
        s = torch.cuda.Stream()
        _, args, out, lse, _, held = split._stage(torch, conn, RIDS, q, new[0], new[1], N_NEW, None, entry="causal", fill=PATTERN, on=s)
        args.update(window=33, n_splits=1)
        lib.attend_chunk_window(**args)                                      # eager: fine
        torch.cuda.synchronize()
        eager = out.clone()
        out.fill_(PATTERN)
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            with pytest.raises(SpeckvError) as e:
                lib.attend_chunk_window(**args)
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert bool((out == PATTERN).all()) and not bool((eager == PATTERN).all())
        del held


# ----------------------------------------------------------------------------- 10. the example
def test_the_sliding_window_example_agrees_with_its_torch_reference():
    """examples/sliding_window_example.py in this process, short: local and global layers alternating, a prompt in chunks, S = 1 decode
    steps over odd and even lengths, every output against torch on the device"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "sliding_window_example.py")
    spec = importlib.util.spec_from_file_location("sliding_window_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run("fp8", window=40, chunks=(37, 70, 1), steps=3, verbose=False) == 111
