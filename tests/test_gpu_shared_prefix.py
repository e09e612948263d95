"""-m gpu: shared-prefix attention -- speckv_ext_attend_prefix_fold (k_attend_prefix whole and split, k_prefix_combine) and
SpeckvKVConnector.attend_shared / attend_chunk_shared on top of it.

Reference: numpy float64 softmax over three parts.  The prefix scores come from the fp16 query over the oracle's decoded prefix rows
[0, prefix_len) (HeadChecker.kv); the member's own stored scores from the query as the format's decode kernel takes it
(HeadChecker.q_rows) in a decode step, from the fp16 query on the chunk route; the tail and the new rows from the fp16 query.
Bounds, the project's, unchanged:
  decode steps     |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta from the own part as in want_rows
  the chunk route  |err| <= 2e-3 sum p|v| + 1e-6, |lse err| <= 2e-3

Shapes: L = 2, T = 256, 8 x 128 heads; prefix lengths 2, 36, 64, 98 and 254 of one 254-position prefix, members that hold 0, 1, 2, 37
and 64 positions of their own; the split cases at T = 512 over a 481-position prefix, as tests/test_gpu_chunk_split.py."""
import contextlib

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, graph_capture, torch_mod
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_spec_step import SCHEMES, _region

pytestmark = pytest.mark.gpu
ALL = ["fp8", "int4", "mxfp4"]
L, T, LAYER = 2, 256, 1
SM = 1.0 / np.sqrt(D)
PATTERN = 0x7C5A3B19
OWN = [0, 1, 2, 37, 64]                              # no pool and no tail, a tail only, one page, pool and tail, whole tiles
PLENS = [2, 36, 64, 98, 254]
P0, P1 = 100, 101                                    # request ids of prefixes
NEG_INF = np.float32(-np.inf).view(np.int32)

_data, _checkers = {}, {}


def _rows(rng, *shape):
    return rng.standard_normal(shape).astype(np.float16)


def _inputs(rpp):
    """the 254-position prefix, a second one of 64, the members' own prompts by length, 65 members' query rows: the same everywhere"""
    if "prefix" not in _data:
        rng = np.random.default_rng(3031)
        _data["prefix"] = (_rows(rng, L, 254, H, D), _rows(rng, L, 254, H, D))
        _data["second"] = (_rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D))
        _data["own"] = {n: (_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in OWN}
    if ("q", rpp) not in _data:
        _data[("q", rpp)] = _rows(np.random.default_rng(300 + rpp), 65, H, rpp, D)
    return _data["prefix"], _data["second"], _data["own"], _data[("q", rpp)]


def _checker(oracle, scheme, kv, layer, t=T):
    """the oracle's records of the even part of (k, v) [L][n][H][D] at `layer`, once per content"""
    k, v = kv
    key = (scheme, layer, t, k.shape[1], float(np.abs(k[layer].astype(np.float32)).sum()), float(np.abs(v[layer].astype(np.float32)).sum()))
    if key not in _checkers:
        even = k.shape[1] & ~1
        _checkers[key] = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], t), t)
    return _checkers[key]


@contextlib.contextmanager
def _world(torch, scheme, prefixes, owns, t=T, kscale=None, **env):
    """a connector that holds the prefixes {request id: (k, v)} and one member per entry of owns (request ids 0, 1, ...)"""
    lib = open_lib(**env) if env else pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, t, scheme)
        if kscale is not None:
            conn.set_k_channel_scale(torch.from_numpy(kscale).cuda())
        keep = []
        for rid, (k, v) in list(prefixes.items()) + list(enumerate(owns)):
            conn.add_request(rid)
            if k.shape[1]:
                keep += conn.write_prefill(rid, torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
        torch.cuda.synchronize()
        yield lib, conn
        torch.cuda.synchronize()
        del keep
    finally:
        lib.finalize()


def _own_step(torch, conn, layer, rids, q):
    """the members' own decode step as attend() issues it, with the log-sum-exp: (out [M][H][R][D], lse [M][H][R]) as int32 bit patterns"""
    out, lse, _ = conn._attend_layers_lse(layer, 1, rids, torch.from_numpy(np.ascontiguousarray(q)).cuda()[None], SM, None, None)
    torch.cuda.synchronize()
    return out[0].cpu().numpy().view(np.int32), lse[0].cpu().numpy().view(np.int32)


def _fold(torch, lib, handles, first, layer, q, lens, n_q, out, lse, n_splits=1, **change):
    """speckv_ext_attend_prefix_fold itself: q [M][C][H][R][D] fp16, out / lse int32 bit patterns of what the members hold going in ->
    (out, lse) bit patterns coming out.  change: arguments to replace (the refusals)"""
    M, C_, _, R, _ = q.shape
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    do, dl = torch.from_numpy(np.ascontiguousarray(out).reshape(M, C_, H, R, D)).cuda(), torch.from_numpy(np.ascontiguousarray(lse).reshape(M, C_, H, R)).cuda()
    st = torch.cuda.Stream()
    args = dict(prefix_handles=np.asarray(handles, np.uint64), first_member=np.asarray(first, np.uint32), layer=layer, d_q=dq.data_ptr(), C=C_,
                rows_per_pos=R, prefix_len=np.asarray(lens, np.uint32), n_q=np.asarray(n_q, np.uint32), n_splits=n_splits, sm_scale=SM,
                d_out=do.data_ptr(), d_lse=dl.data_ptr(), stream=st.cuda_stream)
    args.update(change)
    torch.cuda.synchronize()
    lib.attend_prefix_fold(**args)
    st.synchronize()
    torch.cuda.synchronize()
    return do.cpu().numpy().reshape(np.shape(out)), dl.cpu().numpy().reshape(np.shape(lse))


def _f32(x):
    return np.ascontiguousarray(x).view(np.float32)


def _softmax(S_, V_):
    s, Va = np.concatenate(S_, axis=1) * SM, np.concatenate(V_)
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return (p @ Va) / l[:, None], mx + np.log(l), (p @ np.abs(Va)) / l[:, None]


def _decode_ref(oracle, scheme, layer, q, members, t=T):
    """float64 of a decode step: q [M][H][R][D] fp16; members[m] = (prefix (k, v) or None, prefix_len, own (k, v) [L][n][H][D] -- all the
    member holds, an odd last position being its tail).  -> want [M][H][R][D], lse [M][H][R], mag, delta [M][H]"""
    M, _, R, _ = q.shape
    want, mag = np.zeros((M, H, R, D)), np.zeros((M, H, R, D))
    wlse, delta = np.full((M, H, R), -np.inf), np.zeros((M, H))
    quant = HeadChecker.q_rows
    for head in range(H):
        qf = q[:, head].astype(np.float64)
        qo = None
        for m, (prefix, plen, own) in enumerate(members):
            S_, V_ = [], []
            if plen:
                Kp, Vp = _checker(oracle, scheme, prefix, layer, t).kv(head)
                S_.append(qf[m] @ Kp[:plen].T); V_.append(Vp[:plen])
            n = own[0].shape[1]
            even = n & ~1
            if even:
                c = _checker(oracle, scheme, own, layer, t)
                if qo is None:
                    qo = quant(c, q[:, head]).reshape(M, R, D)                  # the query as the format's decode kernel takes it
                Ko, Vo = c.kv(head)
                S_.append(qo[m] @ Ko[:even].T); V_.append(Vo[:even])
                if scheme != "int4":
                    delta[m, head] = 3e-5 * float((np.abs(qo[m]) @ np.abs(Ko[:even]).T).max()) * SM
            if n & 1:
                S_.append(qf[m] @ own[0][layer, n - 1, head].astype(np.float64)[:, None]); V_.append(own[1][layer, n - 1, head].astype(np.float64)[None])
            if S_:
                want[m, head], wlse[m, head], mag[m, head] = _softmax(S_, V_)
    return want, wlse, mag, delta


def _assert_decode(got, got_lse, ref, what, members=None):
    """out [M][H][R][D] and lse [M][H][R] (None: the output only) as bit patterns against _decode_ref; prints and returns the worst err /
    tol.  members: the members to judge (default: all); every member's rows must be finite"""
    want, wlse, mag, delta = ref
    got = _f32(got).astype(np.float64)
    assert np.all(np.isfinite(got)), (what, "not finite")
    if members is not None:
        got, want, wlse, mag, delta = got[members], want[members], wlse[members], mag[members], delta[members]
        got_lse = None if got_lse is None else np.ascontiguousarray(got_lse)[members]
    live = np.isfinite(wlse)
    assert np.all(np.isfinite(got)), (what, "not finite")
    err, tol = np.abs(got - want), (2e-3 + 2 * delta)[:, :, None, None] * mag + 1e-6
    worst = float((err / tol).max())
    lworst = 0.0
    if got_lse is not None:
        lerr = np.abs(_f32(got_lse).astype(np.float64) - wlse)[live] / np.broadcast_to((2e-3 + delta)[:, :, None], wlse.shape)[live]
        lworst = float(lerr.max(initial=0.0))
    print(f"{what}: worst err / tol out {worst:.3f}, lse {lworst:.3f}")
    assert worst <= 1.0, (what, "out", worst, [int(x) for x in np.argwhere(err > tol)[0]])
    assert lworst <= 1.0, (what, "lse", lworst)
    return max(worst, lworst)


def _dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _shared(torch, conn, layer, rids, pids, q, lens=None, **kw):
    got = conn.attend_shared(layer, rids, pids, _dev(torch, q), SM, prefix_lens=lens, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.int32)


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("rpp,n", [(1, 65), (4, 17), (16, 5), (4, 1)])
@pytest.mark.parametrize("scheme", ALL)
def test_decode_steps_against_float64(oracle, scheme, rpp, n):
    """groups of 65 (rows_per_pos 1), 17 (4) and 5 (16) members -- each crosses a 64-row block -- and of one member; prefix lengths 2,
    36, 64, 98 and 254 and own lengths 0, 1, 2, 37 and 64 mixed; both layers.  The entry over the members' own (out, lse) against
    float64, and SpeckvKVConnector.attend_shared gives the entry's bits (splits 1 and the rule, which cuts nothing this short)"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(rpp)
    q, rids = q[:n], list(range(n))
    lens = [PLENS[(m + m // 5) % 5] for m in rids]
    mine = [owns[OWN[m % 5]] for m in rids]
    with _world(torch, scheme, {P0: prefix}, mine) as (lib, conn):
        for layer in range(L):
            out, lse = _own_step(torch, conn, layer, rids, q)
            got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, n], layer, q[:, None], lens, [1] * n, out, lse)
            ref = _decode_ref(oracle, scheme, layer, q, [(prefix, lens[m], mine[m]) for m in rids])
            _assert_decode(got, glse, ref, f"attend_prefix_fold {scheme} rows_per_pos {rpp} members {n} layer {layer}")
            for splits in (1, 0):
                via = _shared(torch, conn, layer, rids, [P0] * n, q, lens, splits=splits)
                assert np.array_equal(via, got), (scheme, rpp, n, layer, splits, "the connector does not give the entry's bits")


# ----------------------------------------------------------------------------- 2. groups, None, order
@pytest.mark.parametrize("scheme", ALL)
def test_two_groups_and_members_without_a_prefix_in_any_order(oracle, scheme):
    """two prefixes (254 and 64 positions) and members without one in one call: against float64, a member without a prefix keeps
    attend()'s bits, and interleaved members give, request by request, the bits of the grouped order"""
    torch = torch_mod()
    prefix, second, owns, q = _inputs(4)
    n = 9
    q, rids = q[:n], list(range(n))
    mine = [owns[OWN[m % 5]] for m in rids]
    pids = [P0, P1, None, P0, P1, None, P0, P0, P1]
    lens = [98, 64, 0, 254, 36, 0, 2, 64, 2]
    which = {P0: prefix, P1: second, None: None}
    with _world(torch, scheme, {P0: prefix, P1: second}, mine) as (lib, conn):
        got = _shared(torch, conn, LAYER, rids, pids, q, [x if p is not None else None for x, p in zip(lens, pids)])
        ref = _decode_ref(oracle, scheme, LAYER, q, [(which[pids[m]], lens[m], mine[m]) for m in rids])
        _assert_decode(got, None, ref, f"attend_shared {scheme} two groups and None, interleaved")
        plain = conn.attend(LAYER, rids, _dev(torch, q), SM)
        torch.cuda.synchronize()
        plain = plain.cpu().numpy().view(np.int32)
        for m in (2, 5):
            assert np.array_equal(got[m], plain[m]), (scheme, m, "a member without a prefix lost attend()'s bits")
        order, prefixes, first = SpeckvKVConnector.shared_groups(rids, pids)
        assert order != rids and prefixes == [P0, P1] and first == [0, 4, 7]
        grouped = _shared(torch, conn, LAYER, order, [pids[b] for b in order], q[order], [lens[b] if pids[b] is not None else None for b in order])
        assert np.array_equal(grouped, got[order]), (scheme, "interleaved members do not give the bits of the grouped order")


# ----------------------------------------------------------------------------- 3. different prefix_len inside one block
def _hostile(kv, rows):
    k, v = kv[0].copy(), kv[1].copy()
    k[:, rows] = (k[:, rows].astype(np.float32) * 200).astype(np.float16)
    v[:, rows] = np.where(v[:, rows] < 0, np.float16(-1000), np.float16(1000))
    return k, v


@pytest.mark.parametrize("scheme", ALL)
def test_members_of_one_block_see_their_own_length_of_the_prefix(oracle, scheme):
    """lengths 2, 36 and 98 over ONE 98-position prefix, all in one block.  The rows at and beyond a member's own length are made
    hostile FOR THAT MEMBER (K x 200, V = +-1000; finite): the block runs over the prefix with rows [2, 98) hostile, where the members
    of length 2 are judged, and over the prefix with rows [36, 98) hostile, where those of length 2 and 36 are -- no judged row sees a
    hostile position, as in every hostile-row test of the project, so a row that stays within its bound shows that the positions
    beyond its own length weigh nothing although its neighbours in the block walk them.  The members that SEE hostile rows are judged
    too where the reference holds the kernel's operands exactly (INT4, MXFP4: HeadChecker.kv rows are fp16 values); over FP8 its rows
    are the unrounded byte x scale, 2^-12 of a row x 200 = 0.1 of a score away from the fp16 values the decoder hands to the product,
    so there these rows are only required finite.  Then, over the same prefix without hostile rows (every position has a weight that
    shows), stored position t is replaced (negated: the record's scales stay): exactly the rows with prefix_len > t change, bit for
    bit elsewhere"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    calm = (prefix[0][:, :98], prefix[1][:, :98])
    hostile = {2: _hostile(calm, slice(2, 98)), 36: _hostile(calm, slice(36, 98))}
    ids = {2: P0, 36: 102}
    places = (0, 1, 2, 35, 36, 97)
    variants = {}
    for i, t_ in enumerate(places):
        k2, v2 = calm[0].copy(), calm[1].copy()
        k2[:, t_], v2[:, t_] = -k2[:, t_], -v2[:, t_]
        variants[110 + i] = (k2, v2)
    lens = [2, 36, 98, 98, 2, 36]
    mine = [owns[n] for n in (0, 37, 2, 0, 64, 1)]
    rids = list(range(len(lens)))
    q = q[:len(lens)]
    with _world(torch, scheme, {P0: hostile[2], 102: hostile[36], P1: calm, **variants}, mine) as (lib, conn):
        for layer in range(L):
            for h, pre in hostile.items():
                got = _shared(torch, conn, layer, rids, [ids[h]] * len(rids), q, lens)
                ref = _decode_ref(oracle, scheme, layer, q, [(pre, lens[m], mine[m]) for m in rids])
                judged = [m for m in rids if lens[m] <= h or scheme != "fp8"]
                _assert_decode(got, None, ref, f"attend_shared {scheme} lengths 2 / 36 / 98 in one block, rows from {h} on hostile, layer {layer}", judged)
        got = _shared(torch, conn, LAYER, rids, [P1] * len(rids), q, lens)
        for i, t_ in enumerate(places):
            other = _shared(torch, conn, LAYER, rids, [110 + i] * len(rids), q, lens)
            for m, n in enumerate(lens):
                changed = (other[m] != got[m]).any(axis=-1)
                if n > t_:
                    assert changed.all(), (scheme, t_, m, "a row that sees the replaced position kept its bits")
                else:
                    assert not changed.any(), (scheme, t_, m, "a row that does not see the replaced position changed")


# ----------------------------------------------------------------------------- 4. alone, in the group, in the call
@pytest.mark.parametrize("scheme", ALL)
def test_a_member_alone_gives_the_bits_it_gives_inside_its_group_and_inside_the_call(scheme):
    """unsplit: a row's walk and fold depend on its own prefix_len and on nothing else of the call (tiles beyond it add exact zeros)"""
    torch = torch_mod()
    prefix, second, owns, q = _inputs(4)
    n = 8
    q, rids = q[:n], list(range(n))
    mine = [owns[OWN[m % 5]] for m in rids]
    lens = [98, 2, 254, 36, 64, 64, 2, 36]
    with _world(torch, scheme, {P0: prefix, P1: second}, mine) as (lib, conn):
        h0, h1 = conn.requests[P0].handle, conn.requests[P1].handle
        out, lse = _own_step(torch, conn, LAYER, rids, q)
        call = _fold(torch, lib, [h0, h1], [0, 5, 8], LAYER, q[:, None], lens, [1] * n, out, lse)
        group = _fold(torch, lib, [h0], [0, 5], LAYER, q[:5, None], lens[:5], [1] * 5, out[:5], lse[:5])
        assert np.array_equal(group[0], call[0][:5]) and np.array_equal(group[1], call[1][:5])
        for m in rids:
            one = _fold(torch, lib, [h0 if m < 5 else h1], [0, 1], LAYER, q[m:m + 1, None], lens[m:m + 1], [1], out[m:m + 1], lse[m:m + 1])
            assert np.array_equal(one[0][0], call[0][m]) and np.array_equal(one[1][0], call[1][m]), (scheme, m)


# ----------------------------------------------------------------------------- 5. nothing of their own
@pytest.mark.parametrize("rpp", [1, 4, 16])
@pytest.mark.parametrize("scheme", ALL)
def test_members_with_nothing_of_their_own(oracle, scheme, rpp):
    """empty members through the connector, and the entry over out = 0, lse = -inf prefilled by hand: the same bits, and those are
    the prefix-only float64 attention (delta = 0: the prefix part takes the fp16 query)"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(rpp)
    n = 7
    q, rids, lens = q[:n], list(range(n)), [2, 36, 64, 98, 254, 98, 2]
    with _world(torch, scheme, {P0: prefix}, [owns[0]] * n) as (lib, conn):
        for layer in range(L):
            via = _shared(torch, conn, layer, rids, [P0] * n, q, lens)
            got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, n], layer, q[:, None], lens, [1] * n,
                              np.zeros((n, H, rpp, D), np.int32), np.full((n, H, rpp), NEG_INF, np.int32))
            assert np.array_equal(via, got), (scheme, rpp, layer)
            ref = _decode_ref(oracle, scheme, layer, q, [(prefix, lens[m], owns[0]) for m in rids])
            assert not ref[3].any()
            _assert_decode(got, glse, ref, f"attend_prefix_fold {scheme} rows_per_pos {rpp} prefix only, layer {layer}")


# ----------------------------------------------------------------------------- 6. dead pairs
@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("scheme", ALL)
def test_dead_pairs_and_members_without_prefix_positions_are_not_written(oracle, scheme, n_splits):
    """C = 3 with n_q = 3, 1, 0, 2, 3 and prefix_len 36, 98, 254, 0, 2: pairs at or beyond n_q and every pair of the member with
    prefix_len 0 keep the fill pattern in out and lse; the live pairs are the prefix-only attention"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    C_, n_q, lens = 3, [3, 1, 0, 2, 3], [36, 98, 254, 0, 2]
    M = len(n_q)
    qc = np.ascontiguousarray(_inputs(4)[3][:M * C_].reshape(M, C_, H, 4, D))
    live = np.asarray([[j < n_q[m] and lens[m] > 0 for j in range(C_)] for m in range(M)])
    out, lse = np.full((M, C_, H, 4, D), PATTERN, np.int32), np.full((M, C_, H, 4), PATTERN, np.int32)
    out[live], lse[live] = 0, NEG_INF
    with _world(torch, scheme, {P0: prefix}, []) as (lib, conn):
        got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, M], LAYER, qc, lens, n_q, out, lse, n_splits)
        assert np.all(got[~live] == PATTERN) and np.all(glse[~live] == PATTERN), (scheme, "a dead pair was written")
        assert not np.any(glse[live] == NEG_INF) and np.all(np.isfinite(_f32(got)[live]))
        flat = [(m, j) for m in range(M) for j in range(C_) if live[m, j]]
        ref = _decode_ref(oracle, scheme, LAYER, np.stack([qc[m, j] for m, j in flat]), [(prefix, lens[m], owns[0]) for m, _ in flat])
        _assert_decode(np.stack([got[m, j] for m, j in flat]), np.stack([glse[m, j] for m, j in flat]), ref,
                       f"attend_prefix_fold {scheme} C = 3 with dead pairs, n_splits {n_splits}")
        # nothing live at all: SPECKV_OK, nothing written
        got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, M], LAYER, qc, [0] * M, n_q, out, lse)
        assert np.array_equal(got, out) and np.array_equal(glse, lse)
        got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, M], LAYER, qc, lens, [0] * M, out, lse)
        assert np.array_equal(got, out) and np.array_equal(glse, lse)
        got, glse = _fold(torch, lib, [], [0], LAYER, qc, [], [], out, lse)
        assert np.array_equal(got, out) and np.array_equal(glse, lse)


# ----------------------------------------------------------------------------- 7. peaked scores
HEAD, SUB, VCONST = 5, 2, 6.0


@pytest.mark.parametrize("c", [0.75, 2.0])
@pytest.mark.parametrize("scheme", ALL)
def test_a_key_that_takes_nearly_all_the_weight(oracle, scheme, c):
    """a key c x the query row (member 0, HEAD, SUB) with a V row of 6.0, once in the prefix (positions 0, 33 and 97) and once in the
    member's own stored part (as _peaked of tests/test_gpu_chunk.py: c = 0.75 about 8, c = 2 about 22 natural units above the rest):
    the other side's fold weight underflows towards 0.  Every row against float64 under the decode bound"""
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    q = q[:3]
    needle = (np.float32(c) * q[0, HEAD, SUB].astype(np.float32)).astype(np.float16)
    cases = {}
    for at in (0, 33, 97):
        k, v = prefix[0][:, :98].copy(), prefix[1][:, :98].copy()
        k[LAYER, at, HEAD], v[LAYER, at, HEAD] = needle, np.float16(VCONST)
        cases[f"prefix-{at}"] = ((k, v), owns[64])
    k, v = owns[64][0].copy(), owns[64][1].copy()
    k[LAYER, 10, HEAD], v[LAYER, 10, HEAD] = needle, np.float16(VCONST)
    cases["own-10"] = ((prefix[0][:, :98], prefix[1][:, :98]), (k, v))
    for name, (pre, own) in cases.items():
        mine = [own, owns[37], owns[0]]
        with _world(torch, scheme, {P0: pre}, mine) as (lib, conn):
            out, lse = _own_step(torch, conn, LAYER, [0, 1, 2], q)
            got, glse = _fold(torch, lib, [conn.requests[P0].handle], [0, 3], LAYER, q[:, None], [98, 98, 36], [1] * 3, out, lse)
            ref = _decode_ref(oracle, scheme, LAYER, q, [(pre, 98, mine[0]), (pre, 98, mine[1]), (pre, 36, mine[2])])
            _assert_decode(got, glse, ref, f"attend_prefix_fold {scheme} needle {name} c {c}")
            side = _f32(got)[0, HEAD, SUB]
            if c == 2.0:
                assert np.all(np.abs(side - VCONST) < 0.05), (scheme, name, "the needle does not take the weight")


# ----------------------------------------------------------------------------- 8. split
T2 = 512


def _split_inputs():
    """a 481-position prefix with a needle in every tile (K x 3 at position 16 of each), members that see 34, 480 and 2 of it"""
    if "split" not in _data:
        rng = np.random.default_rng(4807)
        k, v = _rows(rng, L, 481, H, D), _rows(rng, L, 481, H, D)
        k[:, 16::32] = (k[:, 16::32].astype(np.float32) * 3).astype(np.float16)
        _data["split"] = (k, v)
    return _data["split"]


@pytest.mark.parametrize("rpp", [4, 1])
@pytest.mark.parametrize("scheme", ALL)
def test_pieces_over_a_long_prefix_against_float64(oracle, scheme, rpp):
    """T = 512, 15 tiles of a 481-position prefix (480 stored) cut into 2, 3, 5 and 16 (-> 15) pieces and by the rule; members that
    see 34 and 480 positions in one block, so the short ones have pieces beyond their prefix_len (m = -inf, l = 0, zeros); a needle
    in every piece.  Every plan against float64; a member alone whose length is the group's maximum gives, under a forced N, the
    bits it gives inside its group (the piece plan follows the group's maximum, so only such a member has the same plan alone)"""
    torch = torch_mod()
    _, _, owns, q = _inputs(rpp)
    prefix = _split_inputs()
    lens = [34, 480, 480, 34, 2, 480]
    mine = [owns[n] for n in (0, 37, 1, 64, 2, 0)]
    n = len(lens)
    q, rids = q[:n], list(range(n))
    with _world(torch, scheme, {P0: prefix}, mine, t=T2) as (lib, conn):
        assert type(conn).chunk_pieces([n], [480], rpp, 5, 256)[0] == [5]
        h = conn.requests[P0].handle
        for layer in range(L):
            out, lse = _own_step(torch, conn, layer, rids, q)
            ref = _decode_ref(oracle, scheme, layer, q, [(prefix, lens[m], mine[m]) for m in rids], t=T2)
            seen = {}
            for n_splits in (1, 2, 3, 5, 16, 0):
                got, glse = _fold(torch, lib, [h], [0, n], layer, q[:, None], lens, [1] * n, out, lse, n_splits)
                _assert_decode(got, glse, ref, f"attend_prefix_fold {scheme} rows_per_pos {rpp} n_splits {n_splits} layer {layer}")
                seen[n_splits] = (got, glse)
                if n_splits > 1:
                    one = _fold(torch, lib, [h], [0, 1], layer, q[1:2, None], [480], [1], out[1:2], lse[1:2], n_splits)
                    assert np.array_equal(one[0][0], got[1]) and np.array_equal(one[1][0], glse[1]), (scheme, n_splits, "alone")
            assert np.array_equal(seen[0][0], seen[1][0])                   # the rule cuts nothing this short: 15 tiles < 2 x 32
            assert not np.array_equal(seen[5][0], seen[1][0])               # forced pieces did run the piece launch and the merge
            via = _shared(torch, conn, layer, rids, [P0] * n, q, lens, splits=5)
            assert np.array_equal(via, seen[5][0]), (scheme, rpp, layer, "attend_shared(splits=5)")


T3 = 2112


@pytest.mark.parametrize("scheme", ALL)
def test_the_rule_cuts_a_prefix_of_64_tiles_in_two(oracle, scheme):
    """T = 2112, a 2050-position prefix (2048 stored: 64 tiles), three members at rows_per_pos 4 -- one block of 8 heads on a whole
    chip, so the library's rule (n_splits 0) cuts the group in 2 pieces of 32 tiles: the rule's bits are the forced 2's and not the
    unsplit walk's, they meet float64, and attend_shared's default is the rule"""
    torch = torch_mod()
    _, _, owns, q = _inputs(4)
    if "long" not in _data:
        rng = np.random.default_rng(2050)
        _data["long"] = (_rows(rng, L, 2050, H, D), _rows(rng, L, 2050, H, D))
    prefix = _data["long"]
    lens, mine = [2048, 34, 2048], [owns[37], owns[0], owns[64]]
    q, rids = q[:3], [0, 1, 2]
    with _world(torch, scheme, {P0: prefix}, mine, t=T3) as (lib, conn):
        assert lib.chunk_split_plan([2048], [3], 4, 0) == ([2], [32])
        h = conn.requests[P0].handle
        out, lse = _own_step(torch, conn, LAYER, rids, q)
        rule, two, whole = (_fold(torch, lib, [h], [0, 3], LAYER, q[:, None], lens, [1] * 3, out, lse, n) for n in (0, 2, 1))
        assert np.array_equal(rule[0], two[0]) and np.array_equal(rule[1], two[1]), (scheme, "the rule is not the forced 2")
        assert not np.array_equal(rule[0], whole[0]), (scheme, "the rule did not cut")
        ref = _decode_ref(oracle, scheme, LAYER, q, [(prefix, lens[m], mine[m]) for m in rids], t=T3)
        _assert_decode(rule[0], rule[1], ref, f"attend_prefix_fold {scheme} the rule over 64 tiles")
        _assert_decode(whole[0], whole[1], ref, f"attend_prefix_fold {scheme} 64 tiles unsplit")
        via = _shared(torch, conn, LAYER, rids, [P0] * 3, q, lens)
        assert np.array_equal(via, rule[0]), (scheme, "attend_shared's default is not the rule")


# ----------------------------------------------------------------------------- 8b. a stream of the caller's, members not grouped
@pytest.mark.parametrize("scheme", ALL)
def test_interleaved_members_on_a_stream_that_is_not_current(scheme):
    """attend_shared and attend_chunk_shared with stream= a stream that is not torch's current one and members that are NOT grouped:
    the gather of q / k_new / v_new and the way back run on that stream, behind the work queued there and behind the fold -- the
    stream is kept busy in front of the call, and after a wait for THAT STREAM ALONE the result is, request by request, the grouped
    order's bits"""
    torch = torch_mod()
    prefix, second, owns, q = _inputs(4)
    n = 9
    q, rids = q[:n], list(range(n))
    mine = [owns[OWN[m % 5]] for m in rids]
    pids = [P0, P1, None, P0, P1, None, P0, P0, P1]
    lens = [98, 64, None, 254, 36, None, 2, 64, 2]
    rng = np.random.default_rng(41)
    S_, n_new = 5, [5, 2, 5, 0, 5, 1, 5, 3, 5]
    qc, new = _rows(rng, n, S_, H, 4, D), (_rows(rng, n, S_, L, H, D), _rows(rng, n, S_, L, H, D))
    with _world(torch, scheme, {P0: prefix, P1: second}, mine) as (lib, conn):
        order, _, _ = SpeckvKVConnector.shared_groups(rids, pids)
        assert order != rids
        pick = lambda xs: [xs[b] for b in order]
        want = _shared(torch, conn, LAYER, pick(rids), pick(pids), q[order], pick(lens))
        want_c = conn.attend_chunk_shared(LAYER, pick(rids), pick(pids), _dev(torch, qc[order]), _dev(torch, new[0][order]),
                                          _dev(torch, new[1][order]), SM, n_new=pick(n_new), prefix_lens=pick(lens))
        torch.cuda.synchronize()
        want_c = want_c.cpu().numpy().view(np.int32)
        st = torch.cuda.Stream()
        dq, dqc, dk, dv = _dev(torch, q), _dev(torch, qc), _dev(torch, new[0]), _dev(torch, new[1])
        x = torch.randn((2048, 2048), device="cuda", dtype=torch.float16)
        torch.cuda.synchronize()
        for _ in range(2):
            with torch.cuda.stream(st):                                       # the stream is busy when the call is issued
                for _ in range(40):
                    x = (x @ x).clamp_(-1, 1)
            got = conn.attend_shared(LAYER, rids, pids, dq, SM, prefix_lens=lens, stream=st)
            with torch.cuda.stream(st):
                for _ in range(40):
                    x = (x @ x).clamp_(-1, 1)
            got_c = conn.attend_chunk_shared(LAYER, rids, pids, dqc, dk, dv, SM, n_new=n_new, prefix_lens=lens, stream=st)
            st.synchronize()                                                  # that stream alone
            a, b = got.cpu().numpy().view(np.int32), got_c.cpu().numpy().view(np.int32)
            assert np.array_equal(a[order], want), (scheme, "attend_shared on a stream of the caller's")
            assert np.array_equal(b[order], want_c), (scheme, "attend_chunk_shared on a stream of the caller's")


# ----------------------------------------------------------------------------- 9. placement
@pytest.mark.parametrize("scheme", ALL)
def test_a_pool_striped_over_three_and_a_migrated_page_of_the_prefix(oracle, scheme):
    torch = torch_mod()
    prefix, _, owns, q = _inputs(4)
    n = 6
    q, rids = q[:n], list(range(n))
    lens = [254, 98, 36, 2, 64, 254]
    mine = [owns[OWN[m % 5]] for m in rids]
    ref = _decode_ref(oracle, scheme, LAYER, q, [(prefix, lens[m], mine[m]) for m in rids])
    with _world(torch, scheme, {P0: prefix}, mine, SPECKV_POOL_DEVICES="0,0,0") as (lib, conn):
        got = _shared(torch, conn, LAYER, rids, [P0] * n, q, lens)
        _assert_decode(got, None, ref, f"attend_shared {scheme} pool striped over 3")
    with _world(torch, scheme, {P0: prefix}, mine, SPECKV_POOL_DEVICES="0,0") as (lib, conn):
        got = _shared(torch, conn, LAYER, rids, [P0] * n, q, lens)
        h = conn.requests[P0].handle
        lib.migrate(h, LAYER * T + 15, 3, 1)                              # a tile's last and next first K pages, one V page
        lib.migrate(h, LAYER * T + T // 2 + 2, 1, 0)
        lib.migrate(h, LAYER * T + 40, 2, 0)
        moved = _shared(torch, conn, LAYER, rids, [P0] * n, q, lens)
        assert np.array_equal(moved, got), (scheme, "a migrated page of the prefix changed bits")


# ----------------------------------------------------------------------------- 10. refusals
def test_the_entry_refuses_bad_arguments_and_capture_and_launches_nothing():
    torch = torch_mod()
    prefix, second, owns, q = _inputs(4)
    n = 4
    q, lens = q[:n, None], [98, 36, 2, 64]
    out, lse = np.full((n, 1, H, 4, D), PATTERN, np.int32), np.full((n, 1, H, 4), PATTERN, np.int32)
    with _world(torch, "fp8", {P0: prefix, P1: second}, []) as (lib, conn):
        h0, h1 = conn.requests[P0].handle, conn.requests[P1].handle
        lib.set_compression_scheme(1)
        int8 = lib.alloc(2 * T * L * H * D * 2); lib.set_layout(int8, T, L, H, D, 2)
        lib.set_compression_scheme(3)
        int4 = lib.alloc(2 * T * L * H * D * 2); lib.set_layout(int4, T, L, H, D, 2)
        lib.set_compression_scheme(4)
        bare = lib.alloc(2 * T * L * H * D * 2)                           # no layout
        # the device buffers live OUTSIDE the refused call: after every refusal, and a wait for the stream and the device, out and lse
        # still hold the fill pattern -- a refusal behind the descriptor copy, a piece launch or the fold would show here
        dq, do, dl = _dev(torch, q), _dev(torch, out), _dev(torch, lse)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()

        def refused(status, what, handles=(h0, h1), first=(0, 2, 4), lens=lens, n_q=(1,) * n, **change):
            args = dict(prefix_handles=np.asarray(handles, np.uint64), first_member=np.asarray(first, np.uint32), layer=LAYER, d_q=dq.data_ptr(),
                        C=1, rows_per_pos=4, prefix_len=np.asarray(lens, np.uint32), n_q=np.asarray(n_q, np.uint32), n_splits=1, sm_scale=SM,
                        d_out=do.data_ptr(), d_lse=dl.data_ptr(), stream=st.cuda_stream)
            args.update(change)
            with pytest.raises(SpeckvError) as e:
                lib.attend_prefix_fold(**args)
                pytest.fail(what)
            assert e.value.status == status, (what, e.value.status)
            st.synchronize(); torch.cuda.synchronize()
            assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all()), (what, "a refused call wrote out / lse")

        invalid = {
            "NULL stream": dict(stream=0), "NULL q": dict(d_q=0), "NULL out": dict(d_out=0), "NULL lse": dict(d_lse=0),
            "a misaligned q": dict(d_q=dq.data_ptr() + 8), "a misaligned out": dict(d_out=do.data_ptr() + 8),
            "rows_per_pos 3": dict(rows_per_pos=3), "rows_per_pos 0": dict(rows_per_pos=0), "rows_per_pos 32": dict(rows_per_pos=32),
            "C 0": dict(C=0), "an odd prefix_len": dict(lens=[98, 35, 2, 64]), "a prefix_len beyond the layout": dict(lens=[98, 36, 2, T + 2]),
            "n_q > C": dict(n_q=[1, 2, 1, 1]), "first_member not from 0": dict(first=[1, 2, 4]), "first_member descending": dict(first=[0, 3, 2]),
            "a prefix without layout": dict(handles=(h0, bare)), "a scheme without a fused form": dict(handles=(int8, int8)),
            "mixed schemes": dict(handles=(h0, int4)), "a layer beyond the layout": dict(layer=L), "n_splits 65": dict(n_splits=65),
        }
        for what, change in invalid.items():
            refused(-4, what, **change)                                      # SPECKV_ERR_INVAL
        refused(-1, "an unknown handle", handles=(h0, 0xDEAD))               # SPECKV_ERR_GENERAL
        # a refusal that comes LATE in the engine's order (the second group's handle is judged behind everything else) with pieces
        # asked for: nothing of the piece launch, the merge or the fold has run
        refused(-4, "mixed schemes, forced pieces", handles=(h0, int4), n_splits=3)
        # more work items than a launch indexes: 2^14 members of 2^16 positions at rows_per_pos 16 are 2^28 blocks x 8 heads.  The
        # host arrays are judged before anything is read on the device
        big = 1 << 14
        refused(-4, "more work items than a launch indexes", handles=(h0,), first=(0, big), lens=np.full(big, 2, np.uint32),
                n_q=np.full(big, 1 << 16, np.uint32), C=1 << 16, rows_per_pos=16)
        # and the same buffers ARE written by the call that is not refused: the pattern is no accident of the buffers
        eager = dict(prefix_handles=np.asarray([h0, h1], np.uint64), first_member=np.asarray([0, 2, 4], np.uint32), layer=LAYER, d_q=dq.data_ptr(),
                     C=1, rows_per_pos=4, prefix_len=np.asarray(lens, np.uint32), n_q=np.ones(n, np.uint32), n_splits=1, sm_scale=SM)
        ok_out, ok_lse = torch.zeros_like(do), torch.full_like(dl, int(NEG_INF))
        torch.cuda.synchronize()
        lib.attend_prefix_fold(d_out=ok_out.data_ptr(), d_lse=ok_lse.data_ptr(), stream=st.cuda_stream, **eager)
        st.synchronize()
        assert not bool((ok_lse == int(NEG_INF)).any())
        # capture: refused, nothing launched
        s = torch.cuda.Stream()
        args = dict(prefix_handles=np.asarray([h0, h1], np.uint64), first_member=np.asarray([0, 2, 4], np.uint32), layer=LAYER, d_q=dq.data_ptr(),
                    C=1, rows_per_pos=4, prefix_len=np.asarray(lens, np.uint32), n_q=np.ones(n, np.uint32), n_splits=1, sm_scale=SM,
                    d_out=do.data_ptr(), d_lse=dl.data_ptr(), stream=s.cuda_stream)
        bump = torch.zeros(4, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with graph_capture(g, s):
            with pytest.raises(SpeckvError) as e:
                lib.attend_prefix_fold(**args)
            assert e.value.status == -4
            bump.add_(1)
        g.replay(); torch.cuda.synchronize()
        assert bool((do == PATTERN).all()) and bool((dl == PATTERN).all())
        for h in (int8, int4, bare):
            lib.free(h)


# ----------------------------------------------------------------------------- 11. through the connector, end to end
def _chunk_ref(oracle, scheme, layer, q, new, n_new, members):
    """float64 of the chunk route: q [M][S][H][R][D], new (k, v) [M][S][L][H][D]; everything from the fp16 query; causal among the new
    rows.  -> want [M][S][H][R][D], mag"""
    M, S_, _, R, _ = q.shape
    want, mag = np.zeros((M, S_, H, R, D)), np.zeros((M, S_, H, R, D))
    for head in range(H):
        for m, (prefix, plen, own) in enumerate(members):
            n, even = own[0].shape[1], own[0].shape[1] & ~1
            Kp, Vp = _checker(oracle, scheme, prefix, layer).kv(head)
            keys, vals = [Kp[:plen]], [Vp[:plen]]
            if even:
                Ko, Vo = _checker(oracle, scheme, own, layer).kv(head)
                keys.append(Ko[:even]); vals.append(Vo[:even])
            if n & 1:
                keys.append(own[0][layer, n - 1, head].astype(np.float64)[None]); vals.append(own[1][layer, n - 1, head].astype(np.float64)[None])
            held = sum(len(x) for x in keys)
            Ka = np.concatenate(keys + [new[0][m, :, layer, head].astype(np.float64)])
            Va = np.concatenate(vals + [new[1][m, :, layer, head].astype(np.float64)])
            for j in range(n_new[m]):
                want[m, j, head], _, mag[m, j, head] = _softmax([q[m, j, head].astype(np.float64) @ Ka[:held + j + 1].T], [Va[:held + j + 1]])
    return want, mag


@pytest.mark.parametrize("pre_scale", [False, True], ids=["plain", "k-pre-scale"])
@pytest.mark.parametrize("scheme", ALL)
def test_connector_end_to_end(oracle, scheme, pre_scale):
    """a 64-position prefix; three members whose suffixes of 5, 33 and 0 positions go through attend_chunk_shared + commit; then six
    attend_shared + append steps, each against float64 -- with the K pre-scale the reference runs over what the kernels are given
    (k / scale, q x scale).  Forked twins (fork + the same suffix + attend) are judged at every step within the same bound: over an
    INT4 pool, where both routes take the fp16 query, against the SAME reference; over FP8 and MXFP4 pools, where attend() quantises
    the query for every stored position and the prefix is one of the twin's own, against the three-part reference applied to the twin
    as it is composed (every position an own stored one: delta then covers the prefix too).  Lengths and tails are those of the same steps without a prefix (the
    moves of _epoch: the next test); a prefix freed right after a call on the call's stream does not disturb it"""
    from tests.test_gpu_chunk import _f16_times, _kscale
    torch = torch_mod()
    rng = np.random.default_rng(88)
    ks = _kscale() if pre_scale else np.ones((L, H, D), np.float32)
    inv = 1.0 / ks
    scaled = lambda k: _f16_times(k, inv[:, None])                         # [L][n][H][D] as the pool and the tails hold K
    prefix = (_rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D))
    S_, n_new, R, M = 33, [5, 33, 0], 4, 3
    new = (_rows(rng, M, S_, L, H, D), _rows(rng, M, S_, L, H, D))
    qc = _rows(rng, L, M, S_, H, R, D)
    rids, twins = [0, 1, 2], [10, 11, 12]
    empty = (np.zeros((L, 0, H, D), np.float16),) * 2
    pre_prefix = (scaled(prefix[0]), prefix[1])
    with _world(torch, scheme, {P0: prefix}, [empty] * M, kscale=ks if pre_scale else None) as (lib, conn):
        plain = SpeckvKVConnector(lib, L, H, D, T, scheme)                 # the same steps without a prefix
        if pre_scale:
            plain.set_k_channel_scale(torch.from_numpy(ks).cuda())
        for r in rids:
            plain.add_request(1000 + r)
        keep = [conn.fork([P0] * M, twins)]
        dk, dv = _dev(torch, new[0]), _dev(torch, new[1])
        for layer in range(L):
            got = conn.attend_chunk_shared(layer, rids, [P0] * M, _dev(torch, qc[layer]), dk, dv, SM, n_new=n_new)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            qs = _f16_times(qc[layer], ks[layer][None, None, :, None, :])
            new_pre = (_f16_times(new[0], inv[None, None]), new[1])
            want, mag = _chunk_ref(oracle, scheme, layer, qs, new_pre, n_new, [(pre_prefix, 64, empty)] * M)
            for m, n in enumerate(n_new):
                err, tol = np.abs(got[m, :n] - want[m, :n]), 2e-3 * mag[m, :n] + 1e-6
                assert np.all(err <= tol), (scheme, layer, m, float((err / tol).max(initial=0.0)))
                assert not got[m, n:].any()
            print(f"attend_chunk_shared {scheme} layer {layer}: worst err / tol "
                  f"{max(float((np.abs(got[m, :n] - want[m, :n]) / (2e-3 * mag[m, :n] + 1e-6)).max(initial=0.0)) for m, n in enumerate(n_new)):.3f}")
        paths = [range(n) for n in n_new]
        keep.append(conn.commit(rids, dk, dv, paths))
        keep.append(conn.commit(twins, dk, dv, paths))
        keep.append(plain.commit([1000 + r for r in rids], dk, dv, paths))
        own = [(np.ascontiguousarray(new[0][m, :n].transpose(1, 0, 2, 3)), np.ascontiguousarray(new[1][m, :n].transpose(1, 0, 2, 3))) for m, n in enumerate(n_new)]
        worst = twin_worst = 0.0
        for step in range(6):
            q = _rows(rng, L, M, H, R, D)
            kn, vn = _rows(rng, M, L, H, D), _rows(rng, M, L, H, D)
            for layer in range(L) if step == 0 else [LAYER]:               # (both layers once; the references cost host time)
                qs = _f16_times(q[layer], ks[layer][None, :, None, :])
                mine = [(scaled(k), v) for k, v in own]
                got = _shared(torch, conn, layer, rids, [P0] * M, q[layer])
                ref = _decode_ref(oracle, scheme, layer, qs, [(pre_prefix, 64, mine[m]) for m in range(M)])
                worst = max(worst, _assert_decode(got, None, ref, f"attend_shared {scheme} step {step} layer {layer}"))
                twin = conn.attend(layer, twins, _dev(torch, q[layer]), SM)
                torch.cuda.synchronize()
                twin = twin.cpu().numpy().view(np.int32)
                if scheme == "int4":                                       # the fp16 query on both routes: the twins meet the SAME reference
                    _assert_decode(twin, None, ref, f"fork + attend {scheme} against the shared reference, step {step} layer {layer}")
                whole = [(np.concatenate([pre_prefix[0], k], axis=1), np.concatenate([pre_prefix[1], v], axis=1)) for k, v in mine]
                ref = _decode_ref(oracle, scheme, layer, qs, [(None, 0, whole[m]) for m in range(M)])
                twin_worst = max(twin_worst, _assert_decode(twin, None, ref, f"fork + attend {scheme} step {step} layer {layer}"))
            dkn, dvn = _dev(torch, kn), _dev(torch, vn)
            keep += [conn.append(rids, dkn, dvn), conn.append(twins, dkn, dvn), plain.append([1000 + r for r in rids], dkn, dvn)]
            own = [(np.concatenate([k, kn[m][:, None]], axis=1), np.concatenate([v, vn[m][:, None]], axis=1)) for m, (k, v) in enumerate(own)]
        torch.cuda.synchronize()
        print(f"attend_shared {scheme} end to end: worst err / tol {worst:.3f}; forked twins {twin_worst:.3f}")
        # state: what the same steps leave without a prefix (the fork's three add_request calls aside)
        for r in rids:
            a, b = conn.requests[r], plain.requests[1000 + r]
            assert a.length == b.length == n_new[r] + 6 and conn.length(10 + r) == 64 + a.length
            assert (a.tail_k is None) == (b.tail_k is None)
            if a.tail_k is not None:
                assert torch.equal(a.tail_k, b.tail_k) and torch.equal(a.tail_v, b.tail_v)
        assert conn.length(P0) == 64
        # freeing the prefix right behind a call on the call's stream is safe: speckv_free waits for the stream (note_use)
        q = _rows(rng, M, H, R, D)
        want = _shared(torch, conn, LAYER, rids, [P0] * M, q)
        st = torch.cuda.Stream()
        got = conn.attend_shared(LAYER, rids, [P0] * M, _dev(torch, q), SM, stream=st)
        conn.free_request(P0)
        st.synchronize(); torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.int32), want), (scheme, "freeing the prefix disturbed the call in flight")
        del keep


@pytest.mark.parametrize("scheme", ALL)
def test_the_epoch_moves_as_without_a_prefix(scheme):
    """attend_shared and attend_chunk_shared change no state; commit and append move _epoch by what they move it without a prefix"""
    torch = torch_mod()
    rng = np.random.default_rng(89)
    prefix = (_rows(rng, L, 64, H, D), _rows(rng, L, 64, H, D))
    empty = (np.zeros((L, 0, H, D), np.float16),) * 2
    new, q = (_rows(rng, 2, 5, L, H, D), _rows(rng, 2, 5, L, H, D)), _rows(rng, 2, 5, H, 4, D)
    with _world(torch, scheme, {P0: prefix}, [empty] * 2) as (lib, conn):
        plain = SpeckvKVConnector(lib, L, H, D, T, scheme)
        for r in (0, 1):
            plain.add_request(1000 + r)
        dk, dv = _dev(torch, new[0]), _dev(torch, new[1])
        keep, moves = [], []
        for c, ids, shared in ((conn, [0, 1], True), (plain, [1000, 1001], False)):
            e0 = c._epoch
            if shared:
                c.attend_chunk_shared(LAYER, ids, [P0, P0], _dev(torch, q), dk, dv, SM, n_new=[5, 2])
            else:
                c.attend_chunk(LAYER, ids, _dev(torch, q), dk, dv, SM, n_new=[5, 2])
            e1 = c._epoch
            keep.append(c.commit(ids, dk, dv, [range(5), range(2)]))
            e2 = c._epoch
            if shared:
                c.attend_shared(LAYER, ids, [P0, None], _dev(torch, q[:, 0]), SM)
            else:
                c.attend(LAYER, ids, _dev(torch, q[:, 0]), SM)
            e3 = c._epoch
            keep.append(c.append(ids, _dev(torch, new[0][:, 0]), _dev(torch, new[1][:, 0])))
            moves.append((e1 - e0, e2 - e1, e3 - e2, c._epoch - e3, [c.length(i) for i in ids]))
        torch.cuda.synchronize()
        assert moves[0] == moves[1] and moves[0][0] == 0 and moves[0][2] == 0, moves
        del keep


# ----------------------------------------------------------------------------- 12. the example
def test_the_shared_prefix_example_runs():
    """examples/shared_prefix_example.py in this process, short: one prompt, samples as empty members, decode steps with attend_shared
    + append, compared against forked twins"""
    import importlib.util
    import os
    torch_mod()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "shared_prefix_example.py")
    spec = importlib.util.spec_from_file_location("shared_prefix_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run("int4", prompt=98, samples=5, steps=4, verbose=False) == 5 * 4
