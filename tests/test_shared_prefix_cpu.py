"""Not -m gpu: shared-prefix attention (speckv_ext_attend_prefix_fold, SpeckvLib.attend_prefix_fold, SpeckvKVConnector.shared_groups /
attend_shared / attend_chunk_shared) as far as it can be judged without a device.

The binding puts every argument where include/speckv_ext.h declares it (the method of tests/test_chunk_entries_cpu.py: a recording
`_ext`; names, order and pointer-ness come from the header); the entry exists on the device-less engine and answers as every data
call does; shared_groups against a brute force; the connector's refusals against a library that must not be called; and a float64
emulation of k_attend_prefix's walk -- tiles of 32, the per-row limit, the group's maximum, pieces, the ascending merge, the fold --
against a plain float64 softmax over prefix + own positions, with what each mutation of a rule would compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
ENTRY = "speckv_ext_attend_prefix_fold"
# host arrays of the entry: (C type, numpy type, entries for 2 groups of 3 members)
ARRAYS = {"prefix_handles": (C.c_uint64, np.uint64, [901, 902]), "first_member": (C.c_uint32, np.uint32, [0, 2, 3]),
          "prefix_len": (C.c_uint32, np.uint32, [10, 20, 30]), "n_q": (C.c_uint32, np.uint32, [1, 2, 3])}


def declared(entry=ENTRY):
    """[(name, is a pointer)] of the entry's parameters, in the header's order"""
    text = re.search(entry + r"\s*\((.*?)\);", HEADER[HEADER.index("speckv_status_t " + entry + "("):], re.S).group(1)
    return [(p.split()[-1].lstrip("*"), "*" in p) for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]


def _call(values):
    lib, got = speckv_ctypes.SpeckvLib.__new__(speckv_ctypes.SpeckvLib), []
    lib._ext = lambda name, *args: got.append((name, args))
    lib.attend_prefix_fold(*[values[name] for name, _ in declared() if name != "n_groups"])
    assert len(got) == 1 and got[0][0] == ENTRY
    assert len(got[0][1]) == len(declared()) == len(speckv_ctypes._EXT_SIGNATURES[ENTRY])
    return dict(zip([name for name, _ in declared()], got[0][1]))


def _sentinels():
    values = {name: 0.375 if name == "sm_scale" else 1000 + k for k, (name, _) in enumerate(declared())}
    values.update({name: list(v[2]) for name, v in ARRAYS.items()})
    return values


def test_the_entry_is_declared_as_proposed_and_keeps_the_abi_version():
    names = [name for name, _ in declared()]
    assert names == ["n_groups", "prefix_handles", "first_member", "layer", "d_q_f16", "C", "rows_per_pos", "prefix_len", "n_q", "n_splits",
                     "sm_scale", "d_out", "d_lse", "stream"]
    assert [p for _, p in declared()] == [n in ARRAYS or n in ("d_q_f16", "d_out", "d_lse", "stream") for n in names]
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in HEADER                  # an additive entry: the version stays
    doc = HEADER[HEADER.index(ENTRY + ":"):]
    assert "NOT capturable" in doc and "READ AND WRITTEN" in doc and "lse = -inf" in doc
    sig = speckv_ctypes._EXT_SIGNATURES[ENTRY]
    for (name, pointer), t in zip(declared(), sig):
        assert (t is C.c_void_p) == pointer and (t is C.c_float) == (name == "sm_scale"), name


def test_every_argument_arrives_in_the_headers_position():
    values = _sentinels()
    got = _call(values)
    assert got["n_groups"] == 2
    for name, pointer in declared():
        if name in ARRAYS:                                               # sequences are copied into C arrays of the declared type
            assert isinstance(got[name], C.Array) and got[name]._type_ is ARRAYS[name][0] and list(got[name]) == values[name], name
        elif pointer:
            assert isinstance(got[name], C.c_void_p) and got[name].value == values[name], name
        elif name != "n_groups":
            assert got[name] == values[name], name


def test_numpy_arrays_arrive_by_their_own_data_pointer_and_a_zero_lse_as_null():
    values = _sentinels()
    arrays = {name: np.asarray(v[2], dtype=v[1]) for name, v in ARRAYS.items()}
    values.update(arrays)
    values["d_lse"] = 0
    got = _call(values)
    for name, a in arrays.items():
        assert isinstance(got[name], C.c_void_p) and got[name].value == a.ctypes.data, name
    assert got["d_lse"].value is None and got["n_groups"] == 2


def test_the_entry_on_the_null_engine_answers_with_the_no_data_path_status():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call; nothing is counted"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    raw = C.CDLL(pkg.build_library())
    assert hasattr(raw, ENTRY)
    raw.speckv_ext_abi_version.restype = C.c_uint32
    assert raw.speckv_ext_abi_version() == 6
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        before = bytes(lib.stats())
        for n_splits in (0, 1, 5, 64):
            with pytest.raises(SpeckvError) as err:
                lib.attend_prefix_fold(np.asarray([a], np.uint64), np.asarray([0, 1], np.uint32), 0, at, 1, 1, np.asarray([2], np.uint32),
                                       np.asarray([1], np.uint32), n_splits, 1.0, at, at, 1)
            assert err.value.status == -2                                 # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- shared_groups
def _brute_groups(prefix_ids):
    """from the statement alone: the prefixes by first member, a prefix's members in the caller's order, None last"""
    seen = []
    for p in prefix_ids:
        if p is not None and p not in seen:
            seen.append(p)
    order, first = [], [0]
    for p in seen:
        order += [b for b, x in enumerate(prefix_ids) if x == p]
        first.append(len(order))
    return order + [b for b, x in enumerate(prefix_ids) if x is None], seen, first


def test_shared_groups_against_a_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(0, 12))
        ids = [None if rng.random() < 0.25 else int(rng.integers(100, 104)) for _ in range(n)]
        req = list(range(n))
        order, prefixes, first = SpeckvKVConnector.shared_groups(req, ids)
        assert (order, prefixes, first) == _brute_groups(ids), ids
        assert sorted(order) == req and len(first) == len(prefixes) + 1 and first[0] == 0
        for g, p in enumerate(prefixes):                                 # a group's members name its prefix, in ascending (stable) order
            members = order[first[g]:first[g + 1]]
            assert members == sorted(members) and members and all(ids[b] == p for b in members)
        assert all(ids[b] is None for b in order[first[-1]:]) and order[first[-1]:] == sorted(order[first[-1]:])
        # laid out already: sorting by the order once more changes nothing
        again, p2, f2 = SpeckvKVConnector.shared_groups(req, [ids[b] for b in order])
        assert again == req and p2 == prefixes and f2 == first
    assert SpeckvKVConnector.shared_groups([], []) == ([], [], [0])
    assert SpeckvKVConnector.shared_groups([1, 2], [None, None]) == ([0, 1], [], [0])
    assert SpeckvKVConnector.shared_groups([1, 2, 3, 4], [7, 7, 8, None]) == ([0, 1, 2, 3], [7, 8], [0, 2, 3])
    assert SpeckvKVConnector.shared_groups([1, 2, 3, 4], [8, None, 7, 8]) == ([0, 3, 2, 1], [8, 7], [0, 2, 3])
    with pytest.raises(ValueError):
        SpeckvKVConnector.shared_groups([1, 2], [7])


class _NoLib:
    """a library that must not be called: the connector refuses in front of it"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


class _Q:
    shape = (2, 8, 4, 128)


def _connector(scheme="fp8", lengths=((1, 0), (2, 5), (50, 64), (51, 37))):
    conn = SpeckvKVConnector.__new__(SpeckvKVConnector)
    SpeckvKVConnector.__init__(conn, _NoLib(), num_layers=2, max_tokens=256, scheme=scheme)
    from cxl_speckv_amd.kv_connector import _Request
    for rid, n in lengths:
        conn.requests[rid] = _Request(1000 + rid)
        conn.requests[rid].length = n
    return conn


@pytest.mark.parametrize("method", ["attend_shared", "attend_chunk_shared"])
def test_the_connector_refuses_in_front_of_any_library_call(method):
    def call(conn, req_ids, prefix_ids, **kw):
        if method == "attend_shared":
            return conn.attend_shared(0, req_ids, prefix_ids, _Q(), 0.1, **kw)
        return conn.attend_chunk_shared(0, req_ids, prefix_ids, _Q(), None, None, 0.1, **kw)
    conn = _connector()
    with pytest.raises(KeyError):
        call(conn, [1, 2], [50, 99])                                      # an unknown prefix
    with pytest.raises(KeyError):
        call(conn, [1, 98], [50, 50])                                     # an unknown member
    with pytest.raises(ValueError, match="member of the call"):
        call(conn, [1, 2], [50, 2])
    with pytest.raises(ValueError, match="member of the call"):
        call(conn, [1, 50], [50, None])
    with pytest.raises(ValueError):
        call(conn, [1, 2], [50])                                          # wrong lengths of the lists
    with pytest.raises(ValueError):
        call(conn, [1, 2], [50, 50], prefix_lens=[64])
    for bad in (True, 2.0, "50", [50]):
        with pytest.raises((ValueError, TypeError)):
            call(conn, [1, 2], [50, bad])
    for bad in (True, 2.5, "2", -2, 3, 66):                               # bools, non-integers, negative, odd, beyond the prefix
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], prefix_lens=[2, bad])
    with pytest.raises(ValueError, match="prefix_lens and keep"):         # an odd prefix needs prefix_lens
        call(conn, [1, 2], [51, 51])
    with pytest.raises(ValueError):
        call(conn, [1, 2], [51, 51], prefix_lens=[36, 38])                # at most length & ~1 = 36
    with pytest.raises(ValueError):
        call(conn, [1, 2], [None, 50], prefix_lens=[2, 2])                # a member without a prefix has no length
    for bad in (-1, 65, True, 1.5):
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], splits=bad)
    with pytest.raises(ValueError, match="FP8, INT4 or MXFP4"):
        call(_connector("int8"), [1, 2], [50, 50])
    with pytest.raises(TypeError):
        call(conn, [1, 2], [50, 50], window=4)                            # there is no window argument


# ----------------------------------------------------------------------------- the float64 emulation
def _ceil(a, b):
    return -(-a // b)


def _emulate(lens, n_q, C_, rpp, q, K, V, own_out, own_lse, pieces=1, mutation=None):
    """k_attend_prefix (+ k_prefix_combine) for ONE group and ONE head in float64.  Member m sees [0, lens[m]) of the prefix K / V
    [max][d]; q [members][C][rpp][d]; own_out / own_lse what the member attended on its own.  The blocks of 64 // rpp flat pairs, the
    tiles up to the GROUP's maximum staged with zeros beyond it, the per-row limit, the skipping of tiles by a wave none of whose rows
    sees them, the running maximum with the m_use path, pieces by chunk_split_plan's rule (tpp = ceil(tiles / pieces)) merged in
    ascending order, the fold.  Dead pairs keep what out / lse held.  mutation: one rule broken."""
    per, members, d = 64 // rpp, len(lens), K.shape[1]
    live_max = max([n for n, k in zip(lens, n_q) if k] + [0])
    out, lse = own_out.copy(), own_lse.copy()
    if live_max == 0:
        return out, lse
    n_pool = _ceil(live_max, 32)
    tpp = _ceil(n_pool, max(1, min(pieces, n_pool)))
    n_pieces = _ceil(n_pool, tpp)
    for p_first in range(0, members * C_, per):
        rows = []                                                        # (member, position, limit) of the block's live pairs
        for p in range(p_first, min(p_first + per, members * C_)):
            m, j = divmod(p, C_)
            if j < n_q[m] and lens[m]:
                limit = lens[m] - (mutation == "limit one lower") + (mutation == "limit one higher")
                rows.append((p - p_first, m, j, live_max if mutation == "the group's maximum for every row" else limit))
        if not rows:
            continue
        for jj, m, j, limit in rows:
            wave_rows = [r for r in rows if (r[0] * rpp) // 16 == (jj * rpp) // 16]
            for r in range(rpp):
                parts = []
                for piece in range(n_pieces):
                    acc, m_run, l_run = np.zeros(d), -np.inf, 0.0
                    for tile in range(piece * tpp, min((piece + 1) * tpp, n_pool)):
                        t = np.arange(32 * tile, 32 * tile + 32)
                        if not any(w[3] > t[0] for w in wave_rows):       # no row of the wave sees the tile
                            continue
                        Kt, Vt = np.zeros((32, d)), np.zeros((32, d))     # staging: zeros at and beyond the group's maximum
                        n = max(0, min(32, live_max - t[0]))
                        Kt[:n], Vt[:n] = K[t[0]:t[0] + n], V[t[0]:t[0] + n]
                        s = np.where(t < limit, Kt @ q[m, j, r], -np.inf)
                        m_new = max(m_run, s.max())
                        m_use = 0.0 if m_new == -np.inf else m_new
                        alpha = np.exp(m_run - m_use)
                        p = np.exp(s - m_use)
                        l_run, m_run, acc = l_run * alpha + p.sum(), m_new, acc * alpha + p @ Vt
                    parts.append((acc, m_run, l_run))
                if mutation == "a piece that saw nothing weighs 1":       # it reports m = 0 (its m_use) for m = -inf: 2^(0 - 0) = 1
                    parts = [(acc, 0.0 if m_p == -np.inf else m_p, l_p) for acc, m_p, l_p in parts]
                M = max(p[1] for p in parts)
                num, den = np.zeros(d), 0.0
                for acc, m_p, l_p in parts:                               # ascending piece order
                    w = np.exp(m_p - M)
                    num, den = num + acc * w, den + l_p * w
                own = own_lse[m, j, r]
                with np.errstate(invalid="ignore", divide="ignore"):
                    lse_p = M + np.log(den)
                    if mutation == "own lse of -inf not handled":         # logaddexp written as own + log1p(exp(lse_p - own))
                        new = own + np.log1p(np.exp(lse_p - own))
                    else:
                        mx = max(own, lse_p)
                        new = mx + np.log(np.exp(own - mx) + np.exp(lse_p - mx))
                    w_own, w_pre = np.exp(own - new), np.exp(lse_p - new)
                    if mutation == "the fold's weights swapped":
                        w_own, w_pre = w_pre, w_own
                    out[m, j, r] = own_out[m, j, r] * w_own + (num / den) * w_pre
                lse[m, j, r] = new
    return out, lse


def _case(lens, n_q, C_, rpp, own_lens, seed=0, hostile=True, low=False):
    """a group: random prefix rows (V of +-1000 with `hostile`), members' own rows; (q, K, V, own_out, own_lse, the plain float64
    softmax over prefix[:lens[m]] + own rows, its lse, and the same softmax over |V|).  low: every prefix score is far below 0
    (around -2000: e^score is 0 in float64), as scores are after a large sm_scale"""
    rng = np.random.default_rng(1000 * seed + sum(lens) + rpp + C_)
    members, d, top = len(lens), 8, max(lens + [2])
    q = rng.standard_normal((members, C_, rpp, d))
    K, V = rng.standard_normal((top, d)), rng.standard_normal((top, d))
    if low:
        q, K = -400.0 * np.abs(q), np.abs(K)
    if hostile:
        V *= 1000.0 * rng.choice([-1.0, 1.0], size=(top, 1))
    own_out, own_lse = np.zeros((members, C_, rpp, d)), np.full((members, C_, rpp), -np.inf)
    want, wlse, mag = np.zeros_like(own_out), np.zeros_like(own_lse), np.zeros_like(own_out)
    for m in range(members):
        Ko, Vo = rng.standard_normal((own_lens[m], d)), rng.standard_normal((own_lens[m], d))
        for j in range(C_):
            for r in range(rpp):
                if own_lens[m]:
                    s = Ko @ q[m, j, r]
                    p = np.exp(s - s.max())
                    own_out[m, j, r], own_lse[m, j, r] = p @ Vo / p.sum(), s.max() + np.log(p.sum())
                Kc, Vc = np.concatenate([K[:lens[m]], Ko]), np.concatenate([V[:lens[m]], Vo])
                if j < n_q[m] and len(Kc):
                    s = Kc @ q[m, j, r]
                    p = np.exp(s - s.max())
                    want[m, j, r], wlse[m, j, r], mag[m, j, r] = p @ Vc / p.sum(), s.max() + np.log(p.sum()), p @ np.abs(Vc) / p.sum()
    return q, K, V, own_out, own_lse, want, wlse, mag


# (prefix lengths of the members, n_q, C, rows_per_pos, own lengths): 2, 36, 64 and 98 mixed inside one block, members with nothing of
# their own (own lse = -inf), a group that crosses a block, a dead member inside a live group, a chunk with dead pairs
EMULATED = [([2, 36, 64, 98], [1] * 4, 1, 4, [0, 3, 0, 5]), ([98, 2, 64, 36, 98], [1] * 5, 1, 16, [0, 0, 7, 1, 2]),
            ([36, 98, 0, 64, 2], [1] * 5, 1, 1, [4, 0, 3, 0, 0]), ([2, 98, 36], [3, 1, 2], 3, 4, [0, 2, 0]),
            ([480, 34, 98], [1] * 3, 1, 4, [0, 0, 6]), ([2 + 2 * (m % 49) for m in range(17)], [1] * 17, 1, 4, [m % 3 for m in range(17)])]
PIECES = [1, 2, 3, 5, 16]


def _compare(case, got, lse, want, wlse):
    lens, n_q, C_, rpp, own = case
    ok = True
    for m in range(len(lens)):
        for j in range(C_):
            if j < n_q[m] and lens[m]:
                ok = ok and np.allclose(got[m, j], want[m, j], rtol=1e-9, atol=1e-9) and np.allclose(lse[m, j], wlse[m, j], rtol=1e-9, atol=1e-9)
    return ok


def test_the_emulated_kernel_is_the_softmax_over_prefix_and_own_positions():
    for case in EMULATED:
        q, K, V, own_out, own_lse, want, wlse, _ = _case(*case)
        for pieces in PIECES:
            got, lse = _emulate(case[0], case[1], case[2], case[3], q, K, V, own_out, own_lse, pieces)
            assert np.all(np.isfinite(got)), (case, pieces)
            assert _compare(case, got, lse, want, wlse), (case, pieces)
            for m, n in enumerate(case[0]):                              # dead pairs keep what they held, bit for bit
                for j in range(case[2]):
                    if j >= case[1][m] or n == 0:
                        assert np.array_equal(got[m, j], own_out[m, j]) and np.array_equal(lse[m, j], own_lse[m, j])


def test_a_member_without_positions_of_its_own_leaves_as_exactly_the_prefix_attention():
    """out = 0, lse = -inf in: the weights are exp(0) = 1 and exp(-inf) = 0, so the prefix part comes out to the bit"""
    lens, n_q = [2, 36, 98], [1, 1, 1]
    q, K, V, own_out, own_lse, want, wlse, _ = _case(lens, n_q, 1, 4, [0, 0, 0], hostile=False)
    got, lse = _emulate(lens, n_q, 1, 4, q, K, V, own_out, own_lse)
    for m, n in enumerate(lens):
        for r in range(4):
            s = np.concatenate([K[t:t + 32] @ q[m, 0, r] for t in range(0, n, 32)])[:n]
            assert abs(lse[m, 0, r] - (s.max() + np.log(np.exp(s - s.max()).sum()))) < 1e-12
    assert _compare((lens, n_q, 1, 4, None), got, lse, want, wlse)


@pytest.mark.parametrize("mutation", ["limit one lower", "limit one higher", "the group's maximum for every row", "the fold's weights swapped",
                                      "a piece that saw nothing weighs 1", "own lse of -inf not handled"])
def test_every_mutation_of_the_rule_leaves_the_float64_bound(mutation):
    """each broken rule moves some row of the emulated cases far outside |err| <= 2e-3 sum p|v| + 1e-6 (or makes it NaN): the float64
    tests of tests/test_gpu_shared_prefix.py run these shapes on the device and would fail"""
    broken = 0
    for case in EMULATED:
        # (the piece mutation shows where every real piece's maximum is far below the 0 the empty piece reports: their weights
        # underflow and the row's sum is 0)
        q, K, V, own_out, own_lse, want, _, mag = _case(*case, low="piece" in mutation)
        for pieces in PIECES if "piece" in mutation else [1]:
            got, _ = _emulate(case[0], case[1], case[2], case[3], q, K, V, own_out, own_lse, pieces, mutation=mutation)
            with np.errstate(invalid="ignore"):
                broken += not np.all(np.abs(got - want) <= 2e-3 * mag + 1e-6)
    assert broken > 0, mutation
