"""Not -m gpu: shared-prefix attention over the split pool (speckv_ext_attend_prefix_fold_kv, SpeckvLib.attend_prefix_fold_kv,
SpeckvSplitKVConnector.attend_shared / attend_chunk_shared) as far as it can be judged without a device.

The declaration and the binding (the method of tests/test_shared_prefix_cpu.py: names, order and pointer-ness come from the header,
a recording `_ext`); the entry on the device-less engine; the connector's refusals against a library that must not be called; and a
float64 emulation of the (FP8, MXFP4) instances of k_attend_prefix over the oracle's records of the contents the GPU tests use
(tests/test_gpu_k8v4_shared_prefix.py) -- E4M3 key values with the page's block scale on the score, MXFP4 values as fp16, tiles of
32, the per-row limit and lower bound, pieces and the ascending merge, fp16(p), the fold -- against a plain float64 softmax over
prefix + own positions, with what each of three broken rules would compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector, _SplitRequest
from tests._gpu import D, H, N
from tests.test_gpu_k8v4_shared_prefix import OWN, PLENS, T2, WIN_LENS, WIN_SEEN, W, _inputs, _pair
from tests.test_gpu_shared_prefix import L, LAYER, SM, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
ENTRY = "speckv_ext_attend_prefix_fold_kv"
WINDOW_ENTRY = "speckv_ext_attend_prefix_fold_window"
# host arrays of the entry: (C type, numpy type, entries for 2 groups of 3 members)
ARRAYS = {"k_handles": (C.c_uint64, np.uint64, [901, 902]), "v_handles": (C.c_uint64, np.uint64, [911, 912]),
          "first_member": (C.c_uint32, np.uint32, [0, 2, 3]), "prefix_len": (C.c_uint32, np.uint32, [10, 20, 30]),
          "n_q": (C.c_uint32, np.uint32, [1, 2, 3]), "own_seen": (C.c_uint32, np.uint32, [4, 5, 6])}


def declared(entry=ENTRY):
    """[(name, is a pointer)] of the entry's parameters, in the header's order"""
    text = re.search(entry + r"\s*\((.*?)\);", HEADER[HEADER.index("speckv_status_t " + entry + "("):], re.S).group(1)
    return [(p.split()[-1].lstrip("*"), "*" in p) for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]


def _call(values):
    lib, got = speckv_ctypes.SpeckvLib.__new__(speckv_ctypes.SpeckvLib), []
    lib._ext = lambda name, *args: got.append((name, args))
    lib.attend_prefix_fold_kv(*[values[name] for name, _ in declared() if name != "n_groups"])
    assert len(got) == 1 and got[0][0] == ENTRY
    assert len(got[0][1]) == len(declared()) == len(speckv_ctypes._EXT_SIGNATURES[ENTRY])
    return dict(zip([name for name, _ in declared()], got[0][1]))


def _sentinels():
    values = {name: 0.375 if name == "sm_scale" else 1000 + k for k, (name, _) in enumerate(declared())}
    values.update({name: list(v[2]) for name, v in ARRAYS.items()})
    return values


def test_the_entry_is_declared_as_proposed_and_keeps_the_abi_version():
    names = [name for name, _ in declared()]
    assert names == ["n_groups", "k_handles", "v_handles", "first_member", "layer", "d_q_f16", "C", "rows_per_pos", "prefix_len", "n_q", "own_seen",
                     "d_depth", "window", "n_splits", "sm_scale", "d_out", "d_lse", "stream"]
    # k_handles, v_handles in the place of prefix_handles, then the window entry's list from first_member on
    assert declared()[3:] == declared(WINDOW_ENTRY)[2:] and declared(WINDOW_ENTRY)[1][0] == "prefix_handles"
    assert [p for _, p in declared()] == [n in ARRAYS or n in ("d_q_f16", "d_depth", "d_out", "d_lse", "stream") for n in names]
    assert "#define SPECKV_EXT_ABI_VERSION 6u" in HEADER                  # an additive entry: the version stays
    doc = HEADER[HEADER.index("/* " + ENTRY + ":"):]
    doc = doc[:doc.index("*/")]
    for said in ("E4M3 value", "block scale multiplies the score in fp32", "speckv_ext_fetch_range", "region `layer`", "NOT capturable",
                 "READ AND WRITTEN", "lse = -inf", "before any launch"):
        assert said in doc, said
    sig = speckv_ctypes._EXT_SIGNATURES[ENTRY]
    for (name, pointer), t in zip(declared(), sig):
        assert (t is C.c_void_p) == pointer and (t is C.c_float) == (name == "sm_scale"), name
    assert ENTRY in open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "c_api.cpp")).read()


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


def test_numpy_arrays_arrive_by_their_own_data_pointer_and_absent_ones_as_null():
    values = _sentinels()
    arrays = {name: np.asarray(v[2], dtype=v[1]) for name, v in ARRAYS.items()}
    values.update(arrays)
    values.update(d_lse=0, d_depth=0, own_seen=None)
    got = _call(values)
    for name, a in arrays.items():
        if name != "own_seen":
            assert isinstance(got[name], C.c_void_p) and got[name].value == a.ctypes.data, name
    assert got["d_lse"].value is None and got["d_depth"].value is None and got["own_seen"] is None and got["n_groups"] == 2
    values.update(k_handles=None)                                        # a NULL array, for the library to refuse: the groups are counted by the other
    assert _call(values)["k_handles"] is None and _call(values)["n_groups"] == 2


def test_the_entry_on_the_null_engine_answers_with_the_no_data_path_status():
    """the fake device has a page table and no data path: SPECKV_ERR_DRIVER, like every data call; nothing is counted"""
    from cxl_speckv_amd.speckv_ctypes import SpeckvError
    raw = C.CDLL(pkg.build_library())
    assert hasattr(raw, ENTRY)
    raw.speckv_ext_abi_version.restype = C.c_uint32
    assert raw.speckv_ext_abi_version() == 6
    assert callable(pkg.SpeckvLib.attend_prefix_fold_kv)
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        a = lib.alloc(64 * 4096)
        buf = np.zeros(16384, dtype=np.uint8)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16
        before = bytes(lib.stats())
        u64, u32 = (lambda *v: np.asarray(v, dtype=np.uint64)), (lambda *v: np.asarray(v, dtype=np.uint32))
        for window, n_splits in ((0, 0), (0, 1), (40, 5), (40, 64)):
            with pytest.raises(SpeckvError) as err:
                lib.attend_prefix_fold_kv(u64(a), u64(a), u32(0, 1), 0, at, 1, 1, u32(2), u32(1), u32(3), 0, window, n_splits, 1.0, at, at, 1)
            assert err.value.status == -2                                 # SPECKV_ERR_DRIVER
        assert bytes(lib.stats()) == before and not buf.any()
    finally:
        lib.finalize()


# ----------------------------------------------------------------------------- the connector's refusals
class _NoLib:
    """a library that must not be called: the connector refuses in front of it"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


class _Q:
    shape = (2, 8, 4, 128)


def _connector(lengths=((1, 0), (2, 5), (50, 64), (51, 37))):
    conn = SpeckvSplitKVConnector(_NoLib(), 2, 8, 128, 256)
    for rid, n in lengths:
        conn.requests[rid] = _SplitRequest(1000 + rid, 2000 + rid)
        conn.requests[rid].length = n
    return conn


@pytest.mark.parametrize("method", ["attend_shared", "attend_chunk_shared"])
def test_the_connector_refuses_in_front_of_any_library_call(method):
    import torch

    def call(conn, req_ids, prefix_ids, q=None, **kw):
        q = _Q() if q is None else q
        if method == "attend_shared":
            return conn.attend_shared(0, req_ids, prefix_ids, q, 0.1, **kw)
        return conn.attend_chunk_shared(0, req_ids, prefix_ids, q, None, None, 0.1, **kw)
    conn = _connector()
    with pytest.raises(KeyError):
        call(conn, [1, 2], [50, 99])                                      # an unknown prefix
    with pytest.raises(KeyError):
        call(conn, [1, 98], [50, 50])                                     # an unknown member
    with pytest.raises(ValueError, match="member of the call"):
        call(conn, [1, 2], [50, 2])                                       # a prefix among the members
    with pytest.raises(ValueError, match="member of the call"):
        call(conn, [1, 50], [50, None])
    with pytest.raises(ValueError, match="prefix_lens and keep"):         # an odd prefix length without prefix_lens
        call(conn, [1, 2], [51, 51])
    with pytest.raises(ValueError):
        call(conn, [1, 2], [51, 51], prefix_lens=[36, 38])                # at most length & ~1 = 36
    with pytest.raises(ValueError):
        call(conn, [1, 2], [50])                                          # wrong list lengths
    with pytest.raises(ValueError):
        call(conn, [1, 2], [50, 50], prefix_lens=[64])
    for bad in (True, 2.0, "50", [50]):                                   # bools (and other non-integers) for ints
        with pytest.raises((ValueError, TypeError)):
            call(conn, [1, 2], [50, bad])
    for bad in (True, 2.5, "2", -2, 3, 66):
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], prefix_lens=[2, bad])
    with pytest.raises(ValueError):
        call(conn, [1, 2], [None, 50], prefix_lens=[2, 2])                # a member without a prefix has no length
    for bad in (-1, 65, True, 1.5):
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], splits=bad)
    for bad in (0, -3, True, 1.5, "64"):                                  # a bad window
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], window=bad)
    with pytest.raises(TypeError):                                        # a q that is no tensor
        call(conn, [1, 2], [50, 50])
    if method == "attend_shared":
        for g in (3, 5, 32):                                              # a bad G
            with pytest.raises(ValueError, match="1, 2, 4, 8 or 16"):
                call(conn, [1, 2], [50, 50], q=torch.zeros((2, 8, g, 128), dtype=torch.float16))
        with pytest.raises(ValueError):
            call(conn, [1, 2], [50, 50], q=torch.zeros((3, 8, 4, 128), dtype=torch.float16))
    assert [conn.length(r) for r in (1, 2, 50, 51)] == [0, 5, 64, 37]


def test_without_a_prefix_the_calls_reach_attend_and_attend_chunk_only():
    import torch
    conn = _connector()
    seen = []
    conn.attend = lambda *a: seen.append(("attend", a)) or "rows"
    conn.attend_chunk = lambda *a: seen.append(("attend_chunk", a)) or "chunk rows"
    q, qc, new = torch.zeros((2, 8, 4, 128), dtype=torch.float16), torch.zeros((2, 3, 8, 4, 128), dtype=torch.float16), torch.zeros((2, 3, 2, 8, 128), dtype=torch.float16)
    assert conn.attend_shared(1, [1, 2], [None, None], q, 0.1, window=40) == "rows"
    assert conn.attend_shared(1, [1, 2], [50, None], q, 0.1, prefix_lens=[0, None], stream="s") == "rows"      # every length 0
    assert conn.attend_chunk_shared(1, [1, 2], [None, None], qc, new, new, 0.1, n_new=[3, 1], window=40, parents=[-1, 0, 0], stream="s") == "chunk rows"
    assert seen == [("attend", (1, [1, 2], q, 0.1, None, 40)), ("attend", (1, [1, 2], q, 0.1, "s", None)),
                    ("attend_chunk", (1, [1, 2], qc, new, new, 0.1, [3, 1], "s", 1, 40, [-1, 0, 0]))]


def test_both_connectors_judge_a_shared_prefix_call_alike():
    """_shared_args of SpeckvKVConnector and of SpeckvSplitKVConnector over the same ids and lengths, 400 seeded calls: members in
    scattered order, None prefixes, given and absent prefix_lens, odd prefix lengths, unknown ids, bools / floats / strings in every
    list, bad splits and windows.  Both raise the same exception type with the same message, or return plans that agree on the
    order, the members, first_member and the lengths; an identical second call returns the kept plan object, and one behind a move
    of _epoch does not."""
    import random
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector, _Request
    lengths = ((1, 0), (2, 5), (3, 6), (4, 33), (50, 64), (51, 37), (52, 128))
    split = _connector(lengths)
    fp8 = SpeckvKVConnector(_NoLib(), num_layers=2, max_tokens=256, scheme="fp8")
    for rid, n in lengths:
        fp8.requests[rid] = _Request(1000 + rid)
        fp8.requests[rid].length = n
    have = dict(lengths)

    def judged(conn, args):
        req_ids, prefix_ids, prefix_lens, splits, window = args
        try:
            SpeckvKVConnector._shared_window(window)                      # as the methods of both do, in front of the lists
            return None, conn._shared_args(req_ids, prefix_ids, prefix_lens, splits, "attend_shared", window)
        except (ValueError, KeyError, TypeError) as e:
            return (type(e), str(e)), None

    rng = random.Random(20261021)
    junk = (True, False, 2.0, 1.5, "2", np.int64(2), np.bool_(True))
    plans = raised = permuted = 0
    for _ in range(400):
        req_ids = rng.sample([1, 2, 3, 4], rng.randint(1, 4))
        prefix_ids = [rng.choice([None, 50, 50, 51, 52]) for _ in req_ids]
        prefix_lens = None
        if rng.random() < 0.6:
            prefix_lens = [None if p is None or rng.random() < 0.2 else rng.randrange(0, have[p] + 1, 2) for p in prefix_ids]
        splits, window = rng.choice([0, 0, 1, 5, 64]), rng.choice([None, None, 1, 40, 300])
        roll = rng.random()
        if roll < 0.08:
            prefix_ids[rng.randrange(len(prefix_ids))] = rng.choice(junk + (99, req_ids[0], [50]))
        elif roll < 0.16 and prefix_lens is not None:
            prefix_lens[rng.randrange(len(prefix_lens))] = rng.choice(junk + (-2, 3, 37, 130, 0))
        elif roll < 0.22:
            req_ids[rng.randrange(len(req_ids))] = rng.choice((98, 50, True, 2.0))
        elif roll < 0.28:
            splits = rng.choice((-1, 65, True, 1.5, "1", None))
        elif roll < 0.34:
            window = rng.choice((0, -3, True, 1.5, "64", 2 ** 32))
        elif roll < 0.38:
            prefix_ids = prefix_ids[:-1]
        elif roll < 0.42 and prefix_lens is not None:
            prefix_lens = prefix_lens + [0]
        args = (req_ids, prefix_ids, prefix_lens, splits, window)
        (err_a, plan_a), (err_b, plan_b) = judged(fp8, args), judged(split, args)
        assert err_a == err_b, (args, err_a, err_b)
        if err_a is not None:
            raised += 1
            continue
        assert (plan_a is None) == (plan_b is None), args
        for conn, plan in ((fp8, plan_a), (split, plan_b)):
            assert judged(conn, args)[1] is plan                         # the kept plan of the step
        if plan_a is None:
            continue
        plans += 1
        permuted += plan_a[0] is not None
        assert plan_a[0] == plan_b[0] and plan_a[1] == plan_b[1], args    # the order, the members in it
        for a, b in ((plan_a[-2], plan_b[-2]), (plan_a[-1], plan_b[-1])):                 # first_member, the lengths
            assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b), args
        order = plan_a[0] if plan_a[0] is not None else list(range(len(req_ids)))
        assert plan_a[1] == [req_ids[b] for b in order]
        for conn, plan in ((fp8, plan_a), (split, plan_b)):
            conn._epoch += 1
            again = judged(conn, args)[1]
            assert again is not plan and again[1] == plan[1] and np.array_equal(again[-1], plan[-1])
    assert plans >= 100 and raised >= 60 and permuted >= 30, (plans, raised, permuted)     # the matrix reaches every kind of call


# ----------------------------------------------------------------------------- the float64 emulation
def _ceil(a, b):
    return -(-a // b)


def _f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _allocations(oracle, kv, head, t):
    """what the two allocations of a split request hold for one kv head, region by region: (E4M3 key values [L t][D], the block scale of
    every position's page [L t], the MXFP4 values as fp16 [L t][D]); region `layer` starts at position layer * t"""
    ke, ks, vv = [], [], []
    for layer in range(L):
        k8, v4 = _pair(oracle, kv, layer, t)
        r4 = k8.recs[:, :N].reshape(-1, 2, H, D)
        ke.append(k8.lut.astype(np.float64)[r4[:t // 2, :, head, :].reshape(-1, D)])
        ks.append(np.repeat(k8.scales[:t // 2].astype(np.float64), 2))
        vv.append(v4.kv(head)[1])
        assert np.array_equal(ke[-1] * ks[-1][:, None], k8.kv(head)[0])    # the rows the GPU tests' reference takes
    return np.concatenate(ke), np.concatenate(ks), np.concatenate(vv)


def _emulate(alloc, t, layer, lens, lo, q, own_out, own_lse, pieces=1, mutation=None):
    """the (FP8, MXFP4) k_attend_prefix (+ k_prefix_combine) for ONE group, ONE position per member and ONE head in float64.  Member m
    sees [lo[m], lens[m]) of region `layer`; q [M][R][D] fp16 values; own_out / own_lse what the member attended on its own.  Region
    `layer` of EITHER allocation starts at page layer * t / 2; tiles of 32 from the group's first tile to its largest length, staged
    as zeros beyond it (and beyond the allocation); the score = E4M3 values . q times the page's block scale times sm_scale; -inf
    outside the row's own [lo, len); the running maximum with the m_use path; p rounded to fp16 for the sum and the product; pieces
    by chunk_split_plan's forced rule over the tiles that are left, merged in ascending order by their maxima; the fold.  A row with
    lo >= len is dead and keeps what out / lse held.  mutation: one rule broken."""
    ke, ks, vv = alloc
    live = [m for m in range(len(lens)) if lo[m] < lens[m]]
    out, lse = own_out.copy(), own_lse.copy()
    if not live:
        return out, lse
    max_len, first_tile = max(lens[m] for m in live), min(lo[m] for m in live) >> 5
    n_pool = _ceil(max_len, 32)
    left = n_pool - first_tile
    tpp = _ceil(left, max(1, min(pieces, left)))
    n_pieces = _ceil(left, tpp)
    k_at = layer * t
    v_at = 2 * layer * t if mutation == "V from the K region's index as a single allocation" else layer * t

    def rows(a, at, n):                                                   # n staged positions from `at` on; zeros beyond the allocation
        got = np.zeros((32,) + a.shape[1:])
        have = max(0, min(n, len(a) - at))
        got[:have] = a[at:at + have]
        return got
    for m in live:
        for r in range(q.shape[1]):
            parts = []
            for piece in range(n_pieces):
                acc, m_run, l_run = np.zeros(D), -np.inf, 0.0
                for tile in range(first_tile + piece * tpp, min(first_tile + (piece + 1) * tpp, n_pool)):
                    pos = np.arange(32 * tile, 32 * tile + 32)
                    n = max(0, min(32, max_len - pos[0]))
                    Kt, St, Vt = rows(ke, k_at + pos[0], n), rows(ks, k_at + pos[0], n), rows(vv, v_at + pos[0], n)
                    if mutation == "the K page scale dropped":
                        St = np.ones(32)
                    s = np.where((pos >= lo[m]) & (pos < lens[m]), (Kt @ q[m, r]) * (SM * St), -np.inf)
                    m_new = max(m_run, s.max())
                    m_use = 0.0 if m_new == -np.inf else m_new
                    alpha = np.exp(m_run - m_use)
                    p = _f16(np.exp(s - m_use))
                    l_run, m_run, acc = l_run * alpha + p.sum(), m_new, acc * alpha + p @ Vt
                parts.append((acc, m_run, l_run))
            M = max(p[1] for p in parts)
            num, den = np.zeros(D), 0.0
            for acc, m_p, l_p in parts:                                   # ascending piece order
                w = 1.0 if mutation == "pieces merged without their maxima" else np.exp(m_p - M)
                num, den = num + acc * w, den + l_p * w
            own = own_lse[m, r]
            with np.errstate(invalid="ignore", divide="ignore"):
                lse_p = M + np.log(den)
                mx = max(own, lse_p)
                new = mx + np.log(np.exp(own - mx) + np.exp(lse_p - mx))
                out[m, r] = own_out[m, r] * np.exp(own - new) + (num / den) * np.exp(lse_p - new)
            lse[m, r] = new
    return out, lse


def _plain(alloc, t, layer, lens, lo, q, own_out, own_lse, own_mag):
    """the plain float64 softmax over prefix [lo, len) + own positions -> want, lse, sum p|v|"""
    ke, ks, vv = alloc
    want, wlse, mag = own_out.copy(), own_lse.copy(), own_mag.copy()
    for m in range(len(lens)):
        if lo[m] >= lens[m]:
            continue
        at = slice(layer * t + lo[m], layer * t + lens[m])
        s = (q[m] @ (ke[at] * ks[at][:, None]).T) * SM                   # [R][n]
        mx = s.max(axis=1)
        p = np.exp(s - mx[:, None])
        l = p.sum(axis=1)
        lse_p = mx + np.log(l)
        with np.errstate(invalid="ignore", divide="ignore"):
            new = np.logaddexp(own_lse[m], lse_p)
            w_own, w_pre = np.exp(own_lse[m] - new)[:, None], np.exp(lse_p - new)[:, None]
        want[m] = own_out[m] * w_own + (p @ vv[at]) / l[:, None] * w_pre
        mag[m] = own_mag[m] * w_own + (p @ np.abs(vv[at])) / l[:, None] * w_pre
        wlse[m] = new
    return want, wlse, mag


def _own_part(oracle, own, layer, head, q16, t):
    """a member's own attention in float64 as attend gives it: the stored part under the E4M3 query, the tail under the fp16 one"""
    R = q16.shape[0]
    n = own[0].shape[1]
    if n == 0:
        return np.zeros((R, D)), np.full(R, -np.inf), np.zeros((R, D))
    S_, V_ = [], []
    if n & ~1:
        k8, v4 = _pair(oracle, own, layer, t)
        S_.append(k8.q_rows(q16) @ k8.kv(head)[0][:n & ~1].T); V_.append(v4.kv(head)[1][:n & ~1])
    if n & 1:
        S_.append(q16.astype(np.float64) @ own[0][layer, n - 1, head].astype(np.float64)[:, None]); V_.append(own[1][layer, n - 1, head].astype(np.float64)[None])
    s, v = np.concatenate(S_, axis=1) * SM, np.concatenate(V_)
    mx = s.max(axis=1)
    p = np.exp(s - mx[:, None])
    l = p.sum(axis=1)
    return (p @ v) / l[:, None], mx + np.log(l), (p @ np.abs(v)) / l[:, None]


HEADS = (0, 5)


def _cases(oracle):
    """the GPU cases' contents at layer 1, rows_per_pos 4: (name, allocation rows, t, lens, lo, q, own (out, lse, mag), piece counts)
      decode  the 254-position prefix, members that see 2, 36, 64, 98, 254 of it behind 0, 1, 2, 37, 64 positions of their own
      window  W = 70 over the same prefix: lo = 189 inside a tile, 192 on a tile boundary, a dead member, shorter lengths
      split   T = 512, the 480-position prefix (15 tiles), members that see 480, 34, 480, 2: whole, 2, 3 and 15 pieces"""
    prefix, _, long_, owns, q = _inputs(4)
    for head in HEADS:
        alloc = _allocations(oracle, prefix, head, T)
        qd = q[:5, head]
        own = [_own_part(oracle, owns[n], LAYER, head, qd[m], T) for m, n in enumerate(OWN)]
        stack = lambda i, parts: np.stack([p[i] for p in parts])
        yield f"decode head {head}", alloc, T, PLENS, [0] * 5, qd.astype(np.float64), [stack(i, own) for i in range(3)], [1]
        nothing = [np.zeros((5, 4, D)), np.full((5, 4), -np.inf), np.zeros((5, 4, D))]
        lo = [max(0, n + s - W) for n, s in zip(WIN_LENS, WIN_SEEN)]
        assert lo == [189, 192, 254, 58, 30]
        yield f"window head {head}", alloc, T, WIN_LENS, lo, qd.astype(np.float64), nothing, [1, 2]
        own = [_own_part(oracle, owns[n], LAYER, head, q[m, head], T2) for m, n in enumerate((37, 64, 0, 1))]
        yield (f"split head {head}", _allocations(oracle, long_, head, T2), T2, [480, 34, 480, 2], [0] * 4, q[:4, head].astype(np.float64),
               [stack(i, own) for i in range(3)], [1, 2, 3, 15])


def _worst(case, mutation=None):
    """the worst |err| / (2e-3 sum p|v| + 1e-6) and |lse err| / 2e-3 of a case over its piece counts (NaN counts as infinite)"""
    name, alloc, t, lens, lo, q, (own_out, own_lse, own_mag), pieces = case
    want, wlse, mag = _plain(alloc, t, LAYER, lens, lo, q, own_out, own_lse, own_mag)
    worst = 0.0
    for n in pieces:
        got, lse = _emulate(alloc, t, LAYER, lens, lo, q, own_out, own_lse, n, mutation)
        live = np.asarray(lo) < np.asarray(lens)
        with np.errstate(invalid="ignore"):
            e = np.abs(got[live] - want[live]) / (2e-3 * mag[live] + 1e-6)
            le = np.abs(lse[live] - wlse[live]) / 2e-3
        worst = max(worst, float(np.nan_to_num(e, nan=np.inf).max()), float(np.nan_to_num(le, nan=np.inf).max()))
        assert np.array_equal(got[~live], own_out[~live]) and np.array_equal(lse[~live], own_lse[~live])       # dead rows keep their bits
    return worst


def test_the_emulated_walk_stays_within_half_the_bound(oracle):
    """the emulation against the plain float64 softmax over the GPU cases' contents: within 0.5 of 2e-3 sum p|v| + 1e-6 and of 2e-3 on
    the lse -- the tier-1 line of DESIGN "Accuracy over value ranges": what the walk's own roundings (fp16(p)) cost leaves the GPU its
    margin.  Measured: 0.07 - 0.11 of the bound in the decode and split cases, 0.10 - 0.14 under the window (the worst: 0.139, W = 70,
    head 0)"""
    worst = {case[0]: _worst(case) for case in _cases(oracle)}
    print("emulated walk, worst err / tol:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("mutation", ["V from the K region's index as a single allocation", "the K page scale dropped", "pieces merged without their maxima"])
def test_every_mutation_of_a_rule_is_caught_by_the_same_check(oracle, mutation):
    """each broken rule moves some row of the emulated cases outside the bound the GPU tests assert (or makes it NaN)"""
    broken = [case[0] for case in _cases(oracle) if _worst(case, mutation) > 1.0]
    assert broken, mutation
    if "pieces" in mutation:
        assert all("split" in name or "window" in name for name in broken)
