"""-m gpu: speckv_ext_attend_kv_batch (k_attend_k8v4 and the merge behind direct_per_seq = 1) against float64 in every launch geometry
attend_geometry.hpp decides for BatchShape{fp8 = true} -- tests/test_gpu_k8v4_decode.py stays below 8 members of 8 tiles and reaches the
pieces only by a forced attend_tiles_per_split.

Each case E1 .. E5 (tests/_k8v4_cases.py) proves on the host first, by the rules the engine decides with, that it reaches its regime:
rule-priced uneven pieces; more workgroup columns than CUs; a heavy tail dispatched rows-first with final, partial, zero and padded rows
in one launch; the serpentine order[]; one piece of 128 tiles.  Then: members whose layouts differ in num_tokens in one call, the NULL
(synchronous) stream, and the refusal of a member in more than 2048 pieces.

Contents: tests/_k8v4_cases.py content() -- MXFP4 block codes and FP8 page scales that change from neighbour to neighbour (a wrong code
byte or scale index shows), 3 per regime written once with write_prefill; member i reads the handle pair of content i % 3 with its own
pos_end and its own query rows (the entry only reads: a pair may appear many times in a call).
Reference and bound: those of tests/test_gpu_k8v4_decode.py (_check: float64 attention over the oracle's FP8 records of K and MXFP4 records
of V with the oracle's E4M3 query; |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta; an empty member exactly 0 / -inf),
every (member, head, row) of out and lse; out and lse start as a fill pattern of which nothing may survive.
tests/test_k8v4_decode_geometry_cpu.py shows without a GPU that the contents are sharp and that the bound is meetable on them."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests import _k8v4_cases as cases
from tests._gpu import D, H, HeadChecker, set_tuning, torch_mod
from tests._rules import DEFAULT_TUNING, decide, load_rules
from tests.test_gpu_k8v4_decode import FP8, MX4, PATTERN, SM, _check
from tests.test_gpu_spec_step import _region

pytestmark = pytest.mark.gpu
L = 2


class _Pool:
    """ONE library for the module; a split connector per num_tokens, the contents of a case written once, their checkers built once"""

    def __init__(self, torch, lib):
        self.torch, self.lib = torch, lib
        self.conns, self.handles, self.checkers, self.keep = {}, {}, {}, []

    def conn(self, T):
        if T not in self.conns:
            self.conns[T] = SpeckvSplitKVConnector(self.lib, L, H, D, T)
        return self.conns[T]

    def write(self, tag, contents, T):
        """[(K handle, V handle)] of the contents [(k, v)] ([L][n][H][D], n <= T), each in a request of its own of the connector of T"""
        if tag not in self.handles:
            conn, torch = self.conn(T), self.torch
            got = []
            for c, (k, v) in enumerate(contents):
                got.append(conn.add_request((tag, c)))
                self.keep += conn.write_prefill((tag, c), torch.from_numpy(np.ascontiguousarray(k)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda())
            torch.cuda.synchronize()
            self.handles[tag] = got
        return self.handles[tag]

    def checker(self, oracle, tag, c, layer, k, v):
        """(HeadChecker over the FP8 records, HeadChecker over the MXFP4 records) of content c of `tag` at `layer`, as
        tests/test_gpu_k8v4_decode.py _checker builds them, over the rows that were written"""
        key = (tag, c, layer)
        if key not in self.checkers:
            n = k.shape[1]
            region = _region(k[layer], v[layer], n)
            self.checkers[key] = (HeadChecker(oracle, FP8, region, n), HeadChecker(oracle, MX4, region, n))
        return self.checkers[key]


@pytest.fixture(scope="module")
def pool():
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    p = _Pool(torch, lib)
    try:
        yield p
    finally:
        torch.cuda.synchronize()
        p.keep.clear()
        lib.finalize()


@pytest.fixture(scope="module")
def rules():
    return load_rules()


def _cus():
    return torch_mod().cuda.get_device_properties(0).multi_processor_count


def _launch(pool, pairs, pos_end, q, layer, null_stream=False, refused=False):
    """speckv_ext_attend_kv_batch over the handle pairs [(K, V)] -> (out [n][H][G][D], lse [n][H][G]) as fp32 numpy; both start as the fill
    pattern.  refused: the call must raise SpeckvError -> (its status, out, lse)"""
    torch = pool.torch
    n, _, G, _ = q.shape
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((n, H, G, D), PATTERN, dtype=torch.int32, device="cuda")
    lse = torch.full((n, H, G), PATTERN, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    call = lambda: pool.lib.attend_kv_batch(np.asarray([p[0] for p in pairs], np.uint64), np.asarray([p[1] for p in pairs], np.uint64), layer,
                                            dq.data_ptr(), G, np.asarray(pos_end, np.uint32), SM, out.data_ptr(), lse.data_ptr(),
                                            0 if null_stream else st.cuda_stream)
    status = None
    if refused:
        with pytest.raises(SpeckvError) as e:
            call()
        status = e.value.status
    else:
        call()
    st.synchronize()                                                         # (the NULL stream's call has returned synchronised)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.float32), lse.cpu().numpy().view(np.float32)
    return (status,) + got if refused else got


def _nothing_of_the_pattern(out, lse, what):
    assert not (out.view(np.uint32) == PATTERN).any() and not (lse.view(np.uint32) == PATTERN).any(), (what, "a row was not written")


def _regime_call(pool, name, g, layer, n_cus, null_stream=False):
    lens = cases.regime(name, n_cus)
    contents = cases.case_contents(name, cases.layout_tokens(lens))
    handles = pool.write(name, contents, cases.layout_tokens(lens))
    q = cases.case_queries(name, len(lens), g)
    out, lse = _launch(pool, [handles[i % len(contents)] for i in range(len(lens))], lens, q, layer, null_stream)
    return lens, contents, q, out, lse


def _check_members(pool, oracle, tag, contents, owner, out, lse, q, lens, layer, what):
    """every member against float64, content by content (member i holds content owner[i]); the worst err / tol"""
    worst, owner, lens = 0.0, np.asarray(owner), np.asarray(lens)
    for c, (k, v) in enumerate(contents):
        idx = np.nonzero(owner == c)[0]
        if len(idx):
            worst = max(worst, _check(pool.checker(oracle, tag, c, layer, k, v), out[idx], lse[idx], q[idx], lens[idx], (what, "content", c)))
    return worst


# ----------------------------------------------------------------------------- E1 .. E5
E_CASES = [(name, g, layer) for name in cases.REGIMES for g in cases.G_OF[name] for layer in cases.LAYERS_OF[name]]


@pytest.mark.parametrize("name,g,layer", E_CASES, ids=[f"{n}-g{g}-layer{l}" for n, g, l in E_CASES])
def test_every_launch_geometry_against_float64(pool, oracle, rules, name, g, layer):
    n_cus = _cus()
    d = cases.assert_branch(rules, name, cases.regime(name, n_cus), n_cus)
    lens, contents, q, out, lse = _regime_call(pool, name, g, layer, n_cus)
    _nothing_of_the_pattern(out, lse, (name, g, layer))
    worst = _check_members(pool, oracle, name, contents, np.arange(len(lens)) % len(contents), out, lse, q, lens, layer, (name, g, layer))
    print(f"attend_kv_batch {name} ({len(lens)} members, {d['tps']} tiles a piece, {d['max_splits']} pieces at most, by length {d['by_length']}, "
          f"rows first {d['rows_first']}) g {g} layer {layer}: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- layouts that differ in num_tokens
def test_members_of_two_layouts_in_one_call(pool, oracle):
    """8 members in turn from a connector of num_tokens 256 and one of 1024 on the same library, layer 1: the K and the V region of a
    member start at ITS num_tokens / 2 pages (AttendSeq::k_first, AttendKvSide::v_first per member)"""
    layer, g = 1, 8
    tokens = (256, 1024)
    lens = np.array([0, 2, 34, 258, 98, 640, 256, 1024])
    contents = {T: cases.mixed_contents(T) for T in tokens}
    handles = {T: pool.write(("mixed", T), contents[T], T) for T in tokens}
    side, owner = np.arange(len(lens)) % 2, np.arange(len(lens)) // 2 % 2
    assert all(lens[i] <= tokens[side[i]] for i in range(len(lens)))
    q = cases.case_queries("E1", len(lens), g)
    out, lse = _launch(pool, [handles[tokens[side[i]]][owner[i]] for i in range(len(lens))], lens, q, layer)
    _nothing_of_the_pattern(out, lse, "mixed layouts")
    worst = 0.0
    for s, T in enumerate(tokens):
        idx = np.nonzero(side == s)[0]
        worst = max(worst, _check_members(pool, oracle, ("mixed", T), contents[T], owner[idx], out[idx], lse[idx], q[idx], lens[idx], layer, ("mixed", T)))
    print(f"attend_kv_batch layouts of 256 and 1024 tokens in one call: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- the NULL stream
def test_the_null_stream_gives_the_bits_of_the_stream_call(pool, oracle, rules):
    """E3 at g = 8, layer 1 with stream = NULL (the engine's stream, a synchronous call): bit for bit what the call on a stream gives"""
    n_cus = _cus()
    cases.assert_branch(rules, "E3", cases.regime("E3", n_cus), n_cus)
    lens, contents, q, out, lse = _regime_call(pool, "E3", 8, 1, n_cus)
    _, _, _, out0, lse0 = _regime_call(pool, "E3", 8, 1, n_cus, null_stream=True)
    _nothing_of_the_pattern(out0, lse0, "NULL stream")
    assert np.array_equal(out0.view(np.uint32), out.view(np.uint32)) and np.array_equal(lse0.view(np.uint32), lse.view(np.uint32))
    worst = _check_members(pool, oracle, "E3", contents, np.arange(len(lens)) % len(contents), out0, lse0, q, lens, 1, "NULL stream")
    print(f"attend_kv_batch E3 on the NULL stream: worst err / tol {worst:.3f}")


# ----------------------------------------------------------------------------- a member in more than 2048 pieces
class _ThenNeverWritten:
    """a HeadChecker pair's side whose written rows are followed by positions that were never written: zero rows of K and of V"""

    def __init__(self, checker, n):
        self.checker, self.n, self._kv = checker, n, {}

    def kv(self, head):
        if head not in self._kv:
            self._kv = {head: tuple(np.concatenate([x, np.zeros((self.n - len(x), D))]) for x in self.checker.kv(head))}      # (one head at a time: 67 MB a side)
        return self._kv[head]

    def q_rows(self, q16):
        return self.checker.q_rows(q16)


def test_a_member_in_more_than_2048_pieces_is_refused(pool, oracle, rules):
    """One member of num_tokens 65 600 with 64 positions written and pos_end = 65 568 (2049 tiles), layer 1.  With attend_tiles_per_split = 1
    that is 2049 pieces: SPECKV_ERR_INVAL (BatchGeometry::fits), nothing written.  With the key back at 0 the same call is served: float64
    over the 64 written positions and 65 504 never-written ones (score 0, V 0: lse >= ln 65 504)."""
    T, written, pos_end, layer, g = 65600, 64, 65568, 1, 8
    n_cus = _cus()
    pages = np.array([pos_end // 2])
    assert decide(rules, FP8, "batch", pages, n_cus, tuning=(1,) + DEFAULT_TUNING[1:])["fits"] == 0
    served = decide(rules, FP8, "batch", pages, n_cus)
    assert served["fits"] == 1 and (pages[0] + 15) // 16 == 2049
    k, v = cases.bound_content()
    handles = pool.write("bound", [(k, v)], T)
    q = cases.case_queries("E5", 1, g)
    try:
        set_tuning("attend_tiles_per_split", 1)
        status, out, lse = _launch(pool, handles, [pos_end], q, layer, refused=True)
        assert status == -4                                                  # SPECKV_ERR_INVAL
        assert (out.view(np.uint32) == PATTERN).all() and (lse.view(np.uint32) == PATTERN).all(), "a refused call wrote something"
    finally:
        set_tuning("attend_tiles_per_split", 0)
    out, lse = _launch(pool, handles, [pos_end], q, layer)
    _nothing_of_the_pattern(out, lse, "2049 tiles")
    pair = tuple(_ThenNeverWritten(c, pos_end) for c in pool.checker(oracle, "bound", 0, layer, k, v))
    worst = _check(pair, out, lse, q, [pos_end], "2049 tiles")
    assert np.all(lse >= np.log(pos_end - written) - 1e-3)
    print(f"attend_kv_batch 2049 tiles ({served['tps']} tiles a piece, {served['max_splits']} pieces): worst err / tol {worst:.3f}")
    pool.conn(T).free_request(("bound", 0))
    del pool.handles["bound"]
