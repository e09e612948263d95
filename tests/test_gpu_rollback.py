"""-m gpu: the rollback of committed positions -- speckv_ext_read_pairs (one launch decodes position rows out of the records where
they lie) and SpeckvKVConnector.truncate on top of it.

References: speckv_ext_fetch_range for the bits of a row; for attention, the two-step float64 reference of
tests/test_gpu_spec_step.py::test_attend_spec_end_to_end with its tolerance (HeadChecker.want over the stored pairs, then the float64
chained fold of every position held outside the pool)."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, HeadChecker, torch_mod
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_spec_step import SCHEMES, _region, chained_folds

pytestmark = pytest.mark.gpu
PAGE, ROW = 4096, 2048
L, T = 2, 128
STEP = T // 2                                   # pages of one (layer, kind) region
FIRSTS = [0, 15, 16, 40]                        # MXFP4 tile rows 0, 15 and 16 (a tile edge is crossed); page 40 of every region is never written
STRIDE = ROW + 64                               # bytes between the layers of a row: larger than a row
SENTINEL = 0x7C5A


def _blocks(n, seed):
    """fp16 page images: random, a few that compress (constant runs, zeros)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ROW)).astype(np.float16)
    x[3] = 0
    x[5] = np.repeat(x[5, :64], 32)
    x[15, 1024:] = x[15, 1024]
    return x


def _fill(lib, h, x):
    """every page of the allocation from x, except page 40 of every (layer, kind) region"""
    for j in range(2 * L):
        for lo, hi in ((j * STEP, j * STEP + 40), (j * STEP + 41, (j + 1) * STEP)):
            part = np.ascontiguousarray(x[lo:hi])
            lib.write(h, lo * PAGE, part.ctypes.data, part.nbytes, False)


def _check_read_pairs(lib, torch, handles, what):
    """read_pairs over FIRSTS of every handle against fetch_range of the whole allocation, for three selections of rows"""
    n_pages = 2 * L * STEP
    st = torch.cuda.Stream()
    refs = []
    for h in handles:
        ref = torch.empty((n_pages, ROW), dtype=torch.float16, device="cuda")
        lib.fetch_range(h, 0, n_pages, ref.data_ptr(), False, st.cuda_stream)
        refs.append(ref)
    st.synchronize()
    refs = [r.cpu().numpy().view(np.uint16) for r in refs]
    for h, r in zip(handles, refs):
        assert not r[40].any() and not r[40 + 3 * STEP].any(), (what, "a page never written decodes to zeros")
        assert r[0].any() and r[16 + STEP].any()
    pairs = [(i, f) for i in range(len(handles)) for f in FIRSTS]
    for sel in ((0, 1, 2, 3), (0, 2), (1, 3)):
        bufs = [[torch.full((L * STRIDE // 2,), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(4)] for _ in pairs]
        rows = np.asarray([[b[k].data_ptr() if k in sel else 0 for k in range(4)] for b in bufs], dtype=np.uint64)
        torch.cuda.synchronize()
        lib.read_pairs(np.asarray([handles[i] for i, _ in pairs], dtype=np.uint64), np.asarray([f for _, f in pairs], dtype=np.uint64), rows,
                       STEP, L, STRIDE, st.cuda_stream)
        st.synchronize()
        for (i, f), b in zip(pairs, bufs):
            for k in range(4):
                got = b[k].cpu().numpy().view(np.uint16).reshape(L, STRIDE // 2)
                assert np.all(got[:, ROW // 2:] == SENTINEL), (what, sel, i, f, k, "the gap between two layers was written")
                if k not in sel:
                    assert np.all(got == SENTINEL), (what, sel, i, f, k, "a row nobody asked for was written")
                    continue
                for layer in range(L):
                    page = f + (2 * layer + k // 2) * STEP
                    want = refs[i][page].reshape(2, ROW // 2)[k & 1]
                    assert np.array_equal(got[layer, :ROW // 2], want), (what, sel, i, f, k, layer)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_read_pairs_is_fetch_range_bit_for_bit(scheme, mode):
    """Every scheme in both quantiser modes; an allocation in one run (INT8_DELTA_RLE: a sealed one beside it), one striped over two
    pools of the one GPU and one of them with pages migrated; pairs at MXFP4 tile rows 0, 15 and 16 and one never written (zeros);
    all four rows, the even rows only, the odd rows only -- rows not wanted and the gap behind every row keep their sentinel."""
    torch = torch_mod()
    n_pages = 2 * L * STEP
    x = _blocks(n_pages, 100 + scheme)
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        handles = [lib.alloc(n_pages * PAGE)]
        _fill(lib, handles[0], x)
        if scheme == 2:
            handles.append(lib.alloc(n_pages * PAGE))
            _fill(lib, handles[1], x[::-1])
            lib.compact(handles[1])                                   # sealed: packed records
        _check_read_pairs(lib, torch, handles, ("one run", scheme, mode))
    finally:
        lib.finalize()
    lib = open_lib(SPECKV_POOL_DEVICES="0,0")
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        handles = [lib.alloc(n_pages * PAGE), lib.alloc(n_pages * PAGE)]
        _fill(lib, handles[0], x)
        _fill(lib, handles[1], x[::-1])
        lib.migrate(handles[1], 15, 3, 1)                              # pages 15..17 now lie in pool 1, wherever they lay
        lib.migrate(handles[1], STEP, 1, 0)
        _check_read_pairs(lib, torch, handles, ("striped / migrated", scheme, mode))
    finally:
        lib.finalize()


def test_read_pairs_refuses_bad_arguments_and_launches_nothing():
    torch = torch_mod()
    lib = open_lib()
    try:
        n_pages = 2 * L * STEP
        lib.set_compression_scheme(4)
        h = lib.alloc(n_pages * PAGE)
        x = _blocks(n_pages, 7)
        lib.write(h, 0, x.ctypes.data, x.nbytes, False)
        lib.set_compression_scheme(3)
        h_other = lib.alloc(n_pages * PAGE)
        buf = torch.full((4, L * STRIDE // 2), SENTINEL, dtype=torch.int16, device="cuda")
        at = [buf[k].data_ptr() for k in range(4)]
        assert all(a % 16 == 0 for a in at)
        s = torch.cuda.Stream().cuda_stream
        u64 = lambda *v: np.asarray(v, dtype=np.uint64)
        inval = [
            dict(stream=0),                                            # NULL stream
            dict(rows=u64([at[0] + 8, at[1], at[2], at[3]])),          # a row not 16-byte aligned
            dict(rows=u64([at[0], 0, at[2], at[3] + 2])),
            dict(stride=STRIDE - 8),                                   # a stride that is no multiple of 16
            dict(step=0),
            dict(handles=u64(h, h_other), firsts=u64(0, 0), rows=u64(at, at)),      # allocations of different schemes
        ]
        general = [
            dict(handles=u64(h + 12345)),                              # an unknown handle
            dict(firsts=u64(STEP + 1)),                                # the last page leaves the allocation
            dict(firsts=u64(n_pages)),
            dict(step=n_pages),
        ]
        for status, cases in ((-4, inval), (-1, general)):
            for c in cases:
                a = dict(handles=u64(h), firsts=u64(0), rows=u64(at), step=STEP, layers=L, stride=STRIDE, stream=s)
                a.update(c)
                with pytest.raises(SpeckvError) as e:
                    lib.read_pairs(a["handles"], a["firsts"], a["rows"], a["step"], a["layers"], a["stride"], a["stream"])
                assert e.value.status == status, (c, e.value.status)
        for name in ("handles", "firsts", "rows"):                    # NULL arrays
            args = dict(handles=u64(h).ctypes.data, firsts=u64(0).ctypes.data, rows=u64(at).ctypes.data)
            args[name] = None
            with pytest.raises(SpeckvError) as e:
                lib._ext("speckv_ext_read_pairs", args["handles"], args["firsts"], args["rows"], 1, STEP, L, STRIDE, s)
            assert e.value.status == -4, name
        lib.read_pairs(u64(), u64(), u64(), STEP, L, STRIDE, s)                         # no pairs: nothing to do, fine
        lib.read_pairs(u64(h), u64(0), u64(at), STEP, 0, STRIDE, s)                     # no layers
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), "a refused call wrote to its destination"
        lib.read_pairs(u64(h), u64(0), u64(at), STEP, L, STRIDE, s)                     # ... and the good call does
        torch.cuda.synchronize()
        assert not bool((buf[:, :ROW // 2] == SENTINEL).all())
    finally:
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------- the connector
def _grow(conn, torch, rid, k, v):
    """request rid prefilled with all but the last of k / v [L][n][H][D] (host fp16) and appended to n positions"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = k.shape[1]
    conn.add_request(rid)
    keep = []
    if n > 1:
        keep += conn.write_prefill(rid, dev(k[:, :n - 1]), dev(v[:, :n - 1]))
    if n:
        keep += conn.append([rid], dev(k[:, n - 1])[None], dev(v[:, n - 1])[None])
    torch.cuda.synchronize()
    return keep


def _tail(conn, rid, layer):
    r = conn.requests[rid]
    return (None, None) if r.tail_k is None else (r.tail_k[layer].cpu().numpy(), r.tail_v[layer].cpu().numpy())


def _check_attend(oracle, torch, conn, scheme, rids, data, layer, rng, what, kscale=None):
    """attend() of the batch against float64 over what the connector holds: the stored pairs through HeadChecker.want (the oracle's
    records of the rows data[rid] = (k, v) [L][n][H][D] that the pairs were encoded from), the held position (fp16, as it is) folded
    in float64.  kscale [L][H][D] (powers of two): the connector's K pre-scale -- data holds K as stored (k / scale), and the
    reference takes the query the connector hands to the kernels, fp16(q * scale)."""
    G, sm = 4, 1.0 / np.sqrt(D)
    q = rng.standard_normal((len(rids), H, G, D)).astype(np.float16)
    got = conn.attend(layer, rids, torch.from_numpy(q).cuda(), sm).cpu().numpy()
    assert np.all(np.isfinite(got)), what
    if kscale is not None:
        q = (q.astype(np.float32) * kscale[layer][None, :, None, :]).astype(np.float16)
    worst = 0.0
    for b, rid in enumerate(rids):
        k, v = data[rid]
        n = conn.length(rid)
        even = n & ~1
        checker = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], T), T)
        tk, tv = _tail(conn, rid, layer)
        assert (tk is not None) == bool(n & 1), (what, rid, n)
        for head in range(H):
            w_out, w_lse, w_mag, delta = checker.want(q[b, head], head, even, sm)
            want, mag, folds = w_out.astype(np.float64), w_mag.astype(np.float64), 0
            if n & 1:
                want, _, mag = chained_folds((w_out, w_mag), w_lse, q[b, head], tk[None, head], tv[None, head], sm)
                folds = 1
            if n == 0:
                assert not got[b, head].any()
                continue
            err = np.abs(got[b, head] - want)
            tol = (2e-3 + 2 * delta) * mag + 1e-6 + folds * (2e-5 * np.abs(want) + 2e-6)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (what, scheme, rid, n, head, float((err / tol).max()), delta)
    print(f"{what} {scheme}: attend worst err / tol {worst:.3f}")


CUTS = [(33, 32), (33, 31), (34, 33), (64, 1), (65, 65), (2, 0), (5, 4)]


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_truncate_leaves_the_state_of_a_connector_that_stopped_there(oracle, scheme):
    """A -> B: a request prefilled and appended to length A, cut to B.  Afterwards length, kv_rows of every position below B and the
    tail rows are the truth -- fetch_range-decoded pages for stored positions, the decoded stored row for a tail read back (both are
    what kv_rows gave before the cut), the held fp16 row for a tail that stayed -- and attend meets float64 over exactly those."""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(11)
        data, keep = {}, []
        for group in (CUTS[:4], CUTS[4:]):                                # batches of at most 6
            rids = [100 + a * 10 + b % 10 for a, b in group]
            for rid, (a, _) in zip(rids, group):
                data[rid] = (rng.standard_normal((L, a, H, D)).astype(np.float16), rng.standard_normal((L, a, H, D)).astype(np.float16))
                keep += _grow(conn, torch, rid, *data[rid])
            before = {(rid, layer, kind): conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16) for rid in rids for layer in range(L) for kind in (0, 1)}
            epoch = conn._epoch
            conn.truncate(rids, [b for _, b in group])
            torch.cuda.synchronize()
            assert conn._epoch != epoch and conn._arg_key is None
            for rid, (a, b) in zip(rids, group):
                assert conn.length(rid) == b
                for layer in range(L):
                    for kind in (0, 1):
                        after = conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16)
                        assert after.shape[0] == b and np.array_equal(after, before[(rid, layer, kind)][:b]), (scheme, a, b, layer, kind)
                    tk, tv = _tail(conn, rid, layer)
                    if b & 1:
                        assert np.array_equal(tk.view(np.uint16), before[(rid, layer, 0)][b - 1]) and np.array_equal(tv.view(np.uint16), before[(rid, layer, 1)][b - 1])
                    else:
                        assert tk is None and tv is None
            for layer in range(L):
                _check_attend(oracle, torch, conn, scheme, rids, data, layer, rng, f"cuts {group} layer {layer}")
            for rid in rids:
                conn.free_request(rid)
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_stale_records_behind_the_cut_are_never_seen(oracle, scheme):
    """The positions to be dropped carry K rows of 200 x the magnitude of the kept ones and V rows of 1000; cuts into the middle of a
    32-position tile (40 -> 35, 40 -> 34) and onto a tile boundary (64 -> 32).  attend, and attend_spec with S = 3 as a chain and as a
    two-leaf tree, meet the float64 reference over the kept positions within the tolerances of the test above.  truncate clears
    nothing: the attention kernels mask what lies at or beyond their range.  Without that masking (or a clearing) this test fails by
    orders of magnitude -- one stale position of score ~200 x takes the whole softmax and puts 1000 into every output element."""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(23)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        cuts = [(40, 35), (40, 34), (64, 32)]
        rids, data, keep = [1, 2, 3], {}, []
        for rid, (a, b) in zip(rids, cuts):
            k, v = rng.standard_normal((L, a, H, D)).astype(np.float16), rng.standard_normal((L, a, H, D)).astype(np.float16)
            k[:, b:] *= np.float16(200.0)
            v[:, b:] = (np.sign(v[:, b:].astype(np.float32)) * 1000.0).astype(np.float16)
            data[rid] = (k, v)
            keep += _grow(conn, torch, rid, k, v)
        conn.truncate(rids, [b for _, b in cuts])
        for layer in range(L):
            _check_attend(oracle, torch, conn, scheme, rids, data, layer, rng, f"stale, layer {layer}")
        # a step of 3 new positions on top: chain, then a tree of a root with two leaves
        S, rpp, layer, sm = 3, 4, 1, 1.0 / np.sqrt(D)
        B = len(rids)
        q = rng.standard_normal((B, S, H, rpp, D)).astype(np.float16)
        k_new, v_new = rng.standard_normal((B, S, L, H, D)).astype(np.float16), rng.standard_normal((B, S, L, H, D)).astype(np.float16)
        for parents, sees in ((None, [[0], [0, 1], [0, 1, 2]]), ([-1, 0, 0], [[0], [0, 1], [0, 2]])):
            got = conn.attend_spec(layer, rids, dev(q), dev(k_new), dev(v_new), sm, parents=parents).cpu().numpy()
            assert np.all(np.isfinite(got))
            worst = 0.0
            for b, rid in enumerate(rids):
                k, v = data[rid]
                n = conn.length(rid)
                even = n & ~1
                checker = HeadChecker(oracle, SCHEMES[scheme], _region(k[layer, :even], v[layer, :even], T), T)
                tk, tv = _tail(conn, rid, layer)
                for head in range(H):
                    q_head = q[b, :, head].reshape(S * rpp, D)
                    w_out, w_lse, w_mag, delta = checker.want(q_head, head, even, sm)
                    for j in range(S):
                        r = slice(j * rpp, (j + 1) * rpp)
                        kh = np.stack(([tk[head]] if n & 1 else []) + [k_new[b, t, layer, head] for t in sees[j]])
                        vh = np.stack(([tv[head]] if n & 1 else []) + [v_new[b, t, layer, head] for t in sees[j]])
                        want, _, mag = chained_folds((w_out[r], w_mag[r]), w_lse[r], q_head[r], kh, vh, sm)
                        err = np.abs(got[b, j, head] - want)
                        tol = (2e-3 + 2 * delta) * mag + 1e-6 + len(kh) * (2e-5 * np.abs(want) + 2e-6)
                        worst = max(worst, float((err / tol).max()))
                        assert np.all(err <= tol), (scheme, parents, rid, head, j, float((err / tol).max()), delta)
            print(f"stale {scheme} attend_spec parents={parents}: worst err / tol {worst:.3f}")
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme,prescale", [("fp8", False), ("int4", False), ("mxfp4", False), ("fp8", True), ("int4", True)])
def test_rollback_then_continue(oracle, scheme, prescale):
    """commit() of 4 draft positions, truncate to 1, 2 and 3 of them across a batch of 3 requests (prompts 37, 63, 22: one cut drops
    a tail, two read a row back), then append_tokens of 2 more; a twin connector goes through append_tokens(n_accept) instead.
    After the cut: lengths agree; the twin's tails are the fp16 rows as given, the rolled-back connector's tails are exactly those
    rows through the format once -- the oracle's encode and decode of the pair the commit stored -- for every layer, K and V.
    After the continue: lengths and tails (bit for bit: both hold the same new row) agree, every position in front of the pair the
    rollback reopened agrees bit for bit, and attend() of EACH connector meets float64 over the values it holds, with the reference
    and tolerance of the tests above: the twin's pairs are encoded from the rows as given, the rolled-back connector's reopened
    pair from (the row read back, its new partner).  The two are not asked to agree with each other.
    With a K pre-scale (channels scaled by 4 and 1/4) everything above is in the stored scaling, K / scale: a row read back that
    were scaled a second time -- by truncate or by the commit that pairs it -- would fail the tail equality or the attention."""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        a, b = SpeckvKVConnector(lib, L, H, D, T, scheme), SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(5)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        rnd = lambda *shape: rng.standard_normal(shape).astype(np.float16)
        kscale = None
        if prescale:
            kscale = np.ones((L, H, D), np.float32)
            kscale[:, :, 0::8] = 4.0; kscale[:, :, 3::8] = 0.25
            a.set_k_channel_scale(dev(kscale)); b.set_k_channel_scale(dev(kscale))
        stored = (lambda k: k) if kscale is None else (lambda k: (k.astype(np.float32) / kscale[:, None]).astype(np.float16))     # k [L][n][H][D]
        ids_a, ids_b, prompts, accept = [1, 2, 3], [11, 12, 13], [37, 63, 22], [1, 2, 3]
        S, keep = 4, []
        k_new, v_new = rnd(3, S, L, H, D), rnd(3, S, L, H, D)
        k2, v2 = rnd(3, 2, L, H, D), rnd(3, 2, L, H, D)
        chain, held_a, held_b = {}, {}, {}                                          # rows as stored, [L][n][H][D] per kind
        for i, (ra, rb, n) in enumerate(zip(ids_a, ids_b, prompts)):
            a.add_request(ra); b.add_request(rb)
            k, v = rnd(L, n, H, D), rnd(L, n, H, D)
            keep += a.write_prefill(ra, dev(k), dev(v)) + b.write_prefill(rb, dev(k), dev(v))
            chain[ra] = (stored(np.concatenate([k, k_new[i].transpose(1, 0, 2, 3)], axis=1)), np.concatenate([v, v_new[i].transpose(1, 0, 2, 3)], axis=1))
            m = accept[i]
            held_b[rb] = tuple(np.concatenate([c[:, :n + m], x], axis=1) for c, x in zip(chain[ra], (stored(k2[i].transpose(1, 0, 2, 3)), v2[i].transpose(1, 0, 2, 3))))
            held_a[ra] = tuple(x.copy() for x in held_b[rb])
        keep += a.commit(ids_a, dev(k_new), dev(v_new), [list(range(S))] * 3)      # optimistic: the whole chain
        a.truncate(ids_a, [n + m for n, m in zip(prompts, accept)])                 # the accept counts arrive
        keep += b.append_tokens(ids_b, dev(k_new), dev(v_new), accept)
        torch.cuda.synchronize()
        read_back = 0
        for ra, rb, n, m in zip(ids_a, ids_b, prompts, accept):
            ln = n + m
            assert a.length(ra) == b.length(rb) == ln
            assert (a.requests[ra].tail_k is None) == (b.requests[rb].tail_k is None) == (ln % 2 == 0)
            if not ln & 1:
                continue
            read_back += 1
            for kind, name in ((0, "tail_k"), (1, "tail_v")):
                ta, tb = getattr(a.requests[ra], name).cpu().numpy(), getattr(b.requests[rb], name).cpu().numpy()      # [L][H][D]
                rows = chain[ra][kind]
                assert np.array_equal(tb.view(np.uint16), rows[:, ln - 1].view(np.uint16)), (scheme, prescale, rb, name, "the twin holds the row as given")
                pages = np.ascontiguousarray(rows[:, ln - 1:ln + 1]).reshape(L, 2 * H * D)                                 # the pair commit() stored, per layer
                sc, lens, recs = oracle.compress_blocks_f16(pages, SCHEMES[scheme], 0)
                once = oracle.decompress_blocks_f16(recs, lens, sc, SCHEMES[scheme], 0).reshape(L, 2, H, D)[:, 0]
                assert np.array_equal(ta.view(np.uint16), np.ascontiguousarray(once).view(np.uint16)), (scheme, prescale, ra, name, "the row through the format once")
                held_a[ra][kind][:, ln - 1] = ta                                    # what the reopened pair is encoded from
        assert read_back == 2
        keep += a.append_tokens(ids_a, dev(k2), dev(v2), [2, 2, 2])
        keep += b.append_tokens(ids_b, dev(k2), dev(v2), [2, 2, 2])
        torch.cuda.synchronize()
        for ra, rb, n, m in zip(ids_a, ids_b, prompts, accept):
            ln = n + m
            assert a.length(ra) == b.length(rb) == ln + 2
            assert (a.requests[ra].tail_k is None) == (b.requests[rb].tail_k is None) == (ln % 2 == 0)
            if ln & 1:
                assert torch.equal(a.requests[ra].tail_k.view(torch.int16), b.requests[rb].tail_k.view(torch.int16))
                assert torch.equal(a.requests[ra].tail_v.view(torch.int16), b.requests[rb].tail_v.view(torch.int16))
            cut = ln - 1 if ln & 1 else ln + 2                                       # first position of the pair that was written again
            for layer in range(L):
                for kind in (0, 1):
                    ra_rows, rb_rows = a.kv_rows(ra, layer, kind), b.kv_rows(rb, layer, kind)
                    assert torch.equal(ra_rows[:cut].view(torch.int16), rb_rows[:cut].view(torch.int16)), (scheme, ra, layer, kind)
        for layer in range(L):
            _check_attend(oracle, torch, a, scheme, ids_a, held_a, layer, rng, f"rolled back and continued, prescale {prescale}, layer {layer}", kscale)
            _check_attend(oracle, torch, b, scheme, ids_b, held_b, layer, rng, f"twin, prescale {prescale}, layer {layer}", kscale)
    finally:
        lib.finalize()


def test_truncate_is_one_launch():
    """a batch of 6 with every case mixed issues exactly one read_pairs call; a cut that needs no row back issues none"""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, "fp8")
        rng = np.random.default_rng(3)
        rids, lengths = [1, 2, 3, 4, 5, 6], [33, 33, 34, 8, 9, 6]
        keep = []
        for rid, n in zip(rids, lengths):
            keep += _grow(conn, torch, rid, rng.standard_normal((L, n, H, D)).astype(np.float16), rng.standard_normal((L, n, H, D)).astype(np.float16))
        calls = []
        inner = lib.read_pairs
        def counted(handles, *args):
            calls.append(len(handles))
            return inner(handles, *args)
        lib.read_pairs = counted
        conn.truncate(rids, [32, 31, 33, 8, 9, 3])                    # drop, read, read, nothing, nothing, read
        assert calls == [3]
        assert [conn.length(r) for r in rids] == [32, 31, 33, 8, 9, 3]
        conn.truncate(rids, [30, 31, 32, 8, 8, 2])                    # even cuts and dropped tails only
        assert calls == [3]
        assert [conn.length(r) for r in rids] == [30, 31, 32, 8, 8, 2]
        assert [conn.requests[r].tail_k is not None for r in rids] == [False, True, False, False, False, False]
        with pytest.raises(ValueError):
            conn.truncate(rids, [30, 32, 32, 8, 8, 2])
        torch.cuda.synchronize()
    finally:
        lib.finalize()


def test_spec_rollback_example_runs():
    """examples/spec_rollback_example.py end to end on the MI355X, as a child process of its own"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "spec_rollback_example.py"), "--steps", "5"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ok:" in out.stdout
