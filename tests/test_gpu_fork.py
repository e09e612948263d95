"""-m gpu: forking requests -- speckv_ext_copy_runs (one launch copies the stored records of page runs from allocation to allocation,
nothing decoded) and SpeckvKVConnector.fork on top of it.

References: the source allocation itself.  A copied page must give the bits of the source's page through every reader
(speckv_ext_fetch_range, the attention entries); a forked request must be the request a caller would have written independently
(a twin built by write_prefill / commit / truncate of the same values), bit for bit."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import D, H, torch_mod
from tests.test_gpu_round2 import open_lib

pytestmark = pytest.mark.gpu
PAGE, ROW = 4096, 2048
L, T = 2, 128
STEP = T // 2                                   # pages of one (layer, kind) region
N_PAGES = 2 * L * STEP
HOLES = (8, 40)                                 # pages of every region that the source never writes
COUNTS = [0, 1, 15, 16, 17, 64]                 # pages per run: MXFP4 tile rows 15 / 16 / 17, and a whole region
u64 = lambda *v: np.asarray(v, dtype=np.uint64)


def _blocks(n, seed):
    """fp16 page images: random, a few that compress (constant runs, zeros)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ROW)).astype(np.float16)
    x[3] = 0
    x[5] = np.repeat(x[5, :64], 32)
    x[15, 1024:] = x[15, 1024]
    x[STEP + 16] = x[STEP + 16, 7]
    return x


def _fill(lib, h, x, holes=HOLES):
    """every page of the allocation from x, except the pages `holes` of every (layer, kind) region"""
    for j in range(2 * L):
        edges = [-1] + list(holes) + [STEP]
        for a, b in zip(edges, edges[1:]):
            lo, hi = j * STEP + a + 1, j * STEP + b
            if hi > lo:
                part = np.ascontiguousarray(x[lo:hi])
                lib.write(h, lo * PAGE, part.ctypes.data, part.nbytes, False)


def _image(lib, torch, h, stream):
    out = torch.empty((N_PAGES, ROW), dtype=torch.float16, device="cuda")
    lib.fetch_range(h, 0, N_PAGES, out.data_ptr(), False, stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy().view(np.uint16)


def _infos(lib, h, pages):
    return {p: lib.translate(h, p * PAGE) for p in pages}


def _check_copy(lib, torch, scheme, src, dsts, counts, runs, what, same_slots=True):
    """copy_runs(src -> every dst, counts[i] pages of the runs `runs`) in ONE call.  Afterwards a copied page decodes (fetch_range)
    to the bits of the source's page and reports its rec_bytes and scale (MXFP4: the destination's own code offset stays); every
    other page of the destination is what it was before (a fresh allocation: zeros, rec_bytes 0).  same_slots: the destination's
    records stay where they lay (not so for a sealed destination, which is unpacked)."""
    st = torch.cuda.Stream()
    probe = [r + p for r in (0, STEP) for p in range(STEP)]               # translate is a synchronous call: two regions of four
    want = _image(lib, torch, src, st)
    want_info = _infos(lib, src, probe)
    for hole in HOLES:
        assert not want[hole].any() and want_info[hole].rec_bytes == 0, (what, "a page never written decodes to zeros")
    assert want[0].any() and want[17].any()
    before = [(_image(lib, torch, d, st), _infos(lib, d, probe)) for d in dsts]
    copied = lib.stats().copied_pages
    lib.copy_runs(u64(*[src] * len(dsts)), u64(*dsts), u64(*counts), u64(*runs), st.cuda_stream)
    st.synchronize()
    assert lib.stats().copied_pages == copied + len(runs) * sum(counts)
    for d, n, (old, old_info) in zip(dsts, counts, before):
        got = _image(lib, torch, d, st)
        info = _infos(lib, d, probe)
        inside = np.zeros(N_PAGES, dtype=bool)
        for r in runs:
            inside[r:r + n] = True
        assert np.array_equal(got[inside], want[inside]), (what, n, "copied pages")
        assert np.array_equal(got[~inside], old[~inside]), (what, n, "pages beyond n_pages and pages of runs not named")
        for p in probe:
            ref = want_info[p] if inside[p] else old_info[p]
            assert info[p].rec_bytes == ref.rec_bytes, (what, n, p)
            if scheme != 5:
                assert np.float32(info[p].scale).view(np.uint32) == np.float32(ref.scale).view(np.uint32), (what, n, p)
            if same_slots:
                assert info[p].aux_offset == old_info[p].aux_offset and info[p].pool_addr == old_info[p].pool_addr, (what, n, p, "the slot is the destination's own")
    return want


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4, 5])
def test_copy_runs_copies_records_bit_for_bit(scheme, mode):
    """Every scheme in both quantiser modes.  One source into six destinations in ONE call, 0 / 1 / 15 / 16 / 17 / 64 pages of runs
    0 and 2 of the four regions (runs 1 and 3 are not named), two pages of every region never written.  Placements: everything in
    one run; INT8_DELTA_RLE with the source sealed (it stays sealed) and with the destination sealed (it is unpacked; it held other
    records before, which stay where nothing is copied and go where a page never written is); two pools of the one GPU with the
    source striped and pages 15..17 migrated, and with the DESTINATION's pages 15..17 migrated instead (for MXFP4 the code rows of
    source and destination then lie at different distances from their nibble rows)."""
    torch = torch_mod()
    x, y = _blocks(N_PAGES, 300 + scheme), _blocks(N_PAGES, 400 + scheme)[::-1]
    runs = [0, 2 * STEP]
    lib = open_lib()
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        src = lib.alloc(N_PAGES * PAGE)
        _fill(lib, src, x)
        dsts = [lib.alloc(N_PAGES * PAGE) for _ in COUNTS]
        _check_copy(lib, torch, scheme, src, dsts, COUNTS, runs, ("one run", scheme, mode))
        _check_copy(lib, torch, scheme, dsts[5], dsts[:3], [64, 17, 3], [STEP, 3 * STEP, 0], ("a copy of a copy, three runs", scheme, mode))
        if scheme == 2:
            lib.compact(src)
            sealed = lib.stats().sealed_allocations
            assert sealed == 1
            fresh = [lib.alloc(N_PAGES * PAGE) for _ in range(3)]
            _check_copy(lib, torch, scheme, src, fresh, [17, 64, 1], runs, ("sealed source", mode))
            assert lib.stats().sealed_allocations == sealed, "a sealed source stays sealed"
            full = lib.alloc(N_PAGES * PAGE)
            _fill(lib, full, y, holes=())
            lib.compact(full)
            assert lib.stats().sealed_allocations == sealed + 1
            _check_copy(lib, torch, scheme, src, [full], [17], runs, ("sealed destination", mode), same_slots=False)
            assert lib.stats().sealed_allocations == sealed, "a sealed destination is unpacked first"
    finally:
        lib.finalize()
    lib = open_lib(SPECKV_POOL_DEVICES="0,0")
    try:
        lib.set_quant_mode(mode)
        lib.set_compression_scheme(scheme)
        src = lib.alloc(N_PAGES * PAGE)
        _fill(lib, src, x)
        lib.migrate(src, 15, 3, 1)                                    # pages 15..17 now lie in pool 1, wherever they lay
        lib.migrate(src, 2 * STEP, 1, 0)
        dsts = [lib.alloc(N_PAGES * PAGE) for _ in COUNTS]
        _check_copy(lib, torch, scheme, src, dsts, COUNTS, runs, ("striped, source migrated", scheme, mode))
        plain = lib.alloc(N_PAGES * PAGE)
        _fill(lib, plain, x)
        moved = [lib.alloc(N_PAGES * PAGE) for _ in range(2)]
        for d in moved:
            _fill(lib, d, y, holes=())
            lib.migrate(d, 15, 3, 1)
            lib.migrate(d, 2 * STEP, 1, 0)
        _check_copy(lib, torch, scheme, plain, moved, [64, 17], runs, ("striped, destination migrated", scheme, mode))
    finally:
        lib.finalize()


def test_copy_runs_refuses_bad_arguments_and_launches_nothing():
    """every SPECKV_ERR_INVAL and SPECKV_ERR_GENERAL case of the header; after each refusal the destinations still decode to zeros;
    the calls with nothing to do succeed and do nothing; then the good call copies"""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(4)
        a, b, c = (lib.alloc(N_PAGES * PAGE) for _ in range(3))
        x = _blocks(N_PAGES, 7)
        lib.write(a, 0, x.ctypes.data, x.nbytes, False)
        lib.set_compression_scheme(3)
        other = lib.alloc(N_PAGES * PAGE)
        st = torch.cuda.Stream()
        s = st.cuda_stream
        runs = u64(0, STEP)
        inval = [
            dict(stream=0),                                            # NULL stream
            dict(dst=u64(other)),                                      # allocations of different schemes
            dict(src=u64(a, other), dst=u64(b, c), n=u64(4, 4)),
            dict(dst=u64(a)),                                          # src[i] == dst[i]
            dict(src=u64(a, b), dst=u64(c, b), n=u64(4, 0)),           # ... in a pair without pages too
            dict(src=u64(a, a), dst=u64(b, b), n=u64(4, 4)),           # two pairs share a destination page
            dict(src=u64(a, b), dst=u64(b, c), n=u64(4, 4)),           # a destination that is also a source
            dict(runs=u64(0, 15)),                                     # runs that overlap
            dict(runs=u64(STEP, 0, STEP)),
        ]
        general = [
            dict(src=u64(a + 12345)),                                  # an unknown handle
            dict(dst=u64(b + 12345)),
            dict(runs=u64(0, N_PAGES - 15)),                           # pages that leave the allocations
            dict(runs=u64(0), n=u64(N_PAGES + 1)),
            dict(runs=u64(0, 2 ** 64 - 8)),
        ]
        def zeros():
            for h in (b, c):
                assert not _image(lib, torch, h, st).any(), "a refused call wrote to its destination"
        for status, cases in ((-4, inval), (-1, general)):
            for case in cases:
                arg = dict(src=u64(a), dst=u64(b), n=u64(16), runs=runs, stream=s)
                arg.update(case)
                with pytest.raises(SpeckvError) as e:
                    lib.copy_runs(arg["src"], arg["dst"], arg["n"], arg["runs"], arg["stream"])
                assert e.value.status == status, (case, e.value.status)
                zeros()
        for name in ("src", "dst", "n", "runs"):                      # NULL arrays
            args = dict(src=u64(a).ctypes.data, dst=u64(b).ctypes.data, n=u64(16).ctypes.data, runs=runs.ctypes.data)
            args[name] = None
            with pytest.raises(SpeckvError) as e:
                lib._ext("speckv_ext_copy_runs", args["src"], args["dst"], args["n"], 1, args["runs"], 2, s)
            assert e.value.status == -4, name
        copied = lib.stats().copied_pages
        lib.copy_runs(u64(), u64(), u64(), runs, s)                   # no pairs: nothing to do, fine
        lib.copy_runs(u64(a), u64(b), u64(16), u64(), s)              # no runs
        lib.copy_runs(u64(a, a), u64(b, c), u64(0, 0), runs, s)       # no pages
        zeros()
        assert lib.stats().copied_pages == copied
        lib.copy_runs(u64(a, a), u64(b, c), u64(16, 0), runs, s)      # ... and the good call copies
        st.synchronize()
        src, got = _image(lib, torch, a, st), _image(lib, torch, b, st)
        assert np.array_equal(got[:16], src[:16]) and np.array_equal(got[STEP:STEP + 16], src[STEP:STEP + 16]) and got[:16].any()
        assert not got[16:STEP].any() and not got[STEP + 16:].any() and not _image(lib, torch, c, st).any()
        assert lib.stats().copied_pages == copied + 32
    finally:
        lib.finalize()


# --------------------------------------------------------------------------------------------------------------- the connector
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(rng, *shape):
    return rng.standard_normal(shape).astype(np.float16)


def _prefill(conn, torch, rid, k, v):
    """a fresh request holding k / v [L][n][H][D] (host fp16), written by write_prefill"""
    conn.add_request(rid)
    keep = conn.write_prefill(rid, _dev(torch, k), _dev(torch, v)) if k.shape[1] else []
    torch.cuda.synchronize()
    return keep


def _all_rows(conn, rid):
    """kv_rows of every layer and kind, as bits"""
    return [conn.kv_rows(rid, layer, kind).cpu().numpy().view(np.uint16) for layer in range(L) for kind in (0, 1)]


def _tails(conn, rid):
    r = conn.requests[rid]
    return None if r.tail_k is None else (r.tail_k.cpu().numpy().view(np.uint16), r.tail_v.cpu().numpy().view(np.uint16))


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("scheme,prescale,pools", [("fp8", False, None), ("int4", False, None), ("mxfp4", False, None), ("int4", True, None),
                                                   ("fp8", True, None), ("fp8", False, "0,0")])
def test_attention_sees_the_same_records(scheme, prescale, pools):
    """Requests of 31, 32, 33 and 96 positions forked at full length.  attend() over the sources twice gives identical bits, and
    attend() over the forks -- the same batch shape -- gives those bits; the same for attend_spec with S = 4.  That is the FP8
    scale tables (page order, and run order over two pools) and the MXFP4 planes through the forms small batches select; once with
    a K pre-scale; FP8 over two pools of the one GPU, where a table or class form is taken."""
    torch = torch_mod()
    lib = open_lib(SPECKV_POOL_DEVICES=pools) if pools else pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(17)
        if prescale:
            kscale = np.ones((L, H, D), np.float32)
            kscale[:, :, 0::8] = 4.0; kscale[:, :, 3::8] = 0.25
            conn.set_k_channel_scale(_dev(torch, kscale))
        lengths = [31, 32, 33, 96]
        srcs, forks, keep = [1, 2, 3, 4], [11, 12, 13, 14], []
        for rid, n in zip(srcs, lengths):
            keep += _prefill(conn, torch, rid, _rows(rng, L, n, H, D), _rows(rng, L, n, H, D))
        keep += conn.fork(srcs, forks)
        torch.cuda.synchronize()
        assert [conn.length(r) for r in forks] == lengths
        G, S, sm = 4, 4, 1.0 / np.sqrt(D)
        for layer in range(L):
            q = _dev(torch, _rows(rng, len(srcs), H, G, D))
            first = conn.attend(layer, srcs, q, sm).cpu().numpy()
            again = conn.attend(layer, srcs, q, sm).cpu().numpy()
            assert np.all(np.isfinite(first)) and first.any()
            assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), (scheme, layer, "attend is not repeatable: nothing can be said")
            got = conn.attend(layer, forks, q, sm).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), (scheme, prescale, pools, layer, "attend over the forks")
            q = _dev(torch, _rows(rng, len(srcs), S, H, G, D))
            k_new, v_new = _dev(torch, _rows(rng, len(srcs), S, L, H, D)), _dev(torch, _rows(rng, len(srcs), S, L, H, D))
            first = conn.attend_spec(layer, srcs, q, k_new, v_new, sm).cpu().numpy()
            again = conn.attend_spec(layer, srcs, q, k_new, v_new, sm).cpu().numpy()
            assert np.all(np.isfinite(first)) and first.any()
            assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), (scheme, layer, "attend_spec is not repeatable: nothing can be said")
            got = conn.attend_spec(layer, forks, q, k_new, v_new, sm).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), (scheme, prescale, pools, layer, "attend_spec over the forks")
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_source_and_fork_diverge(scheme):
    """A request of 33 positions (the shared last pair is encoded again on both sides) and one of 32, each forked; then 3 different
    positions are committed to the fork and 3 others to the source.  Each request equals, bit for bit over kv_rows of all layers, a
    twin built by write_prefill + commit of the same values in a fresh request; neither commit changes the other side; freeing
    the source leaves the fork readable."""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(29)
        S, keep = 3, []
        for n, base in ((33, 100), (32, 200)):
            src, fork, twin_src, twin_fork = base + 1, base + 2, base + 3, base + 4
            k, v = _rows(rng, L, n, H, D), _rows(rng, L, n, H, D)
            new = {rid: (_dev(torch, _rows(rng, 1, S, L, H, D)), _dev(torch, _rows(rng, 1, S, L, H, D))) for rid in (src, fork)}
            keep += _prefill(conn, torch, src, k, v)
            keep += conn.fork([src], [fork])
            torch.cuda.synchronize()
            start = _all_rows(conn, src)
            assert _same(_all_rows(conn, fork), start) and conn.length(fork) == n
            keep += conn.commit([fork], *new[fork], [list(range(S))])
            torch.cuda.synchronize()
            assert _same(_all_rows(conn, src), start), (scheme, n, "the fork's commit changed the source")
            fork_rows = _all_rows(conn, fork)
            keep += conn.commit([src], *new[src], [list(range(S))])
            torch.cuda.synchronize()
            assert _same(_all_rows(conn, fork), fork_rows), (scheme, n, "the source's commit changed the fork")
            for rid, twin in ((src, twin_src), (fork, twin_fork)):
                keep += _prefill(conn, torch, twin, k, v)
                keep += conn.commit([twin], *new[rid], [list(range(S))])
                torch.cuda.synchronize()
                assert conn.length(rid) == conn.length(twin) == n + S
                assert _same(_all_rows(conn, rid), _all_rows(conn, twin)), (scheme, n, rid, "not the request written independently")
                a, b = _tails(conn, rid), _tails(conn, twin)
                assert (a is None) == (b is None) == ((n + S) % 2 == 0)
                assert a is None or (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
            assert not _same(_all_rows(conn, src), fork_rows)
            conn.free_request(src)
            assert _same(_all_rows(conn, fork), fork_rows), (scheme, n, "the fork after its source was freed")
    finally:
        lib.finalize()


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_shorter_forks_are_twins_cut_by_truncate(scheme):
    """32 -> 17 (the tail is read out of the source's stored pair), 33 -> 33 (the source's held row), 33 -> 32 and 33 -> 0 as ONE
    batch: exactly one copy_runs and one read_pairs call; length, tail bits and kv_rows of every fork equal those of a twin of the
    source cut with truncate to the same length."""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        rng = np.random.default_rng(31)
        data = {n: (_rows(rng, L, n, H, D), _rows(rng, L, n, H, D)) for n in (32, 33)}
        keep = []
        for n in data:
            keep += _prefill(conn, torch, n, *data[n])
        cases = [(32, 17), (33, 33), (33, 32), (33, 0)]
        forks, twins = [101, 102, 103, 104], [201, 202, 203, 204]
        for twin, (n, _) in zip(twins, cases):
            keep += _prefill(conn, torch, twin, *data[n])
        conn.truncate(twins, [m for _, m in cases])
        before = {n: _all_rows(conn, n) for n in data}
        calls = []
        copy_runs, read_pairs = lib.copy_runs, lib.read_pairs
        lib.copy_runs = lambda *a: (calls.append("copy_runs"), copy_runs(*a))[1]
        lib.read_pairs = lambda *a: (calls.append("read_pairs"), read_pairs(*a))[1]
        keep += conn.fork([n for n, _ in cases], forks, [m for _, m in cases])
        lib.copy_runs, lib.read_pairs = copy_runs, read_pairs
        torch.cuda.synchronize()
        assert sorted(calls) == ["copy_runs", "read_pairs"]
        for fork, twin, (n, m) in zip(forks, twins, cases):
            assert conn.length(fork) == conn.length(twin) == m
            a, b = _tails(conn, fork), _tails(conn, twin)
            assert (a is None) == (b is None) == (m % 2 == 0), (scheme, n, m)
            assert a is None or (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), (scheme, n, m, "tail bits")
            assert _same(_all_rows(conn, fork), _all_rows(conn, twin)), (scheme, n, m)
            assert _all_rows(conn, fork)[0].shape[0] == m
        for n in data:                                                # the sources are what they were
            assert conn.length(n) == n and _same(_all_rows(conn, n), before[n])
    finally:
        lib.finalize()


def test_fork_follows_a_commit_on_the_same_stream():
    """commit and then fork queued on one stream with no synchronisation between them: the fork holds the committed rows"""
    torch = torch_mod()
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        conn = SpeckvKVConnector(lib, L, H, D, T, "fp8")
        rng = np.random.default_rng(37)
        B, n, S = 4, 40, 8
        rids, forks, keep = list(range(1, B + 1)), list(range(11, 11 + B)), []
        for rid in rids:
            keep += _prefill(conn, torch, rid, _rows(rng, L, n, H, D), _rows(rng, L, n, H, D))
        k_new, v_new = _dev(torch, _rows(rng, B, S, L, H, D)), _dev(torch, _rows(rng, B, S, L, H, D))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        keep += conn.commit(rids, k_new, v_new, [list(range(S))] * B, stream=st)
        keep += conn.fork(rids, forks, stream=st)
        st.synchronize()
        for rid, fork in zip(rids, forks):
            assert conn.length(fork) == n + S
            rows = _all_rows(conn, fork)
            assert _same(rows, _all_rows(conn, rid))
            assert all(r[n:].any() for r in rows), "the committed positions are missing from the fork"
    finally:
        lib.finalize()


def test_fork_example_runs():
    """examples/fork_example.py end to end on the MI355X, as a child process of its own"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "fork_example.py"), "--steps", "5"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ok:" in out.stdout
