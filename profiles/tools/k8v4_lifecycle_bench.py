#!/usr/bin/env python3
"""The split pool's fork and rollback launches against the routes there were before them, and against an FP8 pool.

(a) fork: speckv_ext_copy_runs_kv (ONE call, one launch over the FP8_E4M3 and the MXFP4 allocation of every request) against
    speckv_ext_copy_runs called once on the K handles and once on the V handles, and (c) against speckv_ext_copy_runs on an FP8 pool of the
    same shape (K and V in one allocation; the split pool holds 0.77 of its record bytes).  Shapes: 64 requests x 8k positions and 8 x 32k,
    8 layers, every stored pair copied into destinations allocated beforehand.
(b) rollback: speckv_ext_read_pairs_kv (ONE call: the even half of one page per layer and allocation, 256 requests) against two
    speckv_ext_read_pairs calls that address the single-kind allocations with commit's n_layers = L / 2 trick, and (c) against
    speckv_ext_read_pairs on the FP8 pool.

All routes of a case run in one process on one stream, in turn, after a warm-up of every route.  HIP events around a route give the device
side as the stream sees it (host gaps between two calls of a route included), a host clock around the same calls the host side.  Reported:
the median of `rounds` medians of `reps`, the lowest and highest of those medians as the spread, and the ratios.  A difference counts only
where the spreads do not overlap; the tool says which do.

    python profiles/tools/k8v4_lifecycle_bench.py [--layers 8] [--reps 5] [--rounds 5] [--shapes 64x8192,8x32768] [--cut-requests 256] [--cut-context 2048]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

H, D = 8, 128
K_REC, V_REC = 2048, 1088                        # record bytes of a page: FP8_E4M3, MXFP4


def measure(torch, st, routes, reps, rounds):
    """routes [(name, fn)] in turn -> {name: (device median ms, lowest median, highest median, host median ms)}"""
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        fn()
        e1.record(st)
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), host
    for _, fn in routes:                                        # warm-up: staging ring, clocks, the destinations' first records
        timed(fn); timed(fn)
    dev, host = {n: [] for n, _ in routes}, {n: [] for n, _ in routes}
    for _ in range(rounds):
        d, h = {n: [] for n, _ in routes}, {n: [] for n, _ in routes}
        for _ in range(reps):
            for name, fn in routes:
                x, y = timed(fn)
                d[name].append(x); h[name].append(y)
        for name, _ in routes:
            dev[name].append(statistics.median(d[name])); host[name].append(statistics.median(h[name]))
    return {n: (statistics.median(dev[n]), min(dev[n]), max(dev[n]), statistics.median(host[n])) for n, _ in routes}


def compare(res, a, b, what):
    (ma, la, ha, _), (mb, lb, hb, _) = res[a], res[b]
    apart = ha < lb or hb < la
    print(f"  {what}: {a} / {b} = {ma / mb:.3f} ({'the spreads do not overlap' if apart else 'WITHIN the spreads: no difference shown'})")


def report(res):
    for name, (m, lo, hi, host) in res.items():
        print(f"  {name:34s} device {m:9.3f} ms (medians {lo:.3f} .. {hi:.3f}), host {host:9.3f} ms")


def pools(lib, L, T, B, torch):
    """a split connector and an FP8 connector with B prefilled sources and B empty destinations each"""
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector
    split, fp8 = SpeckvSplitKVConnector(lib, L, H, D, T), SpeckvKVConnector(lib, L, H, D, T, "fp8")
    k, v = torch.randn((L, T, H, D), device="cuda").half(), torch.randn((L, T, H, D), device="cuda").half()
    for conn in (split, fp8):
        for rid in range(B):
            conn.add_request(rid)
            conn.write_prefill(rid, k, v)
            conn.add_request(1000 + rid)
        torch.cuda.synchronize()
    return split, fp8


def fork_case(B, T, a):
    import torch
    import cxl_speckv_amd as pkg
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        L = a.layers
        split, fp8 = pools(lib, L, T, B, torch)
        st = torch.cuda.Stream()
        u64 = lambda xs: np.asarray(list(xs), dtype=np.uint64)
        src, dst = [split.requests[r] for r in range(B)], [split.requests[1000 + r] for r in range(B)]
        ks, vs, kd, vd = (u64(r.k_handle for r in src), u64(r.v_handle for r in src), u64(r.k_handle for r in dst), u64(r.v_handle for r in dst))
        fs, fd = u64(fp8.requests[r].handle for r in range(B)), u64(fp8.requests[1000 + r].handle for r in range(B))
        n_pages = u64([T // 2] * B)
        firsts, firsts_fp8 = u64(l * (T // 2) for l in range(L)), u64(j * (T // 2) for j in range(2 * L))

        def one():
            lib.copy_runs_kv(ks, vs, kd, vd, n_pages, firsts, st.cuda_stream)

        def two():
            lib.copy_runs(ks, kd, n_pages, firsts, st.cuda_stream)
            lib.copy_runs(vs, vd, n_pages, firsts, st.cuda_stream)

        def pool8():
            lib.copy_runs(fs, fd, n_pages, firsts_fp8, st.cuda_stream)

        res = measure(torch, st, [("copy_runs_kv, one call", one), ("copy_runs on K, then on V", two), ("copy_runs, FP8 pool", pool8)], a.reps, a.rounds)
        pages = B * L * (T // 2)
        moved, moved8 = 2 * pages * (K_REC + V_REC), 2 * pages * 2 * K_REC
        print(f"fork: {B} requests x {T} positions x {L} layers; split pool {moved / 1e9:.2f} GB read + written, FP8 pool {moved8 / 1e9:.2f} GB")
        report(res)
        compare(res, "copy_runs_kv, one call", "copy_runs on K, then on V", "(a) one launch against two calls")
        compare(res, "copy_runs_kv, one call", "copy_runs, FP8 pool", f"(c) split pool against FP8 pool (bytes {moved / moved8:.2f})")
        m, m8 = res["copy_runs_kv, one call"][0], res["copy_runs, FP8 pool"][0]
        print(f"  per byte: split {moved / (m * 1e-3) / 1e12:.2f} TB/s, FP8 pool {moved8 / (m8 * 1e-3) / 1e12:.2f} TB/s over the whole call")
    finally:
        lib.finalize()


def cut_case(a):
    import torch
    import cxl_speckv_amd as pkg
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        L, T, B = a.layers, a.cut_context, a.cut_requests
        split, fp8 = pools(lib, L, T, B, torch)
        st = torch.cuda.Stream()
        u64 = lambda xs: np.asarray(list(xs), dtype=np.uint64)
        reqs = [split.requests[r] for r in range(B)]
        ks, vs, fh = u64(r.k_handle for r in reqs), u64(r.v_handle for r in reqs), u64(fp8.requests[r].handle for r in range(B))
        layer_bytes = H * D * 2
        tk = torch.empty((B, L, H, D), dtype=torch.float16, device="cuda")
        tv = torch.empty_like(tk)
        pages = u64((T - 2 * (1 + r % 7) - 1) // 2 for r in range(B))                # cut to odd lengths: the even half of a stored page each
        at = np.arange(B, dtype=np.uint64) * np.uint64(L * layer_bytes)
        rows = np.zeros((B, 4), dtype=np.uint64)
        rows[:, 0], rows[:, 2] = at + np.uint64(tk.data_ptr()), at + np.uint64(tv.data_ptr())
        # a single-kind allocation through read_pairs: the rows of real layer 0 in the "K" slots, of real layer 1 in the "V" slots
        rows_k, rows_v = np.zeros((B, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
        rows_k[:, 0], rows_k[:, 2] = rows[:, 0], rows[:, 0] + np.uint64(layer_bytes)
        rows_v[:, 0], rows_v[:, 2] = rows[:, 2], rows[:, 2] + np.uint64(layer_bytes)

        def one():
            lib.read_pairs_kv(ks, vs, pages, rows, T // 2, L, layer_bytes, st.cuda_stream)

        def two():
            lib.read_pairs(ks, pages, rows_k, T // 2, L // 2, 2 * layer_bytes, st.cuda_stream)
            lib.read_pairs(vs, pages, rows_v, T // 2, L // 2, 2 * layer_bytes, st.cuda_stream)

        def pool8():
            lib.read_pairs(fh, pages, rows, T // 2, L, layer_bytes, st.cuda_stream)

        one(); torch.cuda.synchronize()
        a1, b1 = tk.clone(), tv.clone()
        tk.zero_(); tv.zero_()
        two(); torch.cuda.synchronize()
        assert torch.equal(a1, tk) and torch.equal(b1, tv), "the two routes must read the same rows"
        res = measure(torch, st, [("read_pairs_kv, one call", one), ("read_pairs on K, then on V", two), ("read_pairs, FP8 pool", pool8)], a.reps, a.rounds)
        print(f"truncate: {B} requests x {T} positions x {L} layers cut to odd lengths, {B * 2 * L} pages decoded, {B * 2 * L * 2048 / 1e6:.1f} MB of rows written")
        report(res)
        compare(res, "read_pairs_kv, one call", "read_pairs on K, then on V", "(b) one launch against two calls")
        compare(res, "read_pairs_kv, one call", "read_pairs, FP8 pool", "(c) split pool against FP8 pool")
    finally:
        lib.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="64x8192,8x32768")
    ap.add_argument("--cut-requests", type=int, default=256)
    ap.add_argument("--cut-context", type=int, default=2048)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        B, T = (int(x) for x in shape.split("x"))
        fork_case(B, T, a)
    cut_case(a)


if __name__ == "__main__":
    main()
