#!/usr/bin/env python3
"""truncate() of a batch against the route without speckv_ext_read_pairs: kv_rows per (request, layer, kind) for the same rows.

256 requests x 8 layers x 2k context (FP8 pool), every request cut from 2048 to 2047 positions: each needs position 2046 back for
every layer, K and V.  Both routes in one process, HIP events around each, after a warm-up; the cut is undone between repetitions
by putting the request's length back (the pool is never changed by either route).

    python profiles/tools/rollback_step.py [--requests 256] [--layers 8] [--context 2048] [--scheme fp8] [--reps 7]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--scheme", default="fp8")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, L, T, B = 8, 128, a.layers, a.context, a.requests
        conn = SpeckvKVConnector(lib, L, H, D, T, a.scheme)
        ids = list(range(1, B + 1))
        k, v = torch.randn((L, T, H, D), device="cuda").half(), torch.randn((L, T, H, D), device="cuda").half()
        for rid in ids:
            conn.add_request(rid)
            conn.write_prefill(rid, k, v)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()

        def restore():
            for rid in ids:
                r = conn.requests[rid]
                r.length = T
                r.clear_tail()

        def one_launch():
            conn.truncate(ids, [T - 1] * B, stream=st)

        def per_row():
            rows = []
            for rid in ids:
                for layer in range(L):
                    for kind in (0, 1):
                        rows.append(conn.kv_rows(rid, layer, kind, T - 2, T - 1))
            return rows

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            with torch.cuda.stream(st):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        res = {}
        for name, fn in (("truncate (one read_pairs launch)", one_launch), ("kv_rows per (request, layer, kind)", per_row)):
            for _ in range(3):                                  # warm-up: allocator, staging ring, clocks
                timed(fn); restore()
            ms = []
            for _ in range(a.reps):
                ms.append(timed(fn)); restore()
            res[name] = ms
            print(f"{name}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} over {a.reps} repetitions "
                  f"({B} requests x {L} layers x {T} positions, {a.scheme})")
        m = [statistics.median(x) for x in res.values()]
        print(f"ratio {m[1] / m[0]:.1f}x")
    finally:
        lib.finalize()


if __name__ == "__main__":
    main()
