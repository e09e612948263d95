#!/usr/bin/env python3
"""fork() of a batch against the only route without speckv_ext_copy_runs: kv_rows of every region plus write_prefill.

256 requests x 8 layers x 2k positions, every request forked at full length, for FP8, INT4_G32 and MXFP4.  Both routes in one
process, alternating; HIP events around each route on one stream give the device side as the stream sees it (the host's work
between two launches included: 256 allocations on either route), events around the speckv_ext_copy_runs call the copy launch alone,
a host clock around the same calls (before the stream is waited for) the host side.  The new requests of a repetition are freed
before the next one.  Reported: the median of five medians of five, the ratio of the two routes, and the copy launch as a fraction
of the 8 TB/s roofline over the record bytes read plus written (the kernel's own duration: rocprofv3 --kernel-trace --stats over
this tool, profiles/fork_step.txt).

    python profiles/tools/fork_bench.py [--requests 256] [--layers 8] [--context 2048] [--schemes fp8,int4,mxfp4] [--reps 5] [--rounds 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REC_BYTES = {"fp8": 2048, "int4": 1152, "mxfp4": 1088}


def bench(scheme, a):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, L, T, B = 8, 128, a.layers, a.context, a.requests
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        ids, new_ids = list(range(1, B + 1)), list(range(10001, 10001 + B))
        k, v = torch.randn((L, T, H, D), device="cuda").half(), torch.randn((L, T, H, D), device="cuda").half()
        for rid in ids:
            conn.add_request(rid)
            conn.write_prefill(rid, k, v)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()

        launches = []                                           # events around the copy launch itself, inside fork()
        copy_runs = lib.copy_runs

        def timed_copy_runs(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            copy_runs(*args)
            e1.record(st)
            launches.append((e0, e1))
        lib.copy_runs = timed_copy_runs

        def fork():
            return conn.fork(ids, new_ids, stream=st)

        def round_trip():
            keep = []
            for rid, new in zip(ids, new_ids):
                kk = torch.stack([conn.kv_rows(rid, layer, 0) for layer in range(L)])
                vv = torch.stack([conn.kv_rows(rid, layer, 1) for layer in range(L)])
                conn.add_request(new)
                keep += conn.write_prefill(new, kk, vv, stream=st)
            return keep

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(st)
            with torch.cuda.stream(st):
                keep = fn()
            e1.record(st)
            host = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            del keep
            for new in new_ids:
                conn.free_request(new)
            return e0.elapsed_time(e1), host

        routes = (("fork", fork), ("round trip", round_trip))
        for _, fn in routes:                                    # warm-up: allocator, staging ring, clocks
            timed(fn)
        dev = {name: [] for name, _ in routes}
        host = {name: [] for name, _ in routes}
        for _ in range(a.rounds):
            d = {name: [] for name, _ in routes}
            h = {name: [] for name, _ in routes}
            for _ in range(a.reps):
                for name, fn in routes:                         # alternating
                    x, y = timed(fn)
                    d[name].append(x); h[name].append(y)
            for name, _ in routes:
                dev[name].append(statistics.median(d[name])); host[name].append(statistics.median(h[name]))
        m = {name: statistics.median(dev[name]) for name, _ in routes}
        launch = [e0.elapsed_time(e1) for e0, e1 in launches[1:]]                   # (the first belongs to the warm-up)
        copy_ms = statistics.median([statistics.median(launch[i:i + a.reps]) for i in range(0, len(launch), a.reps)])
        pages = B * 2 * L * (T // 2)
        moved = 2 * pages * REC_BYTES[scheme]
        print(f"{scheme}: {B} requests x {L} layers x {T} positions, {pages} records of {REC_BYTES[scheme]} B")
        for name, _ in routes:
            print(f"  {name:10s} device {m[name]:9.3f} ms (medians {min(dev[name]):.3f} .. {max(dev[name]):.3f}), host {statistics.median(host[name]):9.3f} ms")
        print(f"  round trip / fork, events around the whole route: {m['round trip'] / m['fork']:.1f}x")
        print(f"  the copy launch alone (events around speckv_ext_copy_runs): {copy_ms:.3f} ms = {m['round trip'] / copy_ms:.1f}x under the round trip; "
              f"{moved / 1e9:.2f} GB read + written: {moved / (copy_ms * 1e-3) / 1e12:.2f} TB/s = {moved / (copy_ms * 1e-3) / 8e12:.2f} of the 8 TB/s roofline")
    finally:
        lib.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for scheme in a.schemes.split(","):
        bench(scheme, a)


if __name__ == "__main__":
    main()
