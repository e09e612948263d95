#!/usr/bin/env python3
"""Paged-cache transfers of the split pool (K8V4) against its row route and against the FP8 pool (profiles/k8v4_paged_io.txt).

Shapes as profiles/paged_io.txt: 4 requests x 8k positions and 1 request x 32k positions, 8 layers; per-layer caches
[2, blocks, 16, 8, 128], fp16 and bf16, every request's positions scattered over blocks by a random block table.  Three routes are
timed in one process, alternating, HIP events on one stream around each call, after a warm-up of every route:
  (a) kv     SpeckvSplitKVConnector.load_paged / store_paged: ONE speckv_ext_read_slots_kv / _write_slots_kv launch over both
             allocations of every request;
  (b) rows   the row route of the same tree: load = kv_rows + index_copy_ per (request, layer, kind); store = index_select per layer
             and kind, torch.stack, write_prefill per request (one speckv_ext_write_runs per allocation);
  (c) fp8    SpeckvKVConnector("fp8").load_paged / store_paged(fused=True) on the same caches and slots: the pool K8V4 is measured
             against (2 x 2048 record bytes per pair and layer where K8V4 has 2048 + 1088).
Reported per route: the median of `rounds` medians of `reps` with the spread of those medians, the library launches counted by a
wrapper around the library object, and for (a) the bytes moved (record bytes plus 4 KiB per page) over the time as a fraction of
8 TB/s; then (a) / (b) and (a) / (c).  A store is timed on fresh requests (allocated before the first event, freed after the last).

    python profiles/tools/k8v4_paged_io_bench.py [--layers 8] [--shapes 4x8192,1x32768] [--elems fp16,bf16] [--reps 5] [--rounds 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = ((4, 8192), (1, 32768))
BS = 16
COUNTED = ("read_slots_kv", "write_slots_kv", "read_slots_ex", "write_slots_ex", "fetch_range", "write_runs")


class Counting:
    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in COUNTED:
            return f

        def counted(*a, **k):
            self.n += 1
            return f(*a, **k)
        return counted


def bench(elem, B, n, a, say):
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        H, D, L = 8, 128, a.layers
        dtype = torch.bfloat16 if elem == "bf16" else torch.float16
        kv, fp8 = SpeckvSplitKVConnector(lib, L, H, D, n), SpeckvKVConnector(lib, L, H, D, n, "fp8")
        blocks = B * n // BS
        caches = [torch.randn((2, blocks, BS, H, D), device="cuda").to(dtype) for _ in range(L)]
        flats = [c.view(2, blocks * BS, H, D) for c in caches]
        table = np.random.default_rng(1).permutation(blocks)
        slots = (table[:, None] * BS + np.arange(BS)[None]).reshape(-1).astype(np.int64)         # request i: slots[i * n : (i + 1) * n]
        d_slots = torch.from_numpy(slots).cuda()
        ids = list(range(1, B + 1))
        st = torch.cuda.Stream()
        for c in (kv, fp8):
            for rid in ids:
                c.add_request(rid)
        keep = kv.store_paged(ids, [n] * B, d_slots, caches, stream=st)
        keep += fp8.store_paged(ids, [n] * B, d_slots, caches, stream=st, fused=True)
        torch.cuda.synchronize()
        del keep
        fresh = iter(range(1000, 10 ** 9))

        def load_kv():
            kv.load_paged(ids, [0] * B, [n] * B, d_slots, caches, stream=st)

        def load_fp8():
            fp8.load_paged(ids, [0] * B, [n] * B, d_slots, caches, stream=st, fused=True)

        def load_rows():
            with torch.cuda.stream(st):
                for i, rid in enumerate(ids):
                    at = d_slots[i * n:(i + 1) * n]
                    for layer, flat in enumerate(flats):
                        for kind in (0, 1):
                            flat[kind].index_copy_(0, at, kv.kv_rows(rid, layer, kind).to(dtype))

        def store_on(conn, **kw):
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    conn.add_request(rid)
                return new

            def run(new):
                return conn.store_paged(new, [n] * B, d_slots, caches, stream=st, **kw)
            return prepare, run, conn

        def store_rows():
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    kv.add_request(rid)
                return new

            def run(new):
                held = []
                with torch.cuda.stream(st):
                    for i, rid in enumerate(new):
                        at = d_slots[i * n:(i + 1) * n]
                        k = torch.stack([f[0].index_select(0, at) for f in flats]).to(torch.float16)      # [layers][tokens][heads][dim]
                        v = torch.stack([f[1].index_select(0, at) for f in flats]).to(torch.float16)
                        held += kv.write_prefill(rid, k, v, st)
                return held
            return prepare, run, kv

        def timed(route):
            prepare, run, owner = route if isinstance(route, tuple) else (None, route, None)
            arg = prepare() if prepare else None
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = lib.n
            e0.record(st)
            keep = run(arg) if prepare else run()
            e1.record(st)
            torch.cuda.synchronize()
            launches = lib.n - before
            del keep
            if prepare:
                for rid in arg:
                    owner.free_request(rid)
            return e0.elapsed_time(e1), launches

        loads = {"(a) kv": load_kv, "(b) rows": load_rows, "(c) fp8": load_fp8}
        stores = {"(a) kv": store_on(kv), "(b) rows": store_rows(), "(c) fp8": store_on(fp8, fused=True)}
        pairs = B * L * (n // 2)
        moved = pairs * (2048 + 1088 + 2 * 4096)
        say(f"{elem} caches: {B} request(s) x {n} positions x {L} layers = {2 * pairs} pages, K8V4 moves {moved / 1e9:.3f} GB of records + rows "
            f"(the FP8 pool {pairs * (2 * 2048 + 2 * 4096) / 1e9:.3f} GB)")
        for what, routes in (("load", loads), ("store", stores)):
            for r in routes.values():
                timed(r)                                            # warm-up: allocator, staging ring, code objects
            ms = {name: [] for name in routes}
            launches = {}
            for _ in range(a.rounds):
                one = {name: [] for name in routes}
                for _ in range(a.reps):
                    for name, r in routes.items():                  # alternating
                        t, launches[name] = timed(r)
                        one[name].append(t)
                for name in routes:
                    ms[name].append(statistics.median(one[name]))
            m = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: (max(v) - min(v)) / m[name] for name, v in ms.items()}
            for name in routes:
                say(f"  {what:5s} {name:9s} {m[name]:9.3f} ms (medians {min(ms[name]):.3f} .. {max(ms[name]):.3f}, spread {spread[name]:.3f}), "
                    f"{launches[name]:4d} library launches")
            say(f"  {what:5s} (a) / (b): {m['(a) kv'] / m['(b) rows']:.3f} (spreads {spread['(a) kv']:.3f}, {spread['(b) rows']:.3f}); "
                f"(a) / (c): {m['(a) kv'] / m['(c) fp8']:.3f} (spreads {spread['(a) kv']:.3f}, {spread['(c) fp8']:.3f}); "
                f"(a) is {moved / (m['(a) kv'] * 1e-3) / 8e12:.3f} of 8 TB/s")
    finally:
        lib.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--elems", default="fp16,bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(f"{b}x{n}" for b, n in SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    for shape in a.shapes.split(","):
        B, n = (int(x) for x in shape.split("x"))
        for elem in a.elems.split(","):
            bench(elem, B, n, a, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
