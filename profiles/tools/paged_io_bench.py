#!/usr/bin/env python3
"""Paged-cache transfers against the row route and against the contiguous ceiling (profiles/paged_io.txt).

Shapes: 4 requests x 8k positions and 1 request x 32k positions, 8 layers, FP8 / INT4_G32 / MXFP4; per-layer caches
[2, blocks, 16, 8, 128] fp16, every request's positions scattered over blocks by a random block table.  Three things are timed in one
process, alternating, HIP events on one stream around each call, after a warm-up of every route:
  paged    SpeckvKVConnector.load_paged / store_paged (one speckv_ext_read_slots / _write_slots launch), in BOTH wave orders
           (speckv_ext_set_tuning slots_kind_fast 0 / 1);
  rows     the row route of the same connector (what load_paged / store_paged fall back to, and what SpeckvVllmConnector does without
           paged_io): kv_rows + index_copy_ per (request, layer, kind); index_select per layer, torch.stack twice, write_prefill;
  ceiling  speckv_ext_fetch_range / speckv_ext_write_runs over the same pages with ONE contiguous buffer per request: no slots at all.
Reported per route: the median of `rounds` medians of `reps`, the library launches counted by a wrapper around the library object,
and bytes moved (record bytes plus 4 KiB per page) over the time as a fraction of the 8 TB/s roofline; then the ratio of the paged
route to the row route and its distance to the ceiling.  A store is timed on fresh requests (allocated before the first event, freed
after the last).

    python profiles/tools/paged_io_bench.py [--layers 8] [--schemes fp8,int4,mxfp4] [--reps 5] [--rounds 3] [--out FILE]

--bf16 (profiles/paged_io_bf16.txt): the fused route (load_paged / store_paged with fused=True: speckv_ext_read_slots_ex /
_write_slots_ex) on bf16 caches, in the same process and alternating with
  fp16 fused   the same call on fp16 caches of the same shape (equal bytes: a gap is the conversion's instruction issue);
  bf16 rows    the row route bf16 caches take without fused=True;
and, for stores, a request that holds one position already and gets n - 2 more (its tail goes in as the held-in row, the new odd
last position comes back as a held-out row) against the even store of n - 2 positions into an empty request.

--kscale (profiles/paged_io_kscale.txt): a connector with a K pre-scale on the one launch (load_paged / store_paged with fused=True,
kscale=True: speckv_ext_read_slots_kmul / _write_slots_kmul), on fp16 and on bf16 caches, in the same process and alternating with
  fused        the unscaled fused call of a connector without a pre-scale on the same caches (the _ex kernels: equal bytes, so a
               gap is the factor's load and multiply on the K waves);
  kscale rows  the row route the pre-scaled connector takes for the same call without kscale=True.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REC_BYTES = {"fp8": 2048, "int4": 1152, "mxfp4": 1088}
SHAPES = ((4, 8192), (1, 32768))
BS = 16
COUNTED = ("read_slots", "write_slots", "read_slots_ex", "write_slots_ex", "read_slots_kmul", "write_slots_kmul", "fetch_range", "write_runs")


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


def bench(scheme, B, n, a, say):
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        H, D, L = 8, 128, a.layers
        conn = SpeckvKVConnector(lib, L, H, D, n, scheme)
        rows_conn = SpeckvKVConnector(lib, L, H, D, n, scheme)
        rows_conn._paged_geometry = lambda caches: None            # the row route of the same tree
        blocks = B * n // BS
        caches = [torch.randn((2, blocks, BS, H, D), device="cuda").half() for _ in range(L)]
        table = np.random.default_rng(1).permutation(blocks)
        slots = (table[:, None] * BS + np.arange(BS)[None]).reshape(-1).astype(np.int64)         # request i: slots[i * n : (i + 1) * n]
        d_slots = torch.from_numpy(slots).cuda()
        ids = list(range(1, B + 1))
        for c in (conn, rows_conn):
            for rid in ids:
                c.add_request(rid if c is conn else 100 + rid)
        rows_ids = [100 + r for r in ids]
        st = torch.cuda.Stream()
        conn.store_paged(ids, [n] * B, d_slots, caches, stream=st)
        keep = rows_conn.store_paged(rows_ids, [n] * B, d_slots, caches, stream=st)
        torch.cuda.synchronize()
        del keep
        contiguous = torch.empty((2 * L * (n // 2), 4096), dtype=torch.uint8, device="cuda")
        fresh = iter(range(1000, 10 ** 9))

        def load_paged():
            conn.load_paged(ids, [0] * B, [n] * B, d_slots, caches, stream=st)

        def load_rows():
            rows_conn.load_paged(rows_ids, [0] * B, [n] * B, d_slots, caches, stream=st)

        def load_ceiling():
            for rid in ids:
                lib.fetch_range(conn.requests[rid].handle, 0, 2 * L * (n // 2), contiguous.data_ptr(), False, st.cuda_stream)

        def store_on(c):
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    c.add_request(rid)
                return new

            def run(new):
                return c.store_paged(new, [n] * B, d_slots, caches, stream=st)
            return prepare, run, c

        def store_ceiling():
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    conn.add_request(rid)
                return new

            def run(new):
                for rid in new:
                    firsts = [j * (n // 2) for j in range(2 * L)]
                    srcs = [contiguous.data_ptr() + j * (n // 2) * 4096 for j in range(2 * L)]
                    lib.write_runs(conn.requests[rid].handle, firsts, srcs, n // 2, st.cuda_stream)
            return prepare, run, conn

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

        def order(kind_fast, route):
            def run(*args):
                conn.lib.set_tuning("slots_kind_fast", kind_fast)
                try:
                    return route(*args)
                finally:
                    conn.lib.set_tuning("slots_kind_fast", 0)
            return run

        sp, sr, _ = store_on(conn)
        stores = {"paged, pair fast": (sp, order(0, sr), conn), "paged, kind fast": (sp, order(1, sr), conn),
                  "rows": store_on(rows_conn), "ceiling": store_ceiling()}
        loads = {"paged, pair fast": order(0, load_paged), "paged, kind fast": order(1, load_paged), "rows": load_rows, "ceiling": load_ceiling}
        pages = B * 2 * L * (n // 2)
        moved = pages * (REC_BYTES[scheme] + 4096)
        say(f"{scheme}: {B} request(s) x {n} positions x {L} layers = {pages} pages, {moved / 1e9:.3f} GB of records + rows")
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
            for name in routes:
                say(f"  {what:5s} {name:17s} {m[name]:9.3f} ms (medians {min(ms[name]):.3f} .. {max(ms[name]):.3f}), {launches[name]:4d} library launches, "
                    f"{moved / (m[name] * 1e-3) / 8e12:.3f} of the 8 TB/s roofline")
            best = min(("paged, pair fast", "paged, kind fast"), key=lambda k: m[k])
            say(f"  {what:5s} rows / paged ({best}): {m['rows'] / m[best]:.2f}x; paged / ceiling: {m[best] / m['ceiling']:.2f}x; "
                f"pair fast / kind fast: {m['paged, pair fast'] / m['paged, kind fast']:.3f}")
    finally:
        lib.finalize()


def bench_bf16(scheme, B, n, a, say):
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        H, D, L = 8, 128, a.layers
        conn = SpeckvKVConnector(lib, L, H, D, n, scheme)
        blocks = B * n // BS
        c16 = [torch.randn((2, blocks, BS, H, D), device="cuda").half() for _ in range(L)]
        cbf = [c.to(torch.bfloat16) for c in c16]
        table = np.random.default_rng(1).permutation(blocks)
        slots = (table[:, None] * BS + np.arange(BS)[None]).reshape(-1).astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        short = torch.from_numpy(np.concatenate([slots[i * n:i * n + n - 2] for i in range(B)])).cuda()       # n - 2 positions per request
        ones = torch.from_numpy(np.asarray([slots[i * n + n - 1] for i in range(B)])).cuda()
        ids = list(range(1, B + 1))
        for rid in ids:
            conn.add_request(rid)
        st = torch.cuda.Stream()
        conn.store_paged(ids, [n] * B, d_slots, cbf, stream=st, fused=True)
        torch.cuda.synchronize()
        fresh = iter(range(1000, 10 ** 9))

        def load(caches, fused):
            return lambda: conn.load_paged(ids, [0] * B, [n] * B, d_slots, caches, stream=st, fused=fused)

        def store(caches, fused, count, mapping, held):
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    conn.add_request(rid)
                if held:                                            # one position first: the request's tail
                    conn.store_paged(new, [1] * B, ones, caches, stream=st, fused=True)
                return new

            def run(new):
                return conn.store_paged(new, [count] * B, mapping, caches, stream=st, fused=fused)
            return prepare, run

        def timed(route):
            prepare, run = route if isinstance(route, tuple) else (None, route)
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
                    conn.free_request(rid)
            return e0.elapsed_time(e1), launches

        loads = {"fp16 fused": load(c16, True), "bf16 fused": load(cbf, True), "bf16 rows": load(cbf, False)}
        stores = {"fp16 fused": store(c16, True, n, d_slots, False), "bf16 fused": store(cbf, True, n, d_slots, False),
                  "bf16 rows": store(cbf, False, n, d_slots, False),
                  "bf16 even n-2": store(cbf, True, n - 2, short, False), "bf16 odd n-2": store(cbf, True, n - 2, short, True)}
        pages = B * 2 * L * (n // 2)
        moved = pages * (REC_BYTES[scheme] + 4096)
        say(f"{scheme}: {B} request(s) x {n} positions x {L} layers = {pages} pages, {moved / 1e9:.3f} GB of records + rows")
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
            for name in routes:
                say(f"  {what:5s} {name:14s} {m[name]:9.3f} ms (medians {min(ms[name]):.3f} .. {max(ms[name]):.3f}), {launches[name]:4d} library launches, "
                    f"{moved / (m[name] * 1e-3) / 8e12:.3f} of the 8 TB/s roofline")
            line = f"  {what:5s} bf16 fused / fp16 fused: {m['bf16 fused'] / m['fp16 fused']:.3f}; bf16 rows / bf16 fused: {m['bf16 rows'] / m['bf16 fused']:.2f}x"
            if what == "store":
                line += f"; odd (held rows) / even at n - 2: {m['bf16 odd n-2'] / m['bf16 even n-2']:.3f}"
            say(line)
    finally:
        lib.finalize()


def bench_kscale(scheme, B, n, a, say):
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = Counting(pkg.SpeckvLib(pkg.library_path(), "hip:0"))
    try:
        H, D, L = 8, 128, a.layers
        plain, scaled = SpeckvKVConnector(lib, L, H, D, n, scheme), SpeckvKVConnector(lib, L, H, D, n, scheme)
        l, h, c = np.meshgrid(np.arange(L), np.arange(H), np.arange(D), indexing="ij")
        scaled.set_k_channel_scale(torch.from_numpy(np.exp2(((7 * l + 3 * h + c) % 9) - 4).astype(np.float32)).cuda())
        blocks = B * n // BS
        c16 = [torch.randn((2, blocks, BS, H, D), device="cuda").half() for _ in range(L)]
        cbf = [c.to(torch.bfloat16) for c in c16]
        table = np.random.default_rng(1).permutation(blocks)
        slots = (table[:, None] * BS + np.arange(BS)[None]).reshape(-1).astype(np.int64)
        d_slots = torch.from_numpy(slots).cuda()
        ids = list(range(1, B + 1))
        st = torch.cuda.Stream()
        for conn, kw in ((plain, dict(fused=True)), (scaled, dict(fused=True, kscale=True))):
            for rid in ids:
                conn.add_request(rid)
            conn.store_paged(ids, [n] * B, d_slots, cbf, stream=st, **kw)
        torch.cuda.synchronize()
        fresh = iter(range(1000, 10 ** 9))

        def load(conn, caches, **kw):
            return lambda: conn.load_paged(ids, [0] * B, [n] * B, d_slots, caches, stream=st, fused=True, **kw)

        def store(conn, caches, **kw):
            def prepare():
                new = [next(fresh) for _ in ids]
                for rid in new:
                    conn.add_request(rid)
                return new

            def run(new):
                return conn.store_paged(new, [n] * B, d_slots, caches, stream=st, fused=True, **kw)
            return prepare, run, conn

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

        loads, stores = {}, {}
        for name, caches in (("fp16", c16), ("bf16", cbf)):
            loads[f"{name} fused"], stores[f"{name} fused"] = load(plain, caches), store(plain, caches)
            loads[f"{name} kscale"], stores[f"{name} kscale"] = load(scaled, caches, kscale=True), store(scaled, caches, kscale=True)
            loads[f"{name} kscale rows"], stores[f"{name} kscale rows"] = load(scaled, caches), store(scaled, caches)
        pages = B * 2 * L * (n // 2)
        moved = pages * (REC_BYTES[scheme] + 4096)
        say(f"{scheme}: {B} request(s) x {n} positions x {L} layers = {pages} pages, {moved / 1e9:.3f} GB of records + rows")
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
            for name in routes:
                say(f"  {what:5s} {name:16s} {m[name]:9.3f} ms (medians {min(ms[name]):.3f} .. {max(ms[name]):.3f}), {launches[name]:4d} library launches, "
                    f"{moved / (m[name] * 1e-3) / 8e12:.3f} of the 8 TB/s roofline")
            for name in ("fp16", "bf16"):
                say(f"  {what:5s} {name} kscale / {name} fused: {m[name + ' kscale'] / m[name + ' fused']:.3f}; "
                    f"{name} kscale rows / {name} kscale: {m[name + ' kscale rows'] / m[name + ' kscale']:.2f}x")
    finally:
        lib.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(f"{b}x{n}" for b, n in SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--bf16", action="store_true", help="the fused route on bf16 caches (see the module's text)")
    ap.add_argument("--kscale", action="store_true", help="a K pre-scale inside the fused route (see the module's text)")
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    for shape in a.shapes.split(","):
        B, n = (int(x) for x in shape.split("x"))
        for scheme in a.schemes.split(","):
            (bench_kscale if a.kscale else bench_bf16 if a.bf16 else bench)(scheme, B, n, a, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
