#!/usr/bin/env python3
"""What a sliding window saves the batch decode step (writes profiles/decode_window.txt).

One process, one layer, G = 8 query rows per kv head, per pool format: 256 requests x {2k, 8k} stored positions x W in {1024, 4096}.
Per shape the stream time of ONE layer's attention of the step, four variants:
    (a) windowed    speckv_ext_attend_*_planned over a plan of speckv_ext_attend_batch_plan_window(window = W)
    (b) unwindowed  the same call over the plan of speckv_ext_attend_batch_plan at the same shape: the launch without a window
    (c) floor       the unwindowed planned call over the first W stored positions of the same requests, planned under the window's
                    tile bound (max_pos_end = 32 ceil((W + 31) / 32)): the same geometry and tile count without the mask -- other
                    addresses, though (the head of the context, not its end), so (a) may also come out FASTER than it; the verdict
                    is two-sided
    (d) chunk       SpeckvKVConnector.attend_chunk(S = 1, window = W): the route a local layer's decode step had before
Device time between two HIP events around one call; clock ramp and warm-up untimed; the variants timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians.  The spread (max - min) of a baseline's rounds'
medians is the noise a difference from it has to exceed.  Ratios are a / baseline (< 1: the windowed call is faster).

    python profiles/tools/decode_window_bench.py [--schemes fp8,int4,mxfp4] [--seqs 256] [--ctxs 2048,8192] [--windows 1024,4096]
                                                 [--reps 7] [--rounds 5] [--out profiles/decode_window.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        keep = fn()
        b.record()
        b.synchronize()
        del keep
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def in_turn(torch, fns, reps, rounds):
    """per function the rounds' medians, the functions timed in turn within every round"""
    meds = [[] for _ in fns]
    for _ in range(rounds):
        for m, fn in zip(meds, fns):
            m.append(timed(torch, fn, reps, 2))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", default="256")
    ap.add_argument("--ctxs", default="2048,8192")
    ap.add_argument("--windows", default="1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_window.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SCHEMES, SpeckvKVConnector

    L, G, H, D = 1, 8, 8, 128
    sm = D ** -0.5
    ints = lambda s: [int(x) for x in s.split(",") if x]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                                           # kept current: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)           # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    say(f"batch decode attention under a sliding window: {L} layer, G = {G}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs "
        f"(profiles/tools/decode_window_bench.py, {a.rounds} rounds of {a.reps} calls, variants in turn; ms per call)")
    say("columns: (a) windowed planned | (b) unwindowed planned, same shape | (c) unwindowed planned over W positions = the floor | "
        "(d) attend_chunk(S = 1, window = W); spread = max - min of that column's rounds' medians; ratios a / x (< 1: the windowed call is faster)")
    st = torch.cuda.Stream()
    for scheme in a.schemes.split(","):
        say(f"{scheme}")
        code = SCHEMES[scheme]
        for B in ints(a.seqs):
            for ctx in ints(a.ctxs):
                T = ctx + 64
                lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
                try:
                    conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
                    ids = list(range(1, B + 1))
                    k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
                    keep = []
                    for rid in ids:
                        conn.add_request(rid)
                        keep += conn.write_prefill(rid, k, v)
                    torch.cuda.synchronize()
                    del keep
                    handles = (ctypes.c_uint64 * B)(*[conn.requests[r].handle for r in ids])
                    q = rnd(B, H, G, D)
                    qc, kn, vn = q[:, None].contiguous(), rnd(B, 1, L, H, D), rnd(B, 1, L, H, D)
                    out = torch.empty((B, H, G, D), dtype=torch.float32, device="cuda")
                    lse = torch.empty((B, H, G), dtype=torch.float32, device="cuda")
                    bound = (ctx + 511) // 512 * 512

                    def plan(n_pos, window, b=None):
                        """a plan buffer for B requests of n_pos stored positions each (the step's own the last of them), bound b"""
                        nbytes = lib.attend_plan_window_bytes(B)
                        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                        pe = (ctypes.c_uint32 * B)(*([n_pos] * B))
                        b = min(T, (n_pos + 511) // 512 * 512) if b is None else b
                        if window:
                            lib.attend_batch_plan_window(handles, pe, (ctypes.c_uint32 * B)(*([n_pos - 1] * B)), window, b, buf.data_ptr(), nbytes, st.cuda_stream)
                        else:
                            lib.attend_batch_plan(handles, pe, b, buf.data_ptr(), lib.attend_plan_bytes(B), st.cuda_stream)
                        st.synchronize()
                        return buf, b

                    def launch(buf_bound):
                        buf, b = buf_bound
                        def fn():
                            with torch.cuda.stream(st):
                                lib.attend_planned(code, buf.data_ptr(), B, 0, q.data_ptr(), G, b, sm, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
                        return fn

                    def timed_on(fn):
                        """events on the stream the launches run on"""
                        def run():
                            with torch.cuda.stream(st):
                                return fn()
                        return run
                    for W in ints(a.windows):
                        if W >= ctx:
                            say(f"  {B:3d} x {ctx:5d} W {W:5d}: the window covers the context: the unwindowed launch")
                            continue
                        fns = [launch(plan(ctx, W)), launch(plan(ctx, 0)), launch(plan(W, 0, min(bound, (W + 62) // 32 * 32))),
                               lambda: conn.attend_chunk(0, ids, qc, kn, vn, sm, splits=0, window=W)]
                        torch.cuda.synchronize()
                        with torch.cuda.stream(st):
                            meds = in_turn(torch, fns, a.reps, a.rounds)
                        med = [statistics.median(m) for m in meds]
                        spread = [max(m) - min(m) for m in meds]
                        tiles = (SpeckvKVConnector.decode_window_range(ctx, W)[2] + 15) // 16
                        within = ("within" if abs(med[0] - med[2]) <= spread[2] + spread[0] + med[2] / max(1, (W + 31) // 32) else
                                  "SLOWER than" if med[0] > med[2] else "FASTER than")
                        beats = "beats" if med[3] - med[0] > spread[0] + spread[3] else "DOES NOT beat"
                        say(f"  {B:3d} x {ctx:5d} W {W:5d}: " + " | ".join(f"{m:7.4f} (spread {s:.4f})" for m, s in zip(med, spread)) +
                            f"   tiles {ctx // 32} -> {tiles}  a/b {med[0] / med[1]:.3f}  a/c {med[0] / med[2]:.3f}  a/d {med[0] / med[3]:.3f}  "
                            f"(a) {within} the floor (both spreads + one tile); {beats} (d) by more than both spreads")
                    for rid in ids:
                        conn.free_request(rid)
                finally:
                    lib.finalize()


if __name__ == "__main__":
    main()
