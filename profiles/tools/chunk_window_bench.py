#!/usr/bin/env python3
"""What a sliding window costs and saves attend_chunk (writes profiles/chunk_window.txt).

One process, one layer, rows_per_pos = 8, per pool format: requests x context x step in {1, 4, 256} x {2k, 8k, 32k} x {S = 1, 16, a
512-position chunk}.  Per shape the stream time of attend_chunk
    none/1   window=None, splits=1: the launch without pieces
    none/0   window=None, splits=0 (the library's rule): THE BASELINE -- the unwindowed call at the same shape
    W1024, W4096        window=W, splits=0: the tiles walked follow W, not the context
    W>=all   a window no row loses a position under: the engine issues the baseline's launches
    W=all-1  one position less: the WINDOW instances over the same tiles -- what the lower bound itself costs
and, for S = 1, of attend() (the decode route, which has no window).  Device time between two HIP events around one call; clock ramp
and warm-up untimed; the variants timed IN TURN within every round, per round the median of --reps calls, --rounds rounds, the median
of the rounds' medians.  The spread (max - min) of the baseline's rounds' medians is the noise a difference has to exceed.

    python profiles/tools/chunk_window_bench.py [--schemes fp8,int4,mxfp4] [--seqs 1,4,256] [--ctxs 2048,8192,32768] [--steps 1,16,512]
                                                [--big-ctxs 2048,8192] [--reps 7] [--rounds 5] [--out profiles/chunk_window.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS = (1024, 4096)


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
    ap.add_argument("--seqs", default="1,4,256")
    ap.add_argument("--ctxs", default="2048,8192,32768")
    ap.add_argument("--steps", default="1,16,512")
    ap.add_argument("--big", type=int, default=64, help="batches of at least this many requests take --big-ctxs and --big-steps")
    ap.add_argument("--big-ctxs", default="2048,8192")
    ap.add_argument("--big-steps", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_window.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, R, H, D = 1, 8, 8, 128
    sm = D ** -0.5
    ints = lambda s: [int(x) for x in s.split(",") if x]
    seqs, ctxs, steps = ints(a.seqs), ints(a.ctxs), ints(a.steps)
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
    say(f"attend_chunk under a sliding window: {L} layer, rows_per_pos {R}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs "
        f"(profiles/tools/chunk_window_bench.py, {a.rounds} rounds of {a.reps} calls, variants in turn; ms per call)")
    say("columns: none/1 | none/0 = BASELINE | W1024 | W4096 | W>=all | W=all-1 | attend() (S = 1 only); "
        "spread = max - min of the baseline's rounds' medians; ratios are baseline / variant (> 1: the variant is faster)")
    say("tiles: 32-position tiles a query block walks, baseline -> W1024 / W4096 (the last block of the step; chunk_window_walk)")
    for scheme in a.schemes.split(","):
        say(f"{scheme}")
        for B in seqs:
            for ctx in (ints(a.big_ctxs) if B >= a.big else ctxs):
                T = ctx + 512 + 64
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
                    for n in (ints(a.big_steps) if B >= a.big else steps):
                        q, kn, vn = rnd(B, n, H, R, D), rnd(B, n, L, H, D), rnd(B, n, L, H, D)
                        call = lambda w, s=0: (lambda: conn.attend_chunk(0, ids, q, kn, vn, sm, splits=s, window=w))
                        fns = [call(None, 1), call(None)] + [call(w) for w in WINDOWS] + [call(ctx + n), call(ctx + n - 1)]
                        if n == 1:
                            qd = q[:, 0].contiguous()
                            fns.append(lambda: conn.attend(0, ids, qd, sm))
                        meds = in_turn(torch, fns, a.reps, a.rounds)
                        med = [statistics.median(m) for m in meds]
                        spread = max(meds[1]) - min(meds[1])
                        walk = lambda w: SpeckvKVConnector.chunk_window_walk([n], [ctx], R, w)[0][-1][1]
                        cols = " | ".join(f"{m:8.4f}" for m in med[:6]) + " | " + (f"{med[6]:8.4f}" if len(med) > 6 else "    --  ")
                        same = "inside" if abs(med[4] - med[1]) <= spread else "BEYOND"
                        say(f"  {B:3d} x {ctx:5d} S {n:3d}: {cols}   spread {spread:.4f}  tiles {walk(None)} -> {walk(1024)} / {walk(4096)}  "
                            f"base/W1024 {med[1] / med[2]:.2f}x  base/W4096 {med[1] / med[3]:.2f}x  W>=all {same} the spread  "
                            f"W=all-1/base {med[5] / med[1]:.3f}" + (f"  attend()/W1024 {med[6] / med[2]:.2f}x" if len(med) > 6 else ""))
                    for rid in ids:
                        conn.free_request(rid)
                finally:
                    lib.finalize()


if __name__ == "__main__":
    main()
