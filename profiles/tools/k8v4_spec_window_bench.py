#!/usr/bin/env python3
"""What a draft step on a SLIDING-WINDOW layer costs on the decode kernel over the K8V4 split pool (writes profiles/k8v4_spec_window.txt).

One process, one layer timed, W = 1024, requests x stored positions in {256 x 2k, 256 x 8k, 8 x 32k} x (S, rows_per_pos) in {(4, 4), (2, 8),
(16, 1)}; every request holds an even number of positions (no tail), the step is a causal chain.
  route a  SpeckvSplitKVConnector.attend_spec(window=W): ONE speckv_ext_attend_kv_spec_window (S x rows_per_pos = 16: one group)
  route b  SpeckvSplitKVConnector.attend_chunk(window=W, splits=0) with the same step: the only route on a local layer before
  route c  SpeckvSplitKVConnector.attend_spec without a window: what the same step costs on a global layer
  route d  SpeckvSplitKVConnector.attend(window=W), ONE position at the same rows_per_pos: the "costs N single windowed steps" figure
Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians (the method of profiles/tools/shared_prefix_bench.py).
The spread (max - min of a route's rounds' medians) is printed beside every ratio's denominator as a fraction of it.

--parent-lib PATH: routes c and d -- whose kernels this tree leaves instruction for instruction as they were -- with PATH (a build of the
parent commit's library) and with this tree's library in ALTERNATING child processes (--alternations of each, a fresh process per run),
per shape the median over the processes and the spread between them.

    python profiles/tools/k8v4_spec_window_bench.py [--shapes 256x2048,256x8192,8x32768] [--steps 4x4,2x8,16x1] [--window 1024] [--reps 7]
                                                    [--rounds 5] [--parent-lib PATH] [--alternations 2] [--out profiles/k8v4_spec_window.txt]
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shared_prefix_bench import in_turn                                     # the method, unchanged


def measure(a, library, routes, say):
    """-> {(n, ctx, S, R): [(median, spread) per route]} for the routes named, over `library`"""
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    L, H, D, W = 2, 8, 128, a.window                                         # (the split pool's allocations hold an even number of regions)
    sm = D ** -0.5
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    steps = [tuple(int(x) for x in s.split("x")) for s in a.steps.split(",")]
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)       # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    got = {}
    for n, ctx in shapes:
        lib = pkg.SpeckvLib(library or pkg.library_path(), "hip:0")
        try:
            conn = SpeckvSplitKVConnector(lib, L, H, D, ctx + 64)
            rids = list(range(n))
            pk, pv = rnd(L, ctx, H, D), rnd(L, ctx, H, D)                   # (every request holds the same rows: the timing does not read values)
            keep = []
            for rid in rids:
                conn.add_request(rid)
                keep += conn.write_prefill(rid, pk, pv)
            torch.cuda.synchronize()
            for S, R in steps:
                q5, k_new, v_new = rnd(n, S, H, R, D), rnd(n, S, L, H, D), rnd(n, S, L, H, D)
                q1 = rnd(n, H, R, D)
                every = dict(a=lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm, window=W),
                             b=lambda: conn.attend_chunk(0, rids, q5, k_new, v_new, sm, splits=0, window=W),
                             c=lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm),
                             d=lambda: conn.attend(0, rids, q1, sm, window=W))
                meds = in_turn(torch, [every[r] for r in routes], a.reps, a.rounds)
                got[(n, ctx, S, R)] = [(statistics.median(m), (max(m) - min(m)) / statistics.median(m)) for m in meds]
                say(n, ctx, S, R, got[(n, ctx, S, R)])
            del keep
            for rid in rids:
                conn.free_request(rid)
        finally:
            lib.finalize()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2048,256x8192,8x32768")
    ap.add_argument("--steps", default="4x4,2x8,16x1")
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--child", default=None, help="internal: measure routes c and d over this library and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k8v4_spec_window.txt"))
    a = ap.parse_args()
    if a.child is not None:
        got = measure(a, a.child or None, "cd", lambda *x: None)
        print("RESULT " + json.dumps({"%dx%d S%d R%d" % k: [m for m, _ in v] for k, v in got.items()}), flush=True)
        return
    sys.path.insert(0, ROOT)
    import torch
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say(f"a draft step on a sliding-window layer over the K8V4 split pool: W = {a.window}, layer 0 of 2, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
        f"{datetime.date.today().isoformat()} (profiles/tools/k8v4_spec_window_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call)")
    say("columns: a = attend_spec(window=W) | b = attend_chunk(window=W, splits=0) | c = attend_spec, no window | d = attend(window=W), one position "
        "| a / b (b's spread) | a / c (c's spread) | a / d (d's spread)")
    rows = []

    def row(n, ctx, S, R, r):
        (ma, _), (mb, sb), (mc, sc), (md, sd) = r
        rows.append((n, ctx, S, R, ma / mb, sb, ma / mc, sc, ma / md, sd))
        say(f"  {n:3d} x {ctx:5d} S {S:2d} R {R}: {ma:7.3f} | {mb:7.3f} | {mc:7.3f} | {md:7.3f} | a / b {ma / mb:4.2f} ({sb:.3f}) | a / c {ma / mc:4.2f} ({sc:.3f}) "
            f"| a / d {ma / md:4.2f} ({sd:.3f})")
    measure(a, None, "abcd", row)
    for name, at in (("a / b", 4), ("a / c", 6), ("a / d", 8)):
        say(f"{name}: {min(r[at] for r in rows):.2f} .. {max(r[at] for r in rows):.2f}")
    slower = [r for r in rows if r[4] >= 1.0 - r[5]]
    say("a does not beat b beyond b's spread at: " + (", ".join(f"{n} x {ctx} S {S} R {R} ({x:.2f})" for n, ctx, S, R, x, *_ in slower) or "no shape"))
    if a.parent_lib:
        # the process that measured above has the GPU open and goes on; every child is a fresh process of its own, one at a time
        runs = {"parent": [], "this tree": []}
        args = [sys.executable, os.path.abspath(__file__), "--shapes", a.shapes, "--steps", a.steps, "--window", str(a.window), "--reps", str(a.reps),
                "--rounds", str(a.rounds)]
        for _ in range(a.alternations):
            for who, library in (("parent", os.path.abspath(a.parent_lib)), ("this tree", "")):
                out = subprocess.run(args + ["--child", library], check=True, capture_output=True, text=True).stdout
                runs[who].append(json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        say(f"routes c and d, the parent commit's library against this tree's, {a.alternations} alternating processes each: median ms (spread between the processes)")
        for key in runs["parent"][0]:
            for i, route in enumerate(("c attend_spec", "d attend(window=W)")):
                stat = {}
                for who, rs in runs.items():
                    xs = [r[key][i] for r in rs]
                    stat[who] = (statistics.median(xs), (max(xs) - min(xs)) / statistics.median(xs))
                (mp, sp), (mt, stt) = stat["parent"], stat["this tree"]
                verdict = "inside the spread" if abs(mt / mp - 1.0) <= max(sp, stt) else "OUTSIDE the spread"
                say(f"  {key:>16s} {route:18s}: parent {mp:7.3f} ({sp:.3f}) | this tree {mt:7.3f} ({stt:.3f}) | this / parent {mt / mp:5.3f}  {verdict}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
