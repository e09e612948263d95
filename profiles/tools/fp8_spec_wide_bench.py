#!/usr/bin/env python3
"""What 32 query rows per kv head in ONE pass cost against the 16-row route over an FP8_E4M3 pool (writes profiles/fp8_spec_wide.txt).

One process, one layer timed, requests x stored positions in {256 x 2k, 256 x 8k, 8 x 32k} x (S, rows_per_pos) in {(4, 8), (8, 4), (16, 2)}:
32 query rows per kv head; every request holds an even number of positions (no tail), the step is a causal chain; on a global layer and
then under a window of --window positions.
  route a  SpeckvKVConnector.attend_spec(rows_per_pass=32): ONE speckv_ext_attend_spec_wide (k_attend_fp8_wide, two blocks of 16 rows per
           wave over each tile's K bytes, f16 V operand and V reference scale; the held rows folded inside it)
  route b  attend_spec() of the same step, what rows_per_pass=16 issues: under a window TWO speckv_ext_attend_spec_window calls of 16
           rows; on a global layer TWO planned calls each followed by its fold launch -- four launches, each pair walking every record
  route c  attend, ONE position at the same rows_per_pos: the "costs N single steps" figure
Before a shape is timed, a's rows are compared with b's (the same step through the other kernels: |a - b| <= 2e-2 on rows of unit-variance
values, far above what the accumulation orders differ by) -- at 8 x 32k that covers the merge of many pieces over both row blocks.
Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians (the method of profiles/tools/shared_prefix_bench.py).
The spread (max - min of a route's rounds' medians, as a fraction of its median) is printed for every column: the noise a difference has to
exceed.  The device's clock as torch reports it is printed before and after.

    python profiles/tools/fp8_spec_wide_bench.py [--shapes 256x2048,256x8192,8x32768] [--steps 4x8,8x4,16x2] [--window 1024] [--reps 7]
                                                 [--rounds 5] [--out profiles/fp8_spec_wide.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shared_prefix_bench import in_turn                                     # the method, unchanged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2048,256x8192,8x32768")
    ap.add_argument("--steps", default="4x8,8x4,16x2")
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_spec_wide.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, H, D = 1, 8, 128
    sm = D ** -0.5
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    steps = [tuple(int(x) for x in s.split("x")) for s in a.steps.split(",")]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def clock():
        try:
            return f"{torch.cuda.clock_rate()} MHz"
        except Exception as e:                                              # (a torch without the query: said, not hidden)
            return f"not reported ({type(e).__name__})"
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)       # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    say(f"32 query rows per kv head in one pass over an FP8_E4M3 pool: layer 0 of {L}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
        f"{datetime.date.today().isoformat()} (profiles/tools/fp8_spec_wide_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call, "
        f"each column's spread in brackets); clock at the start {clock()}")
    say("columns: a = attend_spec(rows_per_pass=32), one wide call | b = attend_spec(), the 16-row route (W: two calls; no W: two planned calls + two folds) "
        "| c = attend, one position | a / b | a / c")
    rows = []
    for n, ctx in shapes:
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            conn = SpeckvKVConnector(lib, L, H, D, ctx + 64, "fp8")
            rids = list(range(n))
            pk, pv = rnd(L, ctx, H, D), rnd(L, ctx, H, D)                   # (every request holds the same rows: the timing does not read values)
            keep = []
            for rid in rids:
                conn.add_request(rid)
                keep += conn.write_prefill(rid, pk, pv)
            torch.cuda.synchronize()
            for window in (None, a.window):
                for S, R in steps:
                    q5, k_new, v_new = rnd(n, S, H, R, D), rnd(n, S, L, H, D), rnd(n, S, L, H, D)
                    q1 = rnd(n, H, R, D)
                    route_a = lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm, window=window, rows_per_pass=32)
                    route_b = lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm, window=window)
                    route_c = lambda: conn.attend(0, rids, q1, sm, window=window)
                    apart = float((route_a() - route_b()).abs().max())
                    torch.cuda.synchronize()
                    if not apart <= 2e-2:
                        raise SystemExit(f"{n} x {ctx} S {S} R {R} window {window}: the wide call and the 16-row route differ by {apart}")
                    meds = in_turn(torch, [route_a, route_b, route_c], a.reps, a.rounds)
                    ma, mb, mc = (statistics.median(m) for m in meds)
                    sa, sb, sc = ((max(m) - min(m)) / statistics.median(m) for m in meds)
                    rows.append((n, ctx, S, R, window, ma / mb, sa, sb, ma / mc))
                    say(f"  {n:3d} x {ctx:5d} S {S:2d} R {R} W {window or '-':>4}: {ma:7.3f} ({sa:.3f}) | {mb:7.3f} ({sb:.3f}) | {mc:7.3f} ({sc:.3f}) "
                        f"| a / b {ma / mb:4.2f} | a / c {ma / mc:4.2f} | max |a - b| {apart:.1e}")
            del keep
            for rid in rids:
                conn.free_request(rid)
        except (RuntimeError, MemoryError) as e:                           # a pool too small for this shape: said, not hidden
            say(f"  {n:3d} x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
        finally:
            lib.finalize()
    if rows:
        say(f"a / b: {min(r[5] for r in rows):.2f} .. {max(r[5] for r in rows):.2f}; a / c: {min(r[8] for r in rows):.2f} .. {max(r[8] for r in rows):.2f}")
        lost = [r for r in rows if r[5] >= 1.0 - max(r[6], r[7])]
        say("a does not beat b beyond both columns' spreads at: "
            + (", ".join(f"{n} x {ctx} S {S} R {R} W {w or '-'} ({x:.2f})" for n, ctx, S, R, w, x, *_ in lost) or "no shape"))
    say(f"clock at the end {clock()}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
