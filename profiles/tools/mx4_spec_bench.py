#!/usr/bin/env python3
"""What a draft step of up to 16 query rows per kv head costs on an MXFP4 pool in ONE pass (attend_spec(row_block=16)) against the planned
route (writes profiles/mx4_spec.txt).

One process, requests x stored positions in {256 x 2k, 256 x 8k, 8 x 32k} x (S, rows_per_pos) in {(4, 4), (2, 8), (16, 1)}: 16 query rows per
kv head; every request holds an even number of positions (no tail), the step is a causal chain; ONE layer of --layers, then ALL of them
through attend_spec_layers.
  route a  SpeckvKVConnector.attend_spec(row_block=16): ONE speckv_ext_attend_spec_mx4 per layer (k_attend_mx4_spec: the 16 MFMA columns
           are the query rows, the records fetched once, the held rows folded inside it)
  route b  attend_spec() of the same step, what row_block=None issues: the planned call (k_attend_mx4 with grid z = 2: every record walked
           twice) and one fold launch
  route c  attend, ONE position at the same rows_per_pos: the "costs N single steps" figure (profiles/spec_step.txt, expectation (a): < 2.00)
Before a shape is timed, a's rows are compared with b's (|a - b| <= 2e-2 on rows of unit-variance values) -- at 8 x 32k that covers the merge
of many pieces.  Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every
round, per round the median of --reps calls, --rounds rounds, the median of the rounds' medians (the method of
profiles/tools/shared_prefix_bench.py).  The spread (max - min of a route's rounds' medians, as a fraction of its median) is printed for every
column: the noise a difference has to exceed.

--against PARENT_LIB: the EXISTING routes (attend and attend_spec() on the MXFP4 pool at the shapes above, and bench.py) with this build's
library and with PARENT_LIB in alternating fresh processes, --pairs pairs; per route the two sides' medians and ranges over the processes are
APPENDED to --out; the order inside a pair alternates.  (--existing is what such a process runs: it prints one JSON line.)

    python profiles/tools/mx4_spec_bench.py [--shapes 256x2048,256x8192,8x32768] [--steps 4x4,2x8,16x1] [--layers 8] [--reps 7] [--rounds 5]
                                            [--out profiles/mx4_spec.txt] [--against PARENT_LIB --pairs 3]
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


def pool(torch, pkg, n, ctx, L, H, D, rnd):
    """an engine and an MXFP4 connector whose n requests hold ctx positions each (the same rows: the timing does not read values)"""
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    conn, keep = SpeckvKVConnector(lib, L, H, D, ctx + 64, "mxfp4"), []
    pk, pv = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
    for rid in range(n):
        conn.add_request(rid)
        keep += conn.write_prefill(rid, pk, pv)
    torch.cuda.synchronize()
    return lib, conn, keep


def ramp(torch):
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)       # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()


def existing(a, shapes, steps):
    """the routes the parent commit has too, one JSON line: {route: ms}"""
    import torch
    import cxl_speckv_amd as pkg
    L, H, D, sm, res = 1, 8, 128, 128 ** -0.5, {}
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    ramp(torch)
    for n, ctx in shapes:
        lib, conn, keep = pool(torch, pkg, n, ctx, L, H, D, rnd)
        try:
            rids = list(range(n))
            for S, R in steps:
                q5, k_new, v_new, q1 = rnd(n, S, H, R, D), rnd(n, S, L, H, D), rnd(n, S, L, H, D), rnd(n, H, R, D)
                meds = in_turn(torch, [lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm), lambda: conn.attend(0, rids, q1, sm)], a.reps, a.rounds)
                res[f"{n}x{ctx} attend_spec S{S} R{R}"], res[f"{n}x{ctx} attend R{R}"] = (statistics.median(m) for m in meds)
        finally:
            del keep
            lib.finalize()
    print("EXISTING " + json.dumps(res), flush=True)


def against(a, say):
    """this build's library and a.against in alternating fresh processes"""
    sides = {"parent": {}, "this": {}}
    for pair in range(a.pairs):
        for side, path in (("parent", a.against), ("this", None))[::1 if pair % 2 == 0 else -1]:      # (parent, this), (this, parent), ...: no side is always second
            env = dict(os.environ)
            env.pop("SPECKV_LIB_PATH", None)
            if path:
                env["SPECKV_LIB_PATH"] = os.path.abspath(path)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing", "--shapes", a.shapes, "--steps", a.steps, "--reps", str(a.reps),
                                  "--rounds", str(a.rounds)], env=env, capture_output=True, text=True, timeout=600, check=True).stdout
            got = json.loads(next(l for l in out.splitlines() if l.startswith("EXISTING "))[9:])
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env, capture_output=True,
                                 text=True, timeout=600, check=True).stdout
            head = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            got["bench.py " + str(head.get("metric", "value"))] = float(head.get("value", head.get("score", 0.0)))
            for k, v in got.items():
                sides[side].setdefault(k, []).append(v)
    say(f"existing MXFP4 routes and bench.py, this build against the parent commit's library: {a.pairs} pairs of fresh processes, alternating, the order inside a pair alternating too; per side the "
        f"median of the processes and their range as a fraction of it (ms per call; bench.py: its own value)")
    outside = []
    for k in sides["this"]:
        p, t = sides["parent"][k], sides["this"][k]
        mp, mt = statistics.median(p), statistics.median(t)
        say(f"  {k:34s}: parent {mp:9.3f} ({(max(p) - min(p)) / mp:.3f}) | this {mt:9.3f} ({(max(t) - min(t)) / mt:.3f}) | this / parent {mt / mp:5.3f}")
        if not min(p) <= mt <= max(p):
            outside.append(f"{k} ({mt / mp:.3f})")
    say("this build's median outside the parent's own process-to-process range at: " + (", ".join(outside) or "no route"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x2048,256x8192,8x32768")
    ap.add_argument("--steps", default="4x4,2x8,16x1")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx4_spec.txt"))
    ap.add_argument("--against", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--existing", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    steps = [tuple(int(x) for x in s.split("x")) for s in a.steps.split(",")]
    if a.existing:
        return existing(a, shapes, steps)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    if a.against:
        against(a, say)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    import torch
    import cxl_speckv_amd as pkg
    L, H, D = a.layers, 8, 128
    sm = D ** -0.5
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    ramp(torch)
    say(f"16 query rows per kv head in one pass over an MXFP4 pool: {L} layers, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
        f"{datetime.date.today().isoformat()} (profiles/tools/mx4_spec_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call, "
        f"each column's spread in brackets)")
    say("columns: a = attend_spec(row_block=16), one speckv_ext_attend_spec_mx4 per layer | b = attend_spec(), the planned call (grid z = 2) + the fold "
        "| c = attend, one position | a / b | a / c (expectation (a) of profiles/spec_step.txt: < 2.00)")
    rows = []
    for n, ctx in shapes:
        try:
            lib, conn, keep = pool(torch, pkg, n, ctx, L, H, D, rnd)
        except (RuntimeError, MemoryError) as e:                           # a pool too small for this shape: said, not hidden
            say(f"  {n:3d} x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
            continue
        try:
            rids = list(range(n))
            for S, R in steps:
                k_new, v_new = rnd(n, S, L, H, D), rnd(n, S, L, H, D)
                for NL in (1, L):
                    q6, q2 = rnd(NL, n, S, H, R, D), rnd(NL, n, H, R, D)
                    route_a = lambda: conn.attend_spec_layers(0, NL, rids, q6, k_new, v_new, sm, row_block=16)
                    route_b = lambda: conn.attend_spec_layers(0, NL, rids, q6, k_new, v_new, sm)
                    route_c = lambda: conn.attend_layers(0, NL, rids, q2, sm)
                    apart = float((route_a() - route_b()).abs().max())
                    torch.cuda.synchronize()
                    if not apart <= 2e-2:
                        raise SystemExit(f"{n} x {ctx} S {S} R {R} layers {NL}: the one-pass call and the planned route differ by {apart}")
                    meds = in_turn(torch, [route_a, route_b, route_c], a.reps, a.rounds)
                    ma, mb, mc = (statistics.median(m) for m in meds)
                    sa, sb, sc = ((max(m) - min(m)) / statistics.median(m) for m in meds)
                    rows.append((n, ctx, S, R, NL, ma / mb, sa, sb, ma / mc))
                    say(f"  {n:3d} x {ctx:5d} S {S:2d} R {R} layers {NL}: {ma:7.3f} ({sa:.3f}) | {mb:7.3f} ({sb:.3f}) | {mc:7.3f} ({sc:.3f}) "
                        f"| a / b {ma / mb:4.2f} | a / c {ma / mc:4.2f} | max |a - b| {apart:.1e}")
        finally:
            del keep
            lib.finalize()
    if rows:
        say(f"a / b: {min(r[5] for r in rows):.2f} .. {max(r[5] for r in rows):.2f}; a / c: {min(r[8] for r in rows):.2f} .. {max(r[8] for r in rows):.2f}")
        lost = [r for r in rows if r[5] >= 1.0 - max(r[6], r[7])]
        say("a does not beat b beyond both columns' spreads at: "
            + (", ".join(f"{n} x {ctx} S {S} R {R} layers {NL} ({x:.2f})" for n, ctx, S, R, NL, x, *_ in lost) or "no shape"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
