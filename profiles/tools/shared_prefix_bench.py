#!/usr/bin/env python3
"""What reading a shared prefix once buys a decode step (writes profiles/shared_prefix.txt).

One process, one layer, per pool format: members x prefix x rows_per_pos in {1, 4, 16, 64, 256} x {2k, 8k, 32k} x {1, 4}; every member
holds 64 positions of its own behind the prefix.
  route A  fork + attend: every member is a fork of the prefix request (speckv_ext_copy_runs) with its own 64 positions committed
           behind it, and the step is SpeckvKVConnector.attend -- the only route before attend_shared existed, unchanged
  route B  attend_shared: the members hold their own 64 positions only, the step is attend + ONE speckv_ext_attend_prefix_fold
Device time between two HIP events around one call; clock ramp and warm-up untimed; the two routes timed IN TURN within every round,
per round the median of --reps calls, --rounds rounds, the median of the rounds' medians.  The spread (max - min) of route A's rounds'
medians is the noise a difference has to exceed.  The last lines give the crossover per prefix length: the smallest member count from
which B is faster than A by more than that spread.

Measured on an MI355X, 2026-10-19 (profiles/shared_prefix.txt): crossover over FP8 at prefix 2k 256 members, 8k 64, 32k 16; over
INT4_G32 and MXFP4 2k none up to 256 members, 8k 256, 32k 64.  At 64 members x 8k x rows_per_pos 4, where B reads 1/16 of A's prefix
bytes, B wins over FP8 (0.206 / 0.159 ms, spread 0.002) and IS slower over INT4_G32 (0.152 / 0.173, spread 0.003) and MXFP4 (0.134 /
0.161, spread 0.004): B's call has a floor of 0.13 ms and the walk runs at about 2 us a tile.
--splits adds columns for other piece counts (profiles/shared_prefix_splits.txt: forced 16 a little faster than the rule at 8k, 32
and 64 slower).

    python profiles/tools/shared_prefix_bench.py [--schemes fp8,int4,mxfp4] [--members 1,4,16,64,256] [--ctxs 2048,8192,32768]
                                                 [--rpps 1,4] [--splits 0] [--reps 7] [--rounds 5] [--out profiles/shared_prefix.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OWN = 64


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
    ap.add_argument("--members", default="1,4,16,64,256")
    ap.add_argument("--ctxs", default="2048,8192,32768")
    ap.add_argument("--rpps", default="1,4")
    ap.add_argument("--splits", default="0", help="attend_shared(splits=...): 0 = the library's rule (the column the verdict goes by); further values add columns")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, H, D = 1, 8, 128
    sm = D ** -0.5
    counts, ctxs, rpps, splits = ([int(x) for x in s.split(",")] for s in (a.members, a.ctxs, a.rpps, a.splits))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)           # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    say(f"a decode step over a shared prefix: {L} layer, {OWN} own positions per member, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
        f"{datetime.date.today().isoformat()} (profiles/tools/shared_prefix_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call)")
    say("columns: A = fork + attend | B = attend_shared" + "".join(f" | B with splits={x}" for x in splits[1:]) +
        " | spread = max - min of A's rounds' medians | A / B")
    wins = {}
    for scheme in a.schemes.split(","):
        say(f"{scheme}")
        for ctx in ctxs:
            T = ctx + OWN + 64
            for n in counts:
                lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
                try:
                    conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
                    root, members, twins = 1, list(range(1000, 1000 + n)), list(range(5000, 5000 + n))
                    conn.add_request(root)
                    keep = conn.write_prefill(root, rnd(L, ctx, H, D), rnd(L, ctx, H, D))
                    for rid in members:
                        conn.add_request(rid)
                    keep += conn.fork([root] * n, twins)
                    kn, vn = rnd(n, OWN, L, H, D), rnd(n, OWN, L, H, D)
                    keep += conn.commit(members, kn, vn, [range(OWN)] * n)
                    keep += conn.commit(twins, kn, vn, [range(OWN)] * n)
                    torch.cuda.synchronize()
                    for R in rpps:
                        q = rnd(n, H, R, D)
                        route_a = lambda: conn.attend(0, twins, q, sm)
                        route_b = lambda x: (lambda: conn.attend_shared(0, members, [root] * n, q, sm, splits=x))
                        meds = in_turn(torch, [route_a] + [route_b(x) for x in splits], a.reps, a.rounds)
                        ma, mb = statistics.median(meds[0]), statistics.median(meds[1])
                        spread = max(meds[0]) - min(meds[0])
                        verdict = "B WINS" if ma - mb > spread else "B not slower" if mb <= ma + spread else "B SLOWER"
                        wins.setdefault((scheme, ctx, R), []).append((n, verdict == "B WINS"))
                        more = "".join(f" | {statistics.median(m):7.3f}" for m in meds[2:])
                        say(f"  {n:3d} members x {ctx:5d} rows_per_pos {R}: {ma:7.3f} | {mb:7.3f}{more} | spread {spread:.3f} | {ma / mb:5.2f}x  {verdict}")
                    del keep
                    for rid in members + twins + [root]:
                        conn.free_request(rid)
                except (RuntimeError, MemoryError) as e:                       # a pool too small for this many forks: said, not hidden
                    say(f"  {n:3d} members x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
                finally:
                    lib.finalize()
    say("crossover (the smallest member count from which B wins by more than A's spread, at every larger count measured):")
    for (scheme, ctx, R), rows in wins.items():
        first = None
        for n, won in sorted(rows, reverse=True):
            if not won:
                break
            first = n
        say(f"  {scheme} prefix {ctx:5d} rows_per_pos {R}: {'none measured' if first is None else first}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
