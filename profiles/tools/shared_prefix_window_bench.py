#!/usr/bin/env python3
"""What a window on the prefix part costs and buys a decode step (writes profiles/shared_prefix_window.txt).

One process, one layer, per pool format: members x prefix x W x rows_per_pos in {64, 256} x {8k, 32k} x {1024, 4096} x {1, 4}; every
member holds 64 positions of its own behind the prefix.
  route U  attend_shared            the unwindowed call of a global layer at the same shape (the fold walks the whole prefix)
  route B  attend_shared(window=W)  attend(window=W) on the members' own 64 positions + ONE speckv_ext_attend_prefix_fold_window,
                                    which walks the ceil((W - 64) / 32) + 1 tiles of the prefix the window still covers
  route A  fork + attend(window=W)  every member a fork of the prefix with its 64 positions behind it: the only correct route for a
                                    local layer before the window entry existed; it walks about W / 32 tiles per member too
Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians with the spread (max - min of the rounds'
medians) beside each figure.  (a) B against U: the windowed fold should follow the tiles walked and be flat in the prefix length;
(b) B against A: sharing saves little bandwidth on a local layer and the fold has a floor, so B may well be SLOWER -- what the
route buys there is correctness and pool capacity (the prefix is stored once on every layer), not speed.
(c) --parent-lib PATH: the unwindowed attend_shared and attend_chunk_shared of this library against another build of the library
(the parent commit's), the two libraries ALTERNATING round by round, each opened, measured and closed in turn.  PATH is a
libcxlspeckv.so built from a checkout of the parent commit in a directory of its own, by that checkout's own build --
`git worktree add ../parent HEAD~1 && (cd ../parent && python -c "import __graft_entry__ as g; g.build()")`, then
`--parent-lib ../parent/cxl-speckv_amd/lib/libcxlspeckv.so`; this tree's connector drives both (an entry the other library lacks is
simply never called by the unwindowed routes).

    python profiles/tools/shared_prefix_window_bench.py [--schemes fp8,int4,mxfp4] [--members 64,256] [--ctxs 8192,32768]
            [--windows 1024,4096] [--rpps 1,4] [--reps 7] [--rounds 5] [--parent-lib PATH] [--out profiles/shared_prefix_window.txt]
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


def fig(meds):
    return f"{statistics.median(meds):7.3f} +-{max(meds) - min(meds):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--members", default="64,256")
    ap.add_argument("--ctxs", default="8192,32768")
    ap.add_argument("--windows", default="1024,4096")
    ap.add_argument("--rpps", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="another build of libcxlspeckv.so to alternate the unwindowed routes against (part c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix_window.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, H, D = 1, 8, 128
    sm = D ** -0.5
    counts, ctxs, windows, rpps = ([int(x) for x in s.split(",")] for s in (a.members, a.ctxs, a.windows, a.rpps))
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
    say(f"a decode step over a shared prefix on a sliding-window layer: {L} layer, {OWN} own positions per member, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs, {datetime.date.today().isoformat()} "
        f"(profiles/tools/shared_prefix_window_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call, "
        "median of the rounds' medians +- their spread)")
    say("columns: tiles the windowed fold walks / the unwindowed one | U = attend_shared | B = attend_shared(window=W) | "
        "A = fork + attend(window=W) | U / B | A / B")
    verdicts = {}
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
                        for W in windows:
                            walk = SpeckvKVConnector.prefix_window_walk([0, n], [ctx] * n, [OWN] * n, [1] * n, W)[0][1]
                            route_u = lambda: conn.attend_shared(0, members, [root] * n, q, sm)
                            route_b = lambda: conn.attend_shared(0, members, [root] * n, q, sm, window=W)
                            route_a = lambda: conn.attend(0, twins, q, sm, window=W)
                            mu, mb, ma = in_turn(torch, [route_u, route_b, route_a], a.reps, a.rounds)
                            u, b, t = (statistics.median(m) for m in (mu, mb, ma))
                            spread = max(max(m) - min(m) for m in (mb, ma))
                            verdict = "B WINS" if t - b > spread else "B not slower" if b <= t + spread else "B SLOWER"
                            verdicts.setdefault((scheme, ctx, W, R), []).append((n, verdict))
                            say(f"  {n:3d} members x {ctx:5d} W {W:4d} rows_per_pos {R}: tiles {walk:3d} / {(ctx + 31) // 32:4d} | {fig(mu)} | {fig(mb)} | "
                                f"{fig(ma)} | {u / b:5.2f}x | {t / b:5.2f}x  {verdict} against fork + attend(window)")
                    del keep
                    for rid in members + twins + [root]:
                        conn.free_request(rid)
                except (RuntimeError, MemoryError) as e:                       # a pool too small for this many forks: said, not hidden
                    say(f"  {n:3d} members x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
                finally:
                    lib.finalize()
    say("(b) attend_shared(window=W) against fork + attend(window=W), per shape and member count:")
    for (scheme, ctx, W, R), rows in verdicts.items():
        say(f"  {scheme} prefix {ctx:5d} W {W:4d} rows_per_pos {R}: " + ", ".join(f"{n} members {v}" for n, v in rows))
    if a.parent_lib:
        say(f"(c) the unwindowed routes, this library against {os.path.basename(a.parent_lib)} = the library built from a checkout of the parent "
            "commit by that checkout's own build (the tool's docstring has the commands), libraries alternating "
            f"({a.rounds} rounds each, a round = the library opened, {a.reps} calls, closed): ms per call, median of the rounds' medians +- spread")
        S = 16
        for scheme in a.schemes.split(","):
            for ctx in ctxs:
                n, R, T = counts[0], rpps[-1], ctx + OWN + 64
                meds = {("this", "attend_shared"): [], ("parent", "attend_shared"): [], ("this", "attend_chunk_shared"): [], ("parent", "attend_chunk_shared"): []}
                for _ in range(a.rounds):
                    for name, path in (("parent", a.parent_lib), ("this", pkg.library_path())):
                        lib = pkg.SpeckvLib(path, "hip:0")
                        try:
                            conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
                            root, members = 1, list(range(1000, 1000 + n))
                            conn.add_request(root)
                            keep = conn.write_prefill(root, rnd(L, ctx, H, D), rnd(L, ctx, H, D))
                            for rid in members:
                                conn.add_request(rid)
                            kn, vn = rnd(n, OWN, L, H, D), rnd(n, OWN, L, H, D)
                            keep += conn.commit(members, kn, vn, [range(OWN)] * n)
                            q, qc, kc, vc = rnd(n, H, R, D), rnd(n, S, H, R, D), rnd(n, S, L, H, D), rnd(n, S, L, H, D)
                            torch.cuda.synchronize()
                            meds[(name, "attend_shared")].append(timed(torch, lambda: conn.attend_shared(0, members, [root] * n, q, sm), a.reps, 2))
                            meds[(name, "attend_chunk_shared")].append(
                                timed(torch, lambda: conn.attend_chunk_shared(0, members, [root] * n, qc, kc, vc, sm), a.reps, 2))
                            del keep
                        finally:
                            lib.finalize()
                for what in ("attend_shared", "attend_chunk_shared"):
                    p, t = meds[("parent", what)], meds[("this", what)]
                    inside = abs(statistics.median(t) - statistics.median(p)) <= max(p) - min(p)
                    say(f"  {scheme} {what} {n} members x {ctx:5d} rows_per_pos {R}: parent {fig(p)} | this {fig(t)} | "
                        f"{'inside' if inside else 'OUTSIDE'} the parent's spread")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
