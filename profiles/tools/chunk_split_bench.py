#!/usr/bin/env python3
"""What splitting the stored positions buys attend_chunk (writes profiles/chunk_split.txt).

One process, one layer, rows_per_pos = 8, per pool format: requests x context x step in {1, 4} x {2k, 8k, 32k} x {a 40-node tree, a
16-position chain, a 512-position chunk}.  Per shape: the piece counts the library's rule chooses (speckv_ext_chunk_split_plan for this
device), then the stream time of attend_chunk with splits=1 (the launch without pieces: what the library did before the split existed),
splits=0 (the rule) and forced 2 / 4 / 8 / 16 pieces, and of attend_spec where it accepts the step (chains of <= 16 positions).
Device time between two HIP events around one call; clock ramp and warm-up untimed; the variants timed IN TURN within every round,
per round the median of --reps calls, --rounds rounds, the median of the rounds' medians.  The spread (max - min) of the splits=1
rounds' medians is the noise a difference has to exceed; the last column says whether splits=0 does.

    python profiles/tools/chunk_split_bench.py [--schemes fp8,int4,mxfp4] [--reps 7] [--rounds 5] [--out profiles/chunk_split.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FORCED = (2, 4, 8, 16)


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


def tree_of(n):
    """a draft tree of n nodes as a top-k expansion leaves it: node j hangs under node (j - 1) // 2, the first is a child of the context"""
    return [-1] + [(j - 1) // 2 for j in range(1, n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", default="1,4")
    ap.add_argument("--ctxs", default="2048,8192,32768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_split.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, R, H, D = 1, 8, 8, 128
    sm = D ** -0.5
    seqs, ctxs = [int(x) for x in a.seqs.split(",")], [int(x) for x in a.ctxs.split(",")]
    steps = (("tree-40", 40, tree_of(40)), ("chain-16", 16, None), ("chunk-512", 512, None))
    T = max(ctxs) + 512 + 64
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
    say(f"attend_chunk with and without pieces: {L} layer, rows_per_pos {R}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs "
        f"(profiles/tools/chunk_split_bench.py, {a.rounds} rounds of {a.reps} calls, variants in turn; ms per call)")
    say("columns: splits=1 | splits=0 (the rule) | forced 2 | 4 | 8 | 16 | attend_spec; spread = max - min of the splits=1 rounds' medians")
    verdicts = []
    for scheme in a.schemes.split(","):
        say(f"{scheme}")
        for B in seqs:
            for ctx in ctxs:
                lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
                try:
                    conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
                    ids = list(range(1, B + 1))
                    k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
                    for rid in ids:
                        conn.add_request(rid)
                        conn.write_prefill(rid, k, v)
                    torch.cuda.synchronize()
                    for name, n, parents in steps:
                        q, kn, vn = rnd(B, n, H, R, D), rnd(B, n, L, H, D), rnd(B, n, L, H, D)
                        pieces, tpp = lib.chunk_split_plan([ctx] * B, [n] * B, R, 0)
                        call = lambda s: (lambda: conn.attend_chunk(0, ids, q, kn, vn, sm, parents=parents, splits=s))
                        fns = [call(1), call(0)] + [call(f) for f in FORCED]
                        if parents is None and n <= 16:
                            fns.append(lambda: conn.attend_spec(0, ids, q, kn, vn, sm))
                        meds = in_turn(torch, fns, a.reps, a.rounds)
                        med = [statistics.median(m) for m in meds]
                        spread = max(meds[0]) - min(meds[0])
                        if pieces[0] > 1:
                            verdict = "rule WINS" if med[0] - med[1] > spread else "rule does NOT win" if med[1] <= med[0] + spread else "rule LOSES"
                        else:
                            verdict = "one piece: same launch" if abs(med[1] - med[0]) <= spread else "one piece, BEYOND the spread"
                        verdicts.append((scheme, B, ctx, name, pieces[0], verdict))
                        cols = " | ".join(f"{m:7.3f}" for m in med[:6]) + " | " + (f"{med[6]:7.3f}" if len(med) > 6 else "   --  ")
                        say(f"  {B} x {ctx:5d} {name:9s} rule {pieces[0]:2d} x {tpp[0]:3d} tiles: {cols}   spread {spread:.3f}  "
                            f"1/0 = {med[0] / med[1]:.2f}x  {verdict}")
                    for rid in ids:
                        conn.free_request(rid)
                finally:
                    lib.finalize()
    split = [v for v in verdicts if v[4] > 1]
    say(f"shapes the rule splits: {len(split)} of {len(verdicts)}; it wins by more than the spread in {sum(v[5] == 'rule WINS' for v in split)}; "
        f"one-piece shapes beyond the spread: {sum(v[5].endswith('BEYOND the spread') for v in verdicts)}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
