#!/usr/bin/env python3
"""What a sliding window saves a draft tree, and that the calls that were there before cost what they cost (profiles/chunk_tree_window.txt).

One process per run, one layer, a 64-node draft tree, rows_per_pos = 4, splits = 0, per pool format: requests x context in {1, 4} x
{2k, 32k}.  Per shape the stream time of
    masked   attend_chunk(parents=tree, splits=0), timed TWICE per round (masked, masked'): the unwindowed tree step, THE BASELINE
    treeW    attend_tree(tree, splits=0, window=W): the tree step of a local layer (-- in a tree without attend_tree, and under
             --skip-tree, which gives both trees the same sequence of calls: what precedes a call moves it by a percent)
    causal   attend_chunk(splits=0) of the same 64 positions as a chain
    chainW   attend_chunk(splits=0, window=W) of the same chain
Device time between two HIP events around one call; clock ramp and warm-up untimed; the variants timed IN TURN within every round, per
round the median of --reps calls, the median of the rounds' medians.

A run measures ONE source tree (--root: the repository to import; default this one) and APPENDS its rows to --out under --label.
Runs of two trees -- the parent commit and this one -- are started alternately by the caller (parent, this, parent, this), and
--summary then reads all rows of --out and appends, per shape: the spread of the parent against itself (max - min over its runs, and
masked against masked' within a run), this / parent for every call both trees have, and masked / treeW.

    python profiles/tools/chunk_tree_window_bench.py --label this [--root .] [--out profiles/chunk_tree_window.txt]
    python profiles/tools/chunk_tree_window_bench.py --summary [--out profiles/chunk_tree_window.txt]
"""
import argparse
import os
import re
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ("masked", "masked'", "treeW", "causal", "chainW")
ROW = re.compile(r"^\[(\S+)\] (\S+)\s+(\d+) x\s*(\d+):(.*)$")


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


def summary(path):
    rows = {}                                                                  # (scheme, B, ctx) -> label -> [run: [ms per name]]
    for line in open(path):
        m = ROW.match(line)
        if m:
            ms = [None if x.strip() == "--" else float(x) for x in m.group(5).split("|")]
            rows.setdefault((m.group(2), int(m.group(3)), int(m.group(4))), {}).setdefault(m.group(1), []).append(ms)
    out = ["", "summary (medians over a label's runs; spread = the parent against itself: the larger of max - min of `masked` over its runs",
           "and |masked - masked'| within a run; per call behind it: max - min of that call over the parent's runs; ratios > 1: the first is slower)"]
    for (scheme, B, ctx), by in rows.items():
        med = {lab: [None if any(r[k] is None for r in runs) else statistics.median(r[k] for r in runs) for k in range(len(NAMES))]
               for lab, runs in by.items()}
        # the tree under test: the label that has the tree call, or (runs under --skip-tree) the one that is not "parent"
        new = next((lab for lab in med if med[lab][2] is not None), None) or next((lab for lab in med if lab != "parent"), None)
        old = next((lab for lab in med if lab != new), None)
        own = by[old] if old else [r for runs in by.values() for r in runs]  # the parent against itself, where there is one
        of = lambda k: max(r[k] for r in own) - min(r[k] for r in own)
        spread = max(of(0), max(abs(r[0] - r[1]) for r in own))
        line = f"  {scheme:5s} {B} x {ctx:5d}: spread {spread:.4f} ms"
        if new and med[new][2] is not None:
            base = med[old][0] if old else med[new][0]
            gap = med[new][2] - base
            line += (f"  masked({old or new}) / treeW({new}) {base / med[new][2]:.2f}x"
                     f"  treeW - masked {gap:+.4f} ms ({'not slower' if gap <= spread else 'SLOWER beyond the spread'})")
        if new and old:
            for k in (0, 3, 4):
                d, own_k = med[new][k] - med[old][k], spread if k == 0 else of(k)
                line += f"  {NAMES[k]} {new}/{old} {med[new][k] / med[old][k]:.3f} ({d:+.4f} ms, {old} spread {own_k:.4f}: {'inside' if abs(d) <= own_k else 'BEYOND'})"
        out.append(line)
    with open(path, "a") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the source tree to measure (its package is imported)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", default="1,4")
    ap.add_argument("--ctxs", default="2048,32768")
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "chunk_tree_window.txt"))
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--skip-tree", action="store_true", help="leave treeW out: the same sequence of calls as a tree without attend_tree")
    a = ap.parse_args()
    if a.summary:
        return summary(a.out)
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    L, R, H, D, S, W = 1, 4, 8, 128, a.nodes, a.window
    sm = D ** -0.5
    ints = lambda s: [int(x) for x in s.split(",") if x]
    rng = np.random.default_rng(64)
    tree = [int(rng.integers(max(-1, j - 6), j)) for j in range(S)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def say(line):
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)           # clock ramp: dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    has_tree = hasattr(SpeckvKVConnector, "attend_tree") and not a.skip_tree
    say(f"run [{a.label}]: a {S}-node draft tree, {L} layer, rows_per_pos {R}, splits 0, W {W}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs "
        f"(profiles/tools/chunk_tree_window_bench.py, {a.rounds} rounds of {a.reps} calls, variants in turn; ms per call: " + " | ".join(NAMES) + ")")
    for scheme in a.schemes.split(","):
        for B in ints(a.seqs):
            for ctx in ints(a.ctxs):
                lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
                try:
                    conn = SpeckvKVConnector(lib, L, H, D, ctx + S + 64, scheme)
                    ids = list(range(1, B + 1))
                    k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
                    keep = []
                    for rid in ids:
                        conn.add_request(rid)
                        keep += conn.write_prefill(rid, k, v)
                    torch.cuda.synchronize()
                    del keep
                    q, kn, vn = rnd(B, S, H, R, D), rnd(B, S, L, H, D), rnd(B, S, L, H, D)
                    masked = lambda: conn.attend_chunk(0, ids, q, kn, vn, sm, parents=tree, splits=0)
                    fns = [masked, masked, (lambda: conn.attend_tree(0, ids, q, kn, vn, sm, tree, splits=0, window=W)) if has_tree else None,
                           lambda: conn.attend_chunk(0, ids, q, kn, vn, sm, splits=0), lambda: conn.attend_chunk(0, ids, q, kn, vn, sm, splits=0, window=W)]
                    meds = [[] for _ in fns]
                    for _ in range(a.rounds):
                        for m, fn in zip(meds, fns):
                            if fn is not None:
                                m.append(timed(torch, fn, a.reps, 2))
                    say(f"[{a.label}] {scheme:5s} {B} x {ctx:5d}: " + " | ".join(f"{statistics.median(m):8.4f}" if m else "   --   " for m in meds))
                    for rid in ids:
                        conn.free_request(rid)
                finally:
                    lib.finalize()


if __name__ == "__main__":
    main()
