#!/usr/bin/env python3
"""What the tree form of attend_chunk costs (writes profiles/chunk_tree.txt).

Batch of --seqs requests x --layers layers at --ctx stored positions, per pool format, rows_per_pos = 8 (8 kv heads x 8 query heads
each: the 70B shape), layer by layer, in one process:
  (a) masked against causal   attend_chunk(parents = a chain) -- speckv_ext_attend_chunk_masked with chain words -- against attend_chunk
                              without parents on the same inputs, 16 nodes, timed in turn.  The mask adds one dword per lane and held
                              tile and one AND per score; the expectation is equality within the causal call's own spread.
  (b) one masked chunk call against attend_spec(parents=...) for a 16-node tree (the largest the old route takes: 8 groups of 2 nodes, 8
                              passes over the records), timed in turn; and the chunk call alone at 32 and 64 nodes.
Device time between two HIP events around the layer loop of a step; clock ramp and warm-up untimed; per round the median of --reps
steps, --rounds rounds, the median of the rounds' medians and their spread (max - min).

    python profiles/tools/chunk_tree_bench.py [--schemes fp8,int4,mxfp4] [--reps 10] [--rounds 5] [--out profiles/chunk_tree.txt]
"""
import argparse
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


def shown(meds):
    return f"{statistics.median(meds):9.3f} ms  (the rounds' medians {min(meds):.3f} .. {max(meds):.3f}, spread {max(meds) - min(meds):.3f})"


def tree_of(n):
    """a draft tree of n nodes as a top-k expansion leaves it: node j hangs under node (j - 1) // 2, the first is a child of the context"""
    return [-1] + [(j - 1) // 2 for j in range(1, n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_tree.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    B, L, R, H, D = a.seqs, a.layers, 8, 8, 128
    T = a.ctx + 64
    sm = D ** -0.5
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
    say(f"attend_chunk under a tree mask: {B} requests x {L} layers x {a.ctx} stored positions, rows_per_pos {R} "
        f"(profiles/tools/chunk_tree_bench.py, {a.rounds} rounds of {a.reps} steps, a step = the {L} layers' calls)")
    for scheme in a.schemes.split(","):
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
            ids = list(range(1, B + 1))
            k, v = rnd(L, a.ctx, H, D), rnd(L, a.ctx, H, D)
            for rid in ids:
                conn.add_request(rid)
                conn.write_prefill(rid, k, v)
            torch.cuda.synchronize()
            k_new, v_new, q = rnd(B, 64, L, H, D), rnd(B, 64, L, H, D), rnd(L, B, 64, H, R, D)
            cut = {n: (q[:, :, :n].contiguous(), k_new[:, :n].contiguous(), v_new[:, :n].contiguous()) for n in (16, 32, 64)}

            def chunk(n, parents):
                qn, kn, vn = cut[n]
                return lambda: [conn.attend_chunk(layer, ids, qn[layer], kn, vn, sm, parents=parents) for layer in range(L)]

            def spec(n, parents):
                qn, kn, vn = cut[n]
                return lambda: [conn.attend_spec(layer, ids, qn[layer], kn, vn, sm, parents=parents) for layer in range(L)]
            say(f"{scheme}")
            causal, masked = in_turn(torch, [chunk(16, None), chunk(16, list(range(-1, 15)))], a.reps, a.rounds)
            c, m = statistics.median(causal), statistics.median(masked)
            spread = max(causal) - min(causal)
            say(f"  (a) 16 positions, causal entry            {shown(causal)}")
            say(f"      16 positions, masked entry, chain     {shown(masked)}")
            say(f"      masked / causal = {m / c:.4f}; the causal call's spread is {spread / c:.4f} of its median: "
                f"{'within it' if abs(m - c) <= spread else 'BEYOND it'}")
            one, old = in_turn(torch, [chunk(16, tree_of(16)), spec(16, tree_of(16))], a.reps, a.rounds)
            say(f"  (b) 16-node tree, one masked chunk call    {shown(one)}")
            say(f"      16-node tree, attend_spec(parents)     {shown(old)}")
            say(f"      attend_spec(parents) / masked chunk = {statistics.median(old) / statistics.median(one):.2f}x")
            for n in (32, 64):
                (alone,) = in_turn(torch, [chunk(n, tree_of(n))], a.reps, a.rounds)
                say(f"      {n}-node tree, one masked chunk call    {shown(alone)}")
            for rid in ids:
                conn.free_request(rid)
        finally:
            lib.finalize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
