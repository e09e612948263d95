#!/usr/bin/env python3
"""What a tree-shaped step costs against the chain step and against one chain call per path (profiles/spec_tree_step.txt).

Batch of --seqs requests x --layers layers at --ctx stored positions plus one odd position in the tail, per pool format, S = 4 new
positions, rows_per_pos = 4 (16 query rows per kv head: one pass over the records), layer by layer:
  (a) chain          SpeckvKVConnector.attend_spec as it stands (speckv_ext_attend_fold_held)
  (b) chain as tree  the same step with parents = [-1, 0, 1, 2] (speckv_ext_attend_fold_masked with chain masks)
  (c) tree           parents = [-1, 0, 1, 1] -- a trunk of 2 with two leaves -- as ONE masked step, against the same tree as two chain
                     calls of its two paths [0, 1, 2] and [0, 1, 3]
(a) and (b) are timed --rounds times in turn; the spread of (a)'s medians over the rounds is what (b) has to be read against.
Device time between two HIP events around the layer loop of a step; clock ramp and warm-up untimed; median of --reps steps.

    python profiles/tools/spec_tree_bench.py [--schemes fp8,int4,mxfp4] [--reps 40] [--rounds 5] [--only-chain]
"""
import argparse
import json
import os
import statistics
import sys


def timed(torch, fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-chain", action="store_true", help="(a) and (b) only: a kernel trace then holds the two fold kernels on the same launch shape")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    B, L, S, R, H, D = a.seqs, a.layers, 4, 4, 8, 128
    T = a.ctx + 64
    sm = D ** -0.5
    chain, tree, paths = [-1, 0, 1, 2], [-1, 0, 1, 1], [[0, 1, 2], [0, 1, 3]]
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    # clock ramp: a second of dense work before anything is timed
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    for scheme in a.schemes.split(","):
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
            ids = list(range(1, B + 1))
            k, v = rnd(L, a.ctx + 1, H, D), rnd(L, a.ctx + 1, H, D)            # ctx stored positions and the odd one in the tail
            for rid in ids:
                conn.add_request(rid)
                conn.write_prefill(rid, k, v)
            torch.cuda.synchronize()
            k_new, v_new, q = rnd(B, S, L, H, D), rnd(B, S, L, H, D), rnd(L, B, S, H, R, D)
            step = lambda parents: [conn.attend_spec(layer, ids, q[layer], k_new, v_new, sm, parents=parents) for layer in range(L)]
            at = [torch.tensor(p, device="cuda") for p in paths]
            cut = [(q[:, :, p].contiguous(), k_new[:, p].contiguous(), v_new[:, p].contiguous()) for p in at]
            per_path = lambda: [conn.attend_spec(layer, ids, qp[layer], kp, vp, sm) for qp, kp, vp in cut for layer in range(L)]
            a_ms, b_ms = [], []
            for _ in range(a.rounds):
                a_ms.append(timed(torch, lambda: step(None), a.reps, 5))
                b_ms.append(timed(torch, lambda: step(chain), a.reps, 5))
            a_med, b_med = statistics.median(a_ms), statistics.median(b_ms)
            res = {"scheme": scheme, "seqs": B, "layers": L, "ctx": a.ctx, "S": S, "rows_per_pos": R, "reps": a.reps,
                   "a_chain_ms": [round(x, 4) for x in a_ms], "b_chain_as_tree_ms": [round(x, 4) for x in b_ms],
                   "a_median_ms": round(a_med, 4), "a_spread": round((max(a_ms) - min(a_ms)) / a_med, 4),
                   "b_median_ms": round(b_med, 4), "b_over_a": round(b_med / a_med, 4),
                   "b_within_a_spread": bool(abs(b_med - a_med) <= max(a_ms) - min(a_ms))}
            if not a.only_chain:
                c_tree = timed(torch, lambda: step(tree), a.reps, 5)
                c_paths = timed(torch, per_path, a.reps, 5)
                res.update({"c_tree_one_step_ms": round(c_tree, 4), "c_two_chain_calls_ms": round(c_paths, 4),
                            "c_tree_over_a": round(c_tree / a_med, 4), "c_tree_over_two_calls": round(c_tree / c_paths, 4)})
            print(json.dumps(res), flush=True)
            for rid in ids:
                conn.free_request(rid)
        finally:
            lib.finalize()


if __name__ == "__main__":
    main()
