#!/usr/bin/env python3
"""What a step of several positions costs against the single-position steps it replaces (profiles/spec_step.txt).

Batch of --seqs requests x --layers layers at --ctx stored positions plus one odd position in the tail, per pool format:
  one-position step   SpeckvKVConnector.attend (with the tail), layer by layer: what a caller had before attend_spec; a step of S
                      positions cost S of these
  attend_spec         S = 4 new positions, rows_per_pos = 4 (16 query rows per kv head: one pass over the records) and rows_per_pos = 8
                      (two groups, two passes), layer by layer, and all layers in one attend_spec_layers call
Device time between two HIP events around the layer loop of a step; clock ramp and warm-up untimed; median of --reps steps.
--tree DIR imports the package from another checkout (the parent commit, built there) to take its one-position step in the
same session on the same device; a tree without attend_spec reports the one-position step only.

    python profiles/tools/spec_step_bench.py [--tree DIR] [--schemes fp8,int4,mxfp4] [--reps 60]
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
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--draft", type=int, default=4)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    B, L, S, H, D = a.seqs, a.layers, a.draft, 8, 128
    T = a.ctx + 64
    sm = D ** -0.5
    have_spec = hasattr(SpeckvKVConnector, "attend_spec")
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
            res = {"label": a.label, "scheme": scheme, "seqs": B, "layers": L, "ctx": a.ctx, "reps": a.reps}
            q1 = rnd(L, B, H, 4, D)
            med, best = timed(torch, lambda: [conn.attend(layer, ids, q1[layer], sm) for layer in range(L)], a.reps, 10)
            res["one_position_step_ms"] = round(med, 4); res["one_position_step_min_ms"] = round(best, 4)
            res[f"{S}_one_position_steps_ms"] = round(S * med, 4)
            if have_spec:
                k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
                for rpp in (4, 8):
                    q = rnd(L, B, S, H, rpp, D)
                    med, best = timed(torch, lambda: [conn.attend_spec(layer, ids, q[layer], k_new, v_new, sm) for layer in range(L)], a.reps, 10)
                    res[f"attend_spec_S{S}_rows{rpp}_ms"] = round(med, 4); res[f"attend_spec_S{S}_rows{rpp}_min_ms"] = round(best, 4)
                    med, best = timed(torch, lambda: conn.attend_spec_layers(0, L, ids, q, k_new, v_new, sm), a.reps, 10)
                    res[f"attend_spec_layers_S{S}_rows{rpp}_ms"] = round(med, 4)
                one, two = res[f"attend_spec_S{S}_rows4_ms"], res[f"attend_spec_S{S}_rows8_ms"]
                res["one_pass_under_two_steps"] = bool(one < 2 * res["one_position_step_ms"])
                res["two_passes_under_two_one_pass_calls_plus_10pct"] = bool(two < 2.2 * one)
            print(json.dumps(res), flush=True)
            for rid in ids:
                conn.free_request(rid)
        finally:
            lib.finalize()


if __name__ == "__main__":
    main()
