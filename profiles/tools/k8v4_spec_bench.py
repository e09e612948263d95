#!/usr/bin/env python3
"""What a draft step on the decode kernel costs over the K8V4 split pool (writes profiles/k8v4_spec_step.txt).

One process, one layer timed, requests x stored positions in {256 x 2k, 256 x 8k, 8 x 32k} x (S, rows_per_pos) in {(4, 4), (2, 8), (16, 1)};
every request holds an even number of positions (no tail), the step is a causal chain.
  route a  SpeckvSplitKVConnector.attend_spec: ONE speckv_ext_attend_kv_spec (S x rows_per_pos = 16: one group)
  route b  SpeckvSplitKVConnector.attend_chunk(splits=0) with the same step: the only route before attend_spec existed
  route c  SpeckvSplitKVConnector.attend, ONE position at the same rows_per_pos: the "costs N single steps" figure
  route d  speckv_ext_attend_kv_batch at g = S x rows_per_pos followed by speckv_ext_attend_fold_masked, two calls on one stream, and
  route e  speckv_ext_attend_kv_spec itself over the same buffers: e / d is what folding inside the launch buys (a, b, c are connector
           calls and carry torch's gathers and the host's share; d and e are the bare entries)
Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians (the method of profiles/tools/shared_prefix_bench.py).
The spread (max - min of a route's rounds' medians) is printed beside every ratio's denominator as a fraction of it: the noise a
difference has to exceed.  The device's clock as torch reports it is printed before and after.

    python profiles/tools/k8v4_spec_bench.py [--shapes 256x2048,256x8192,8x32768] [--steps 4x4,2x8,16x1] [--reps 7] [--rounds 5]
                                             [--out profiles/k8v4_spec_step.txt]
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
    ap.add_argument("--steps", default="4x4,2x8,16x1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k8v4_spec_step.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    L, H, D = 2, 8, 128                                                     # (the split pool's allocations hold an even number of regions)
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
    say(f"a draft step over the K8V4 split pool: layer 0 of {L}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
        f"{datetime.date.today().isoformat()} (profiles/tools/k8v4_spec_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call); "
        f"clock at the start {clock()}")
    say("columns: a = attend_spec | b = attend_chunk(splits=0) | c = attend, one position | d = attend_kv_batch + attend_fold_masked (entries) "
        "| e = attend_kv_spec (entry) | a / b (b's spread) | a / c (c's spread) | e / d (d's spread)")
    side = torch.cuda.Stream()
    rows = []
    for n, ctx in shapes:
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            conn = SpeckvSplitKVConnector(lib, L, H, D, ctx + 64)
            rids = list(range(n))
            pk, pv = rnd(L, ctx, H, D), rnd(L, ctx, H, D)                   # (every request holds the same rows: the timing does not read values)
            keep = []
            for rid in rids:
                conn.add_request(rid)
                keep += conn.write_prefill(rid, pk, pv)
            torch.cuda.synchronize()
            reqs = [conn.requests[r] for r in rids]
            k_handles, v_handles = (np.asarray([getattr(r, x) for r in reqs], np.uint64) for x in ("k_handle", "v_handle"))
            pos_end = np.full(n, ctx, np.uint32)
            for S, R in steps:
                g = S * R
                q5, k_new, v_new = rnd(n, S, H, R, D), rnd(n, S, L, H, D), rnd(n, S, L, H, D)
                q1 = rnd(n, H, R, D)
                route_a = lambda: conn.attend_spec(0, rids, q5, k_new, v_new, sm)
                route_b = lambda: conn.attend_chunk(0, rids, q5, k_new, v_new, sm, splits=0)
                route_c = lambda: conn.attend(0, rids, q1, sm)
                meds = in_turn(torch, [route_a, route_b, route_c], a.reps, a.rounds)
                ma, mb, mc = (statistics.median(m) for m in meds)
                sb, sc = ((max(m) - min(m)) / statistics.median(m) for m in meds[1:])
                # the bare entries over the same buffers every call: one group (g <= 16)
                if g <= 16:
                    qg = q5.permute(0, 2, 1, 3, 4).reshape(n, H, g, D).contiguous()
                    kh = torch.cat([k_new[:, :, 0], k_new[:, -1:, 0]], dim=1).contiguous()          # [n][1 + S][H][D], the last slot never visible
                    vh = torch.cat([v_new[:, :, 0], v_new[:, -1:, 0]], dim=1).contiguous()
                    words = SpeckvKVConnector.tree_masks(list(range(-1, S - 1)), [0] * n)
                    masks = torch.from_numpy(np.asarray(words, np.uint32).view(np.int32)).cuda()
                    out = torch.zeros((n, H, g, D), dtype=torch.float32, device="cuda")
                    lse = torch.zeros((n, H, g), dtype=torch.float32, device="cuda")
                    ptrs = (kh.data_ptr(), vh.data_ptr(), (1 + S) * H * D, H * D, masks.data_ptr(), S, sm, out.data_ptr(), lse.data_ptr(), side.cuda_stream)

                    def route_d():
                        lib.attend_kv_batch(k_handles, v_handles, 0, qg.data_ptr(), g, pos_end, sm, out.data_ptr(), lse.data_ptr(), side.cuda_stream)
                        lib.attend_fold_masked(n, 0, H, g, R, qg.data_ptr(), *ptrs)
                    route_e = lambda: lib.attend_kv_spec(k_handles, v_handles, 0, qg.data_ptr(), g, R, pos_end, *ptrs)
                    torch.cuda.synchronize()
                    with torch.cuda.stream(side):
                        em = in_turn(torch, [route_d, route_e], a.reps, a.rounds)
                    torch.cuda.synchronize()
                    md, me = statistics.median(em[0]), statistics.median(em[1])
                    sd = (max(em[0]) - min(em[0])) / md
                    tail = f"{md:7.3f} | {me:7.3f}"
                    ratio_ed = f"{me / md:4.2f} ({sd:.3f})"
                else:
                    md = me = sd = None
                    tail, ratio_ed = "   -    |    -   ", "-"
                rows.append((n, ctx, S, R, ma / mb, sb, ma / mc, sc, None if md is None else me / md, sd))
                say(f"  {n:3d} x {ctx:5d} S {S:2d} R {R}: {ma:7.3f} | {mb:7.3f} | {mc:7.3f} | {tail} | a / b {ma / mb:4.2f} ({sb:.3f}) | a / c {ma / mc:4.2f} ({sc:.3f}) "
                    f"| e / d {ratio_ed}")
            del keep
            for rid in rids:
                conn.free_request(rid)
        except (RuntimeError, MemoryError) as e:                           # a pool too small for this shape: said, not hidden
            say(f"  {n:3d} x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
        finally:
            lib.finalize()
    if rows:
        say(f"a / b: {min(r[4] for r in rows):.2f} .. {max(r[4] for r in rows):.2f}; a / c: {min(r[6] for r in rows):.2f} .. {max(r[6] for r in rows):.2f}; e / d: "
            + (" .. ".join(f"{f(r[8] for r in rows if r[8] is not None):.2f}" for f in (min, max)) if any(r[8] is not None for r in rows) else "-"))
        slower_b = [r for r in rows if r[4] >= 1.0 - r[5]]
        say("a does not beat b beyond b's spread at: " + (", ".join(f"{n} x {ctx} S {S} R {R} ({x:.2f})" for n, ctx, S, R, x, *_ in slower_b) or "no shape"))
        not_d = [r for r in rows if r[8] is not None and r[8] >= 1.0 - r[9]]
        say("e does not beat d beyond d's spread at: " + (", ".join(f"{r[0]} x {r[1]} S {r[2]} R {r[3]} ({r[8]:.2f})" for r in not_d) or "no shape"))
    say(f"clock at the end {clock()}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
