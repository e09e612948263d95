#!/usr/bin/env python3
"""The split pool's decode step of several layers in one call (SpeckvSplitKVConnector.attend_layers, speckv_ext_attend_kv_layers) on an MI355X,
against the per-layer route (one SpeckvSplitKVConnector.attend per layer: a batch call and, with odd lengths, a tail fold behind each) and
beside the FP8 connector's attend_layers on the same shapes.  Whole steps of L layers, device events around the step's calls, the routes in
turn within every round, in one process; per route the median of the rounds' medians and the spread of the rounds.

Each shape first with every length even, then -- after a commit of one position to every second request -- with half the lengths odd.

    python profiles/tools/k8v4_layers_bench.py [--shapes 256x2048,256x8192,8x32768] [--layers 8] [--out profiles/k8v4_layers.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from k8v4_bench import REC, in_turn                                            # noqa: E402  (the timing loop of the other K8V4 tools)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="256x2048,256x8192,8x32768")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--g", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k8v4_layers.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    L, G, H, D = a.layers, a.g, 8, 128
    sm = D ** -0.5
    lines = []
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def say(line):
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)           # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    say(f"K8V4 decode step of {L} layers, g = {G}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs: attend_layers (one call) against {L} x attend "
        f"(a batch call per layer, a tail fold behind it while lengths are odd), the FP8 connector's attend_layers beside them "
        f"(profiles/tools/k8v4_layers_bench.py, {a.rounds} rounds of {a.reps} steps, routes in turn; median of the rounds' medians, spread of the rounds)")
    for shape in a.shapes.split(","):
        B, ctx = (int(s) for s in shape.split("x"))
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
            split, fp8 = SpeckvSplitKVConnector(lib, L, H, D, ctx + 32), SpeckvKVConnector(lib, L, H, D, ctx + 32, "fp8")
            ids, keep = list(range(1, B + 1)), []
            for conn in (split, fp8):
                for rid in ids:
                    conn.add_request(rid)
                    keep.append(conn.write_prefill(rid, k, v))
            torch.cuda.synchronize()
            q = rnd(L, B, H, G, D)
            names = ["k8v4 attend_layers", f"k8v4 {L} x attend", "fp8 attend_layers"]
            fns = [lambda: split.attend_layers(0, L, ids, q, sm), lambda: [split.attend(layer, ids, q[layer], sm) for layer in range(L)],
                   lambda: fp8.attend_layers(0, L, ids, q, sm)]
            for lengths in ("all lengths even", "half the lengths odd"):
                if lengths != "all lengths even":
                    kn, vn, acc = rnd(B, 1, L, H, D), rnd(B, 1, L, H, D), [b & 1 for b in range(B)]
                    keep += [split.commit(ids, kn, vn, acc), fp8.commit(ids, kn, vn, [list(range(n)) for n in acc])]
                    torch.cuda.synchronize()
                both = torch.stack([fns[0](), torch.stack(fns[1]())])
                apart = float((both[0] - both[1]).abs().max())                  # the two routes on the same inputs, at the size that is timed
                meds = in_turn(torch, fns, a.reps, a.rounds)
                got = {}
                for name, rounds_ in zip(names, meds):
                    got[name] = statistics.median(rounds_)
                    nbytes = L * B * ctx * REC[name.split()[0]]
                    say(f"  {B:3d} x {ctx:5d}  {lengths:20s} {name:20s} {got[name]:8.3f} ms  spread {max(rounds_) - min(rounds_):.3f}  "
                        f"{nbytes / 1e6:9.1f} MB of records  {nbytes / (got[name] * 1e-3) / 1e9:7.1f} GB/s")
                say(f"  {'':34s} attend_layers / {L} x attend = {got[names[0]] / got[names[1]]:.3f} of the time; k8v4 attend_layers / fp8 attend_layers = "
                    f"{got[names[0]] / got[names[2]]:.3f} ({REC['k8v4'] / REC['fp8']:.3f} of the bytes); the two k8v4 routes differ by at most {apart:.2e}")
            del keep
        finally:
            lib.finalize()


if __name__ == "__main__":
    main()
