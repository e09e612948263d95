#!/usr/bin/env python3
"""What reading a shared prefix once buys a decode step over the K8V4 split pool (writes profiles/k8v4_shared_prefix.txt).

The method of profiles/tools/shared_prefix_bench.py, unchanged: one process, one layer timed, members x prefix x rows_per_pos in
{16, 64, 256} x {2k, 8k, 32k} x {1, 4}; every member holds 64 positions of its own behind the prefix.
  route A  copies + attend: every member of the split pool holds prefix + its own 64 positions and the step is
           SpeckvSplitKVConnector.attend -- the only route before attend_shared existed, unchanged
  route B  SpeckvSplitKVConnector.attend_shared: the members hold their own 64 positions only, the step is attend + ONE
           speckv_ext_attend_prefix_fold_kv over the prefix's FP8 keys and MXFP4 values
  route C  SpeckvKVConnector.attend_shared over an FP8 pool at the same shapes in the same process (attend + ONE
           speckv_ext_attend_prefix_fold): the walk B's walk is measured against
Device time between two HIP events around one call; clock ramp and warm-up untimed; the routes timed IN TURN within every round, per
round the median of --reps calls, --rounds rounds, the median of the rounds' medians.  The spread (max - min) of route A's rounds'
medians is the noise a difference has to exceed; route C's own spread is printed beside B / C.  B and C are whole steps: their own
parts differ too (the split pool's attend stages its descriptors per call, the FP8 pool's goes through its plan), so the two FOLD
entries are timed by themselves as well, in turn on a stream of their own over the same members, prefix and query
(speckv_ext_attend_prefix_fold_kv against speckv_ext_attend_prefix_fold, n_splits 0): the last column.  The last lines give the
crossover of B against A per prefix length -- the smallest member count from which B is faster than A by more than that spread --
and the ranges of B / C and of the folds' ratio.  Pool bytes are arithmetic, not measured: B stores (members - 1) x prefix / 2 x 3136 B per layer less than A.

    python profiles/tools/k8v4_shared_prefix_bench.py [--members 16,64,256] [--ctxs 2048,8192,32768] [--rpps 1,4] [--reps 7]
                                                      [--rounds 5] [--out profiles/k8v4_shared_prefix.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shared_prefix_bench import OWN, in_turn                                # the method, unchanged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="16,64,256")
    ap.add_argument("--ctxs", default="2048,8192,32768")
    ap.add_argument("--rpps", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k8v4_shared_prefix.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    L, H, D = 2, 8, 128                                                     # (the split pool's allocations hold an even number of regions)
    sm = D ** -0.5
    counts, ctxs, rpps = ([int(x) for x in s.split(",")] for s in (a.members, a.ctxs, a.rpps))
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)       # clock ramp: a second of dense work before anything is timed
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    say(f"a decode step over a shared prefix, K8V4 split pool: layer 0 of {L}, {OWN} own positions per member, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs, {datetime.date.today().isoformat()} "
        f"(profiles/tools/k8v4_shared_prefix_bench.py, {a.rounds} rounds of {a.reps} calls, routes in turn; ms per call)")
    say("columns: A = K8V4 copies + attend | B = K8V4 attend_shared | C = FP8 attend_shared | spread = max - min of A's rounds' medians | A / B "
        "| B / C (spread of C's rounds' medians as a fraction of C) | the fold entries alone, K8V4 / FP8 = ratio (spread of FP8's as a fraction)")
    wins, ratios, folds = {}, [], []
    import numpy as np
    side = torch.cuda.Stream()
    for ctx in ctxs:
        T = ctx + OWN + 64
        for n in counts:
            lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
            try:
                split = SpeckvSplitKVConnector(lib, L, H, D, T)
                fp8 = SpeckvKVConnector(lib, L, H, D, T, "fp8")
                root, members, copies = 1, list(range(1000, 1000 + n)), list(range(5000, 5000 + n))
                root8, members8 = 2, list(range(10000, 10000 + n))
                pk, pv = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
                ok, ov = rnd(L, OWN, H, D), rnd(L, OWN, H, D)               # (every member's own rows are the same rows: the timing does not read values)
                fk, fv = torch.cat([pk, ok], dim=1), torch.cat([pv, ov], dim=1)
                split.add_request(root)
                keep = split.write_prefill(root, pk, pv)
                fp8.add_request(root8)
                keep += fp8.write_prefill(root8, pk, pv)
                for rid, full, rid8 in zip(members, copies, members8):
                    split.add_request(rid)
                    keep += split.write_prefill(rid, ok, ov)
                    split.add_request(full)
                    keep += split.write_prefill(full, fk, fv)
                    fp8.add_request(rid8)
                    keep += fp8.write_prefill(rid8, ok, ov)
                torch.cuda.synchronize()
                for R in rpps:
                    q = rnd(n, H, R, D)
                    route_a = lambda: split.attend(0, copies, q, sm)
                    route_b = lambda: split.attend_shared(0, members, [root] * n, q, sm)
                    route_c = lambda: fp8.attend_shared(0, members8, [root8] * n, q, sm)
                    meds = in_turn(torch, [route_a, route_b, route_c], a.reps, a.rounds)
                    ma, mb, mc = (statistics.median(m) for m in meds)
                    spread, spread_c = max(meds[0]) - min(meds[0]), max(meds[2]) - min(meds[2])
                    verdict = "B WINS" if ma - mb > spread else "B not slower" if mb <= ma + spread else "B SLOWER"
                    wins.setdefault((ctx, R), []).append((n, verdict == "B WINS"))
                    ratios.append((mb / mc, spread_c / mc, n, ctx, R))
                    # the two fold entries by themselves: the same arrays every call (a fold into a buffer that was folded before
                    # reads and writes the same bytes)
                    out, lse = torch.zeros((n, H, R, D), dtype=torch.float32, device="cuda"), torch.zeros((n, H, R), dtype=torch.float32, device="cuda")
                    first, lens, ones = np.asarray([0, n], np.uint32), np.full(n, ctx, np.uint32), np.ones(n, np.uint32)
                    kh, vh = (np.asarray([getattr(split.requests[root], x)], np.uint64) for x in ("k_handle", "v_handle"))
                    h8 = np.asarray([fp8.requests[root8].handle], np.uint64)
                    fold_kv = lambda: lib.attend_prefix_fold_kv(kh, vh, first, 0, q.data_ptr(), 1, R, lens, ones, None, 0, 0, 0, sm, out.data_ptr(),
                                                                lse.data_ptr(), side.cuda_stream)
                    fold_8 = lambda: lib.attend_prefix_fold(h8, first, 0, q.data_ptr(), 1, R, lens, ones, 0, sm, out.data_ptr(), lse.data_ptr(),
                                                            side.cuda_stream)
                    torch.cuda.synchronize()
                    with torch.cuda.stream(side):
                        fm = in_turn(torch, [fold_kv, fold_8], a.reps, a.rounds)
                    torch.cuda.synchronize()
                    fk_, f8_ = statistics.median(fm[0]), statistics.median(fm[1])
                    folds.append((fk_ / f8_, (max(fm[1]) - min(fm[1])) / f8_, n, ctx, R))
                    say(f"  {n:3d} members x {ctx:5d} rows_per_pos {R}: {ma:7.3f} | {mb:7.3f} | {mc:7.3f} | spread {spread:.3f} | {ma / mb:5.2f}x  {verdict} "
                        f"| B / C {mb / mc:4.2f} ({spread_c / mc:.3f}) | {fk_:6.3f} / {f8_:6.3f} = {fk_ / f8_:4.2f} ({folds[-1][1]:.3f})")
                del keep
                for rid in members + copies + [root]:
                    split.free_request(rid)
                for rid in members8 + [root8]:
                    fp8.free_request(rid)
            except (RuntimeError, MemoryError) as e:                       # a pool too small for this many copies: said, not hidden
                say(f"  {n:3d} members x {ctx:5d}: NOT MEASURED ({type(e).__name__}: {e})")
            finally:
                lib.finalize()
    say("crossover of B against A (the smallest member count from which B wins by more than A's spread, at every larger count measured):")
    for (ctx, R), rows in wins.items():
        first = None
        for n, won in sorted(rows, reverse=True):
            if not won:
                break
            first = n
        say(f"  prefix {ctx:5d} rows_per_pos {R}: {'none measured' if first is None else first}")
    if ratios:
        over = [r for r in ratios if r[0] > 1.0 + r[1]]
        say(f"B / C: {min(r[0] for r in ratios):.2f} .. {max(r[0] for r in ratios):.2f} over {len(ratios)} shapes; above 1.00 + C's spread at {len(over)}: "
            + ", ".join(f"{n} x {ctx} rpp {R} ({b:.2f})" for b, _, n, ctx, R in over))
    if folds:
        over = [r for r in folds if r[0] > 1.0 + r[1]]
        say(f"the fold entries alone, K8V4 / FP8: {min(r[0] for r in folds):.2f} .. {max(r[0] for r in folds):.2f} over {len(folds)} shapes; above 1.00 + "
            f"FP8's spread at {len(over)}: " + ", ".join(f"{n} x {ctx} rpp {R} ({b:.2f})" for b, _, n, ctx, R in over))
    say("pool bytes (arithmetic, not measured): B stores (members - 1) x prefix / 2 x 3136 B per layer less than A -- "
        + ", ".join(f"{n} x {ctx}: {(n - 1) * (ctx // 2) * 3136 / 2 ** 20:.0f} MiB" for ctx in ctxs for n in counts))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
