#!/usr/bin/env python3
"""The split pool (K8V4: FP8 keys, MXFP4 values) next to the FP8 and MXFP4 pools (writes profiles/k8v4.txt).

One process, layer 0 of 2, rows_per_pos = 4.
  chunk   a 512-position chunk over 8k and 32k stored positions, one and four requests: SpeckvSplitKVConnector.attend_chunk (K8V4) and
          SpeckvKVConnector.attend_chunk over an FP8 and an MXFP4 pool -- the same kernel body, three instances; splits = 1 everywhere.
  decode  a 256-request step of ONE new position at 2k and 8k stored positions: K8V4 through SpeckvSplitKVConnector.attend (the batch
          decode kernel over FP8 keys and MXFP4 values, which quantises the query) and through attend_chunk (n_new = 1; splits = 1 and the
          library's rule, splits = 0) next to FP8 and MXFP4 through SpeckvKVConnector.attend -- the planned decode kernels.
  window  a 256-request step of ONE new position on a SLIDING-WINDOW layer (W = 1024) at 2k and 8k stored positions, K8V4 only, g = 8:
          (a) SpeckvSplitKVConnector.attend(window=W) -- lo on a tile bound (32 tiles a request, nothing masked) -- and attend(window=W + 15):
          lo 17 positions into its tile (33 tiles, an odd count of masked positions, a cut page); (b) attend() without a window at the same
          context; (c) attend() without a window over W + 32 stored positions, the same 33 tiles; (d) attend_chunk(window=W) with one new
          position, splits = 1 and the library's rule.  (profiles/k8v4_decode_window.txt: --sections window --out ...)
  plain   (b) alone, one line per context under --label: the yardstick against another build of the library.  Run in alternating fresh
          processes with SPECKV_LIB_PATH naming the parent commit's build and this one's, --append collecting the lines in one file.
Device time between two HIP events around one call; clock ramp and warm-up untimed; the variants of a shape timed IN TURN within every
round, per round the median of --reps calls, --rounds rounds, the median of the rounds' medians; the spread (max - min of the rounds'
medians) stands beside each figure.  Bytes per call are the records the call has to read, from the shapes: requests x stored positions x
(K bytes + V bytes per position and layer: FP8 1024, MXFP4 544); GB/s = those bytes over the time (a chunk's query blocks read them
again from the caches: not counted).

    python profiles/tools/k8v4_bench.py [--reps 5] [--rounds 3] [--sections chunk,decode] [--out profiles/k8v4.txt]
(profiles/k8v4_decode.txt: --sections decode --out profiles/k8v4_decode.txt)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REC = {"fp8": 1024 + 1024, "mxfp4": 544 + 544, "k8v4": 1024 + 544}      # record bytes per stored position of one layer, K + V


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk-ctxs", default="8192,32768")
    ap.add_argument("--chunk-seqs", default="1,4")
    ap.add_argument("--decode-ctxs", default="2048,8192")
    ap.add_argument("--decode-seqs", type=int, default=256)
    ap.add_argument("--sections", default="chunk,decode")
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--append", action="store_true", help="keep what --out already holds and add to it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k8v4.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    L, R, H, D, S = 2, 4, 8, 128, 512
    sm = D ** -0.5
    lines = []
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.append and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()

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

    def pools(lib, T, B, ctx):
        """the three pools with the same prompt in every request: {name: (connector, ids)}"""
        k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
        made = {}
        for name in ("k8v4", "fp8", "mxfp4"):
            conn = SpeckvSplitKVConnector(lib, L, H, D, T) if name == "k8v4" else SpeckvKVConnector(lib, L, H, D, T, name)
            ids = list(range(1, B + 1))
            for rid in ids:
                conn.add_request(rid)
                conn.write_prefill(rid, k, v)
            made[name] = (conn, ids)
        torch.cuda.synchronize()
        return made

    def report(what, names, meds, nbytes):
        med = [statistics.median(m) for m in meds]
        for name, m, rounds_ in zip(names, med, meds):
            say(f"  {what:22s} {name:18s} {m:8.3f} ms  spread {max(rounds_) - min(rounds_):.3f}  {nbytes[name.split()[0]] / 1e6:9.1f} MB of records  "
                f"{nbytes[name.split()[0]] / (m * 1e-3) / 1e9:7.1f} GB/s")
        return dict(zip(names, med))

    sections = a.sections.split(",")
    if sections != ["plain"]:
        say(f"K8V4 split pool next to FP8 and MXFP4: layer 0 of {L}, rows_per_pos {R}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs "
            f"(profiles/tools/k8v4_bench.py, {a.rounds} rounds of {a.reps} calls, variants in turn; median of the rounds' medians)")
    if "chunk" in sections:
        say(f"chunk: {S} new positions per request through attend_chunk, splits = 1")
    for B in [int(s) for s in a.chunk_seqs.split(",")] if "chunk" in sections else []:
        for ctx in [int(c) for c in a.chunk_ctxs.split(",")]:
            lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
            try:
                made = pools(lib, ctx + S + 32, B, ctx)
                q, kn, vn = rnd(B, S, H, R, D), rnd(B, S, L, H, D), rnd(B, S, L, H, D)
                names = ["k8v4", "fp8", "mxfp4"]
                fns = [(lambda c, ids: lambda: c.attend_chunk(0, ids, q, kn, vn, sm))(*made[n]) for n in names]
                got = report(f"{B} x {ctx:5d} + {S}", names, in_turn(torch, fns, a.reps, a.rounds), {n: B * ctx * REC[n] for n in names})
                say(f"  {'':22s} k8v4 / fp8 = {got['k8v4'] / got['fp8']:.3f} of the time ({REC['k8v4'] / REC['fp8']:.3f} of the bytes), "
                    f"k8v4 / mxfp4 = {got['k8v4'] / got['mxfp4']:.3f} ({REC['k8v4'] / REC['mxfp4']:.3f} of the bytes)")
            finally:
                lib.finalize()
    B = a.decode_seqs
    if "decode" in sections:
        say(f"decode: {B} requests, ONE new position each; K8V4 through attend (the batch decode kernel) and through attend_chunk (n_new = 1), "
            f"FP8 and MXFP4 through attend (the planned decode kernels)")
    for ctx in [int(c) for c in a.decode_ctxs.split(",")] if "decode" in sections else []:
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            made = pools(lib, ctx + 32, B, ctx)
            q, kn, vn = rnd(B, 1, H, R, D), rnd(B, 1, L, H, D), rnd(B, 1, L, H, D)
            qd = q[:, 0].contiguous()
            split, ids = made["k8v4"]
            fp8, _ = made["fp8"]
            mx4, _ = made["mxfp4"]
            names = ["k8v4 attend", "k8v4 chunk splits=1", "k8v4 chunk splits=0", "fp8 chunk splits=1", "fp8 attend", "mxfp4 attend"]
            fns = [lambda: split.attend(0, ids, qd, sm), lambda: split.attend_chunk(0, ids, q, kn, vn, sm), lambda: split.attend_chunk(0, ids, q, kn, vn, sm, splits=0),
                   lambda: fp8.attend_chunk(0, ids, q, kn, vn, sm), lambda: fp8.attend(0, ids, qd, sm), lambda: mx4.attend(0, ids, qd, sm)]
            got = report(f"{B} x {ctx:5d} + 1", names, in_turn(torch, fns, a.reps, a.rounds), {n: B * ctx * REC[n] for n in REC})
            best = min(got["k8v4 chunk splits=1"], got["k8v4 chunk splits=0"])
            say(f"  {'':22s} k8v4 chunk route / fp8 attend = {best / got['fp8 attend']:.2f} x the time at {REC['k8v4'] / REC['fp8']:.3f} of the bytes; "
                f"fp8 chunk route / fp8 attend = {got['fp8 chunk splits=1'] / got['fp8 attend']:.2f} x")
            say(f"  {'':22s} k8v4 attend / k8v4 chunk route = {got['k8v4 attend'] / best:.3f} of the time; k8v4 attend / fp8 attend = "
                f"{got['k8v4 attend'] / got['fp8 attend']:.3f} ({REC['k8v4'] / REC['fp8']:.3f} of the bytes); k8v4 attend / mxfp4 attend = "
                f"{got['k8v4 attend'] / got['mxfp4 attend']:.3f} ({REC['k8v4'] / REC['mxfp4']:.3f} of the bytes)")
        finally:
            lib.finalize()

    def split_pool(lib, T, B, ctx):
        """a split pool of B requests with the same prompt of ctx positions"""
        k, v = rnd(L, ctx, H, D), rnd(L, ctx, H, D)
        conn = SpeckvSplitKVConnector(lib, L, H, D, T)
        ids = list(range(1, B + 1))
        for rid in ids:
            conn.add_request(rid)
            conn.write_prefill(rid, k, v)
        torch.cuda.synchronize()
        return conn, ids

    W, G = a.window, 8
    if "window" in sections:
        say(f"window: {B} requests, ONE new position each on a sliding-window layer, W = {W}, g = {G}; K8V4 through attend(window=W) (k_attend_k8v4<true>), "
            f"attend() and attend_chunk(window=W, n_new = 1, rows_per_pos = {G}); MB of records = what the call has to read")
    for ctx in [int(c) for c in a.decode_ctxs.split(",")] if "window" in sections else []:
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            split, ids = split_pool(lib, ctx + 32, B, ctx)
            short, sids = split_pool(lib, W + 64, B, W + 32)
            q, kn, vn = rnd(B, 1, H, G, D), rnd(B, 1, L, H, D), rnd(B, 1, L, H, D)
            qd = q[:, 0].contiguous()
            tiles = lambda w: SpeckvKVConnector.decode_window_range(ctx, w)[2] * 2
            names = [f"(a) attend W={W}", f"(a) attend W={W + 15}", "(b) attend", f"(c) attend ctx={W + 32}", "(d) chunk splits=1", "(d) chunk splits=0"]
            fns = [lambda: split.attend(0, ids, qd, sm, window=W), lambda: split.attend(0, ids, qd, sm, window=W + 15), lambda: split.attend(0, ids, qd, sm),
                   lambda: short.attend(0, sids, qd, sm), lambda: split.attend_chunk(0, ids, q, kn, vn, sm, window=W),
                   lambda: split.attend_chunk(0, ids, q, kn, vn, sm, window=W, splits=0)]
            walked = [tiles(W), tiles(W + 15), ctx, W + 32, tiles(W), tiles(W)]
            meds = in_turn(torch, fns, a.reps, a.rounds)
            got = {}
            for name, rounds_, pos in zip(names, meds, walked):
                got[name] = statistics.median(rounds_)
                say(f"  {B} x {ctx:5d} + 1  {name:24s} {got[name]:8.3f} ms  spread {max(rounds_) - min(rounds_):.3f}  {pos // 32:4d} tiles a request  "
                    f"{B * pos * REC['k8v4'] / 1e6:8.1f} MB of records  {B * pos * REC['k8v4'] / (got[name] * 1e-3) / 1e9:7.1f} GB/s")
            a32, a33, b, c33 = got[f"(a) attend W={W}"], got[f"(a) attend W={W + 15}"], got["(b) attend"], got[f"(c) attend ctx={W + 32}"]
            d = min(got["(d) chunk splits=1"], got["(d) chunk splits=0"])
            say(f"  {'':16s} (a) / (b) = {a32 / b:.3f} and {a33 / b:.3f} of the unwindowed step's time; (a) / (d) = {a32 / d:.3f} and "
                f"{a33 / d:.3f} of the chunk route's; (a) / (c) at 33 tiles each = {a33 / c33:.3f} (the mask and the shifted start)")
        finally:
            lib.finalize()
    if "plain" in sections:
        for ctx in [int(c) for c in a.decode_ctxs.split(",")]:
            lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
            try:
                split, ids = split_pool(lib, ctx + 32, B, ctx)
                qd = rnd(B, H, G, D)
                rounds_ = in_turn(torch, [lambda: split.attend(0, ids, qd, sm)], a.reps, a.rounds)[0]
                say(f"  {B} x {ctx:5d} + 1  (b) attend, {a.label:12s} {statistics.median(rounds_):8.3f} ms  spread {max(rounds_) - min(rounds_):.3f}  "
                    f"rounds {' '.join(f'{m:.3f}' for m in rounds_)}")
            finally:
                lib.finalize()


if __name__ == "__main__":
    main()
