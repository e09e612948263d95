#!/usr/bin/env python3
"""attend_chunk against the routes a caller has without it, in one process (writes profiles/chunk_prefill.txt).

Shapes, per pool format (one layer, 8 kv heads x 128):
  A   1 request  x 8k stored x a chunk of 512 positions, rows_per_pos 4
  B  16 requests x 2k stored x a chunk of 128 positions, rows_per_pos 4
  C 256 requests x 2k stored x 16 positions, rows_per_pos 1 (the small end)
Routes: attend_chunk; (a) the K and V prefix decoded to fp16 by speckv_ext_fetch_range, the new rows concatenated, torch's
scaled_dot_product_attention with the causal block as a mask; (b) at the small end only, attend_spec.  HIP events around each route on
one stream, two warm-up calls, then `reps` calls each, alternating; three repetitions of that, the median of each and the spread of the
three medians.  Reported besides the times and ratios: attend_chunk's fp16 MFMA rate (4 * rows * positions seen * 128 flop) as a
fraction of the 2.5 PFLOP/s dense fp16 peak, and the record bytes it reads per second.

    python profiles/tools/chunk_prefill_bench.py [--schemes fp8,int4,mxfp4] [--reps 5] [--out profiles/chunk_prefill.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REC_BYTES = {"fp8": 2048, "int4": 1152, "mxfp4": 1088}
SHAPES = (("A", 1, 8192, 512, 4), ("B", 16, 2048, 128, 4), ("C", 256, 2048, 16, 1))
PEAK_F16 = 2.5e15


def bench(scheme, name, B, ctx, S, R, reps, say):
    import torch
    import torch.nn.functional as F
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, L = 8, 128, 1
        T = ctx + (S + 31) // 32 * 32
        conn = SpeckvKVConnector(lib, L, H, D, T, scheme)
        ids = list(range(1, B + 1))
        k, v = torch.randn((L, ctx, H, D), device="cuda").half(), torch.randn((L, ctx, H, D), device="cuda").half()
        for rid in ids:
            conn.add_request(rid)
            conn.write_prefill(rid, k, v)
        q = torch.randn((B, S, H, R, D), device="cuda").half()
        k_new, v_new = torch.randn((B, S, L, H, D), device="cuda").half(), torch.randn((B, S, L, H, D), device="cuda").half()
        sm = D ** -0.5
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        sees = torch.ones((S, ctx + S), dtype=torch.bool, device="cuda")
        sees[:, ctx:] = torch.tril(torch.ones((S, S), dtype=torch.bool, device="cuda"))
        pages = ctx // 2

        def chunk():
            return conn.attend_chunk(0, ids, q, k_new, v_new, sm, stream=st)

        def fetch_and_torch():
            kk = torch.empty((B, ctx + S, H, D), dtype=torch.float16, device="cuda")
            vv = torch.empty((B, ctx + S, H, D), dtype=torch.float16, device="cuda")
            for b, rid in enumerate(ids):
                h = conn.requests[rid].handle
                lib.fetch_range(h, 0, pages, kk[b].data_ptr(), False, st.cuda_stream)
                lib.fetch_range(h, T // 2, pages, vv[b].data_ptr(), False, st.cuda_stream)
            kk[:, ctx:], vv[:, ctx:] = k_new[:, :, 0], v_new[:, :, 0]
            expand = lambda x: x.permute(0, 2, 1, 3)[:, :, None].expand(B, H, R, ctx + S, D).reshape(B, H * R, ctx + S, D)
            qq = q.permute(0, 2, 3, 1, 4).reshape(B, H * R, S, D)
            return F.scaled_dot_product_attention(qq, expand(kk), expand(vv), attn_mask=sees, scale=sm)

        def spec():
            return conn.attend_spec(0, ids, q, k_new, v_new, sm, stream=st)

        routes = [("attend_chunk", chunk), ("fetch_range + torch", fetch_and_torch)] + ([("attend_spec", spec)] if S <= 16 else [])

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(st)
            with torch.cuda.stream(st):
                keep = fn()
            e1.record(st)
            torch.cuda.synchronize()
            del keep
            return e0.elapsed_time(e1)

        for _, fn in routes:
            timed(fn); timed(fn)
        med = {n: [] for n, _ in routes}
        for _ in range(3):
            t = {n: [] for n, _ in routes}
            for _ in range(reps):
                for n, fn in routes:
                    t[n].append(timed(fn))
            for n, _ in routes:
                med[n].append(statistics.median(t[n]))
        m = {n: statistics.median(x) for n, x in med.items()}
        say(f"{scheme} {name}: {B} requests x {ctx} stored x {S} new positions, rows_per_pos {R}")
        for n, _ in routes:
            say(f"  {n:20s} {m[n]:9.3f} ms  (three medians {min(med[n]):.3f} .. {max(med[n]):.3f})")
        for n, _ in routes[1:]:
            spread = max(med[n]) - min(med[n])
            verdict = "attend_chunk wins" if m["attend_chunk"] <= m[n] else ("the other route wins beyond its spread" if m["attend_chunk"] - m[n] > spread else "within the spread")
            say(f"  {n} / attend_chunk = {m[n] / m['attend_chunk']:.2f}x  ({verdict})")
        seen = B * sum(ctx + j + 1 for j in range(S))                       # positions seen, summed over the query positions
        flops = 4.0 * R * H * D * seen
        blocks = B * H * ((S + 64 // R - 1) // (64 // R))
        rec = blocks * 2 * pages * REC_BYTES[scheme] / H                    # every block reads its head's eighth of the K and V records
        sec = m["attend_chunk"] * 1e-3
        say(f"  attend_chunk: {flops / sec / 1e12:.1f} TFLOP/s fp16 MFMA = {flops / sec / PEAK_F16:.3f} of the dense fp16 peak; "
            f"{rec / sec / 1e12:.3f} TB/s of record bytes")
    finally:
        lib.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_prefill.txt"))
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say("attend_chunk against fetch_range + torch attention and, at the small end, attend_spec (profiles/tools/chunk_prefill_bench.py)")
    for scheme in a.schemes.split(","):
        for name, B, ctx, S, R in SHAPES:
            if name in a.shapes.split(","):
                bench(scheme, name, B, ctx, S, R, a.reps, say)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
