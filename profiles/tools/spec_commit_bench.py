#!/usr/bin/env python3
"""What committing a multi-position step costs: SpeckvKVConnector.commit (one speckv_ext_write_pairs launch, rows gathered by the
encoder) against append_tokens (torch-built page images, one write call per pair index) -- profiles/spec_commit.txt.

Two connectors on one library in ONE process, --seqs requests x --layers layers each, half of them at --ctx stored positions and
half at --ctx + 1 (odd and even lengths mixed).  Every call commits S = --draft new positions' accepted prefixes, the accept counts
drawn 0..S per request (the same draw for both connectors), commit and append_tokens alternating and swapping who goes first.
Two figures per call, wall clock:
  host      the call itself, the stream idle before it
  passed    from the call until the stream has passed the writes (stream.synchronize() returned)
Per repeat the median over --calls calls; --repeats repeats.  The claim to read off: commit is not slower than append_tokens by
more than the spread (max - min) of append_tokens' own medians, on either figure.

    python profiles/tools/spec_commit_bench.py [--schemes fp8,int4,mxfp4] [--calls 20] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--schemes", default="fp8,int4,mxfp4")
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--draft", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    B, L, S, H, D = a.seqs, a.layers, a.draft, 8, 128
    n_calls = a.warm + a.calls * a.repeats
    T = (a.ctx + 1 + n_calls * S + 31) // 32 * 32
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
    x = torch.randn((4096, 4096), device="cuda", dtype=torch.float16)           # clock ramp
    for _ in range(200):
        x = (x @ x).clamp_(-1, 1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for scheme in a.schemes.split(","):
        lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
        try:
            conns = {"commit": SpeckvKVConnector(lib, L, H, D, T, scheme), "append_tokens": SpeckvKVConnector(lib, L, H, D, T, scheme)}
            ids = {"commit": list(range(1, B + 1)), "append_tokens": list(range(B + 1, 2 * B + 1))}
            k, v = rnd(L, a.ctx + 1, H, D), rnd(L, a.ctx + 1, H, D)
            for name, conn in conns.items():
                for i, rid in enumerate(ids[name]):
                    conn.add_request(rid)
                    n = a.ctx + (i & 1)
                    conn.write_prefill(rid, k[:, :n], v[:, :n])
            torch.cuda.synchronize()
            k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
            rng = np.random.default_rng(7)
            run = {
                "commit": lambda n_accept: conns["commit"].commit(ids["commit"], k_new, v_new, [list(range(n)) for n in n_accept], stream=st),
                "append_tokens": lambda n_accept: conns["append_tokens"].append_tokens(ids["append_tokens"], k_new, v_new, n_accept, stream=st),
            }
            host = {name: [] for name in run}
            passed = {name: [] for name in run}
            with torch.cuda.stream(st):
                for call in range(n_calls):
                    n_accept = [int(n) for n in rng.integers(0, S + 1, B)]
                    for name in (("commit", "append_tokens") if call & 1 else ("append_tokens", "commit")):
                        st.synchronize()
                        t0 = time.perf_counter()
                        keep = run[name](n_accept)
                        t1 = time.perf_counter()
                        st.synchronize()
                        t2 = time.perf_counter()
                        del keep
                        if call >= a.warm:
                            host[name].append((t1 - t0) * 1e3); passed[name].append((t2 - t0) * 1e3)
            assert all(conns["commit"].length(x) == conns["append_tokens"].length(y) for x, y in zip(ids["commit"], ids["append_tokens"]))
            res = {"scheme": scheme, "seqs": B, "layers": L, "ctx": a.ctx, "S": S, "calls_per_repeat": a.calls, "repeats": a.repeats}
            for fig, data in (("host_ms", host), ("passed_ms", passed)):
                med = {name: [statistics.median(data[name][r * a.calls:(r + 1) * a.calls]) for r in range(a.repeats)] for name in run}
                spread = max(med["append_tokens"]) - min(med["append_tokens"])
                c, t = statistics.median(med["commit"]), statistics.median(med["append_tokens"])
                res[fig] = {"commit_medians": [round(m, 4) for m in med["commit"]], "append_tokens_medians": [round(m, 4) for m in med["append_tokens"]],
                            "commit": round(c, 4), "append_tokens": round(t, 4), "append_tokens_spread": round(spread, 4),
                            "commit_over_append_tokens": round(c / t, 3), "commit_not_slower_beyond_spread": bool(c - t <= spread)}
            print(json.dumps(res), flush=True)
        finally:
            lib.finalize()


if __name__ == "__main__":
    main()
