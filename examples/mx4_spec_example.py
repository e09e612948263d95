#!/usr/bin/env python3
"""Draft and verify on an MXFP4 pool in one pass over the records: `SpeckvKVConnector.attend_spec(row_block=16)` -- up to 16 query rows per
kv head (S draft positions x rows per position) verified by ONE `speckv_ext_attend_spec_mx4` launch per layer and group
(k_attend_mx4_spec), the held rows folded inside it; no plan and no fold launch.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.  Three requests of odd and even lengths go in through
`write_prefill`; then rounds of a CHAIN of S = 4 drafts per request at 4 query rows per position: `attend_spec(row_block=16)` on both
layers, a pretended accept count per request, `commit`.

Checked in the example itself against `attend_spec()` with the same step -- the planned call (query rows in blocks of 8: every record
walked twice) and its fold launch.  Both routes quantise the query to MXFP8 per 16 channels with the same bits and read the same records;
what is left are the routes' own roundings of weights and sums, so the example asks |difference| <= 2 x (2e-3 max|v| + 1e-6), twice the
bound either route is tested against with sum p|v| <= max|v|.

    python examples/mx4_spec_example.py [--rounds 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompts=(37, 64, 130), rounds=3, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        layers, H, D, T, S, R = 2, 8, 128, 256, 4, 4
        conn = SpeckvKVConnector(lib, layers, H, D, T, "mxfp4")
        gen = torch.Generator(device="cuda"); gen.manual_seed(54)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm, keep = list(range(1, len(prompts) + 1)), D ** -0.5, []
        B = len(rids)
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, rnd(layers, n, H, D), rnd(layers, n, H, D))
        for rnd_i in range(rounds):
            q, k_new, v_new = rnd(B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            for layer in range(layers):
                one = conn.attend_spec(layer, rids, q, k_new, v_new, sm, row_block=16)
                two = conn.attend_spec(layer, rids, q, k_new, v_new, sm)
                torch.cuda.synchronize()
                worst = float((one - two).abs().max()) / (2.0 * (2e-3 * 6.0 + 1e-6))       # (|v| of randn rows stays below 6)
                if verbose:
                    print(f"round {rnd_i} layer {layer}: lengths {[conn.length(r) for r in rids]}, attend_spec(row_block=16) against attend_spec() "
                          f"{worst:.3f} of the bound")
                assert torch.isfinite(one).all() and worst <= 1.0, (rnd_i, layer, worst)
            accept = [(rnd_i + b) % S + 1 for b in range(B)]                               # the pretended verdict
            keep.append(conn.commit(rids, k_new, v_new, [list(range(n)) for n in accept]))
        torch.cuda.synchronize()
        del keep
        return rounds
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    run(rounds=ap.parse_args().rounds)
    print("ok")
