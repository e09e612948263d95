#!/usr/bin/env python3
"""Draft and verify on an FP8 pool of a model that interleaves LOCAL and GLOBAL attention: `SpeckvKVConnector.attend_spec(window=W)` --
the draft positions of every request verified on the decode kernel on the sliding-window layers too, ONE `speckv_ext_attend_spec_window`
launch per layer and group (k_attend_fp8_spec), no plan and no fold launch.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.  Layer 0 is a local layer (window W = 40), layer 1 a
global one.  Three requests of odd and even lengths go in through `write_prefill`; then rounds of a CHAIN of S = 4 drafts per request:
`attend_spec(window=W)` on layer 0, `attend_spec()` on layer 1, a pretended accept count per request, `commit`.

Checked in the example itself against `attend_tree(window=W)` / `attend_tree()` with the same step -- the chunk walk, until now the only
route on a local layer.  The two routes take the query differently (E4M3 x a row scale on the decode kernel, fp16 on the chunk walk), so
the toy queries are +-2^-k, k = 0..3, with a 1 in every row: exact in both.  What is left are the routes' own roundings of weights and
sums; the example asks |difference| <= 2 x (2e-3 max|v| + 1e-6), twice the bound either route is tested against with sum p|v| <= max|v|.

    python examples/fp8_spec_window_example.py [--rounds 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOW = 40


def run(prompts=(37, 64, 130), rounds=3, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        layers, H, D, T, S, R = 2, 8, 128, 256, 4, 4
        conn = SpeckvKVConnector(lib, layers, H, D, T, "fp8")
        gen = torch.Generator(device="cuda"); gen.manual_seed(53)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm, keep = list(range(1, len(prompts) + 1)), D ** -0.5, []
        B = len(rids)
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, rnd(layers, n, H, D), rnd(layers, n, H, D))
        chain = list(range(-1, S - 1))
        for rnd_i in range(rounds):
            sign = torch.randint(0, 2, (B, S, H, R, D), generator=gen, device="cuda") * 2.0 - 1.0
            q = (sign * torch.exp2(-torch.randint(0, 4, (B, S, H, R, D), generator=gen, device="cuda").float())).to(torch.float16)
            q[..., 0] = 1.0
            k_new, v_new = rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            for layer, window in ((0, WINDOW), (1, None)):
                spec = conn.attend_spec(layer, rids, q, k_new, v_new, sm, window=window)
                tree = conn.attend_tree(layer, rids, q, k_new, v_new, sm, chain, window=window)
                torch.cuda.synchronize()
                worst = float((spec - tree).abs().max()) / (2.0 * (2e-3 * 6.0 + 1e-6))      # (|v| of randn rows stays below 6)
                if verbose:
                    print(f"round {rnd_i} layer {layer} ({'window %d' % window if window else 'global'}): lengths {[conn.length(r) for r in rids]}, "
                          f"attend_spec against attend_tree {worst:.3f} of the bound")
                assert torch.isfinite(spec).all() and worst <= 1.0, (rnd_i, layer, worst)
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
