#!/usr/bin/env python3
"""Draft and verify on an FP8 pool at 8 query heads per kv head: `SpeckvKVConnector.attend_spec(rows_per_pass=32)` -- four draft
positions x 8 query rows are 32 rows per kv head, verified in ONE launch and one pass over the stored records instead of two.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.  Three requests of different lengths go in through
`write_prefill`; then rounds of three steps each:
  a CHAIN of S = 4 drafts at rows_per_pos = 8 on a global layer -- per layer ONE `speckv_ext_attend_spec_wide` (k_attend_fp8_wide: a
        wave carries rows 0..15 and 16..31 of the group over each tile's K bytes, f16 V operand and V reference scale, the held rows
        folded inside the launch); `attend_spec()` without the argument is two planned calls, each followed by its fold launch;
  the same chain on a SLIDING-WINDOW layer, `window=W` (without the argument: two `speckv_ext_attend_spec_window` calls);
  a TREE of 8 nodes at rows_per_pos = 4 (root, a branch of three and a branch of four): the second branch lies in the second row block.
Then a pretended accept count per request and `append_tokens(n_accept)`.  No state moves in `attend_spec`.

Checked in the example itself: every layer of every step against `attend_spec()` with the same step.  Under a window the 16-row kernel
computes every row with the same arithmetic in the same order over the same pieces; on a global layer the 16-row route folds the held
rows in a second launch, in another order.  Both are held to 1e-3 on rows of unit-variance values; the float64 checks are
tests/test_gpu_fp8_spec_wide.py's.

    python examples/fp8_spec_wide_example.py [--rounds 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TREE = [-1, 0, 1, 2, 0, 4, 5, 6]


def run(prompts=(37, 64, 130), rounds=3, layers=2, window=48, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T = 8, 128, 256
        conn = SpeckvKVConnector(lib, layers, H, D, T, "fp8")
        gen = torch.Generator(device="cuda"); gen.manual_seed(47)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm = list(range(1, len(prompts) + 1)), 1.0 / np.sqrt(D)
        B = len(rids)
        keep = []
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, rnd(layers, n, H, D), rnd(layers, n, H, D))

        def verify(S, R, **how):
            """attend_spec(rows_per_pass=32) against attend_spec() layer by layer -> the step's rows and the worst difference"""
            assert [n * R for _, n in SpeckvKVConnector.spec_groups(S, R, 32)] == [32] and len(SpeckvKVConnector.spec_groups(S, R)) == 2
            q, k_new, v_new = rnd(layers, B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            worst = 0.0
            for layer in range(layers):
                wide = conn.attend_spec(layer, rids, q[layer], k_new, v_new, sm, rows_per_pass=32, **how)
                two = conn.attend_spec(layer, rids, q[layer], k_new, v_new, sm, **how)
                torch.cuda.synchronize()
                assert tuple(wide.shape) == (B, S, H, R, D) and bool(torch.isfinite(wide).all())
                worst = max(worst, float((wide - two).abs().max()))
            assert worst <= 1e-3, worst
            return k_new, v_new, worst

        for rnd_no in range(rounds):
            k_new, v_new, worst_chain = verify(4, 8)
            _, _, worst_window = verify(4, 8, window=window)
            _, _, worst_tree = verify(len(TREE), 4, parents=TREE)
            accept = [(rnd_no + b) % 5 for b in range(B)]                  # of the chain's four drafts
            keep += conn.append_tokens(rids, k_new, v_new, accept) or []
            if verbose:
                print(f"round {rnd_no}: lengths {[conn.length(r) for r in rids]}, 32 rows in one launch vs the 16-row route, worst difference: "
                      f"chain {worst_chain:.1e}, window {window} {worst_window:.1e}, tree {worst_tree:.1e}")
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: {rounds} rounds of a chain, a windowed chain and a tree step over {B} requests, one attention launch per layer and step")
        return rounds
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    run(rounds=ap.parse_args().rounds)
