#!/usr/bin/env python3
"""Speculative decoding with a TREE of drafts over the compressed KV pool: verify every branch in ONE pass over the records.

A toy loop on an MI355X.  Per step a "draft" proposes a small token tree per request -- a trunk of 2 with two branches of 2
(random K / V rows and queries stand in for a model):

        context - 0 - 1 - 2 - 3
                       \\
                        4 - 5

`SpeckvKVConnector.attend_spec(parents=...)` computes the attention of all 6 nodes from one pass over the compressed records; a
node sees the request's stored context, its ancestors and itself, not the other branch.  The "verifier" then accepts a path
per request -- here a random root-to-node chain stands in for the longest path whose tokens match -- and `append_path` commits
exactly that path.

Every step is checked against what the library offered before: one chain `attend_spec` call per root-to-leaf path (two calls,
two passes over the records), which must give the same rows for the nodes of that path; and a second connector that receives
the accepted nodes one `append` at a time must end up holding the same bits: lengths, rows, and the next attention.

    python examples/spec_tree_example.py [--steps 6] [--scheme fp8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARENTS = [-1, 0, 1, 2, 1, 4]                      # a trunk of 2 (nodes 0, 1) with two branches of 2 (2, 3 and 4, 5)
LEAF_PATHS = [[0, 1, 2, 3], [0, 1, 4, 5]]
PATHS = [[], [0], [0, 1], [0, 1, 2], [0, 1, 2, 3], [0, 1, 4], [0, 1, 4, 5]]       # every chain from the context down to a node


def run(steps=6, scheme="fp8", layers=2, rows_per_pos=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, S = 8, 128, 512, len(PARENTS)
        spec = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        eager = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(5)
        prompts = [64, 97, 150]
        ids, ids_e = [1, 2, 3], [101, 102, 103]
        keep = []
        for rid, rid_e, n in zip(ids, ids_e, prompts):
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            spec.add_request(rid); eager.add_request(rid_e)
            keep += spec.write_prefill(rid, k, v) + eager.write_prefill(rid_e, k, v)
        B, sm = len(ids), 1.0 / np.sqrt(D)
        accepted_total, worst = 0, 0.0
        for step in range(steps):
            k_new, v_new = rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)       # the draft tree's S nodes per request
            q = rnd(layers, B, S, H, rows_per_pos, D)
            out = [spec.attend_spec(layer, ids, q[layer], k_new, v_new, sm, parents=PARENTS) for layer in range(layers)]     # [B][S][H][rows][D] each
            # the same tree as one chain step per root-to-leaf path: the nodes of the path get the same rows
            for path in LEAF_PATHS:
                at = torch.tensor(path, device="cuda")
                for layer in range(layers):
                    chain = spec.attend_spec(layer, ids, q[layer][:, at].contiguous(), k_new[:, at].contiguous(), v_new[:, at].contiguous(), sm)
                    rel = float((out[layer][:, at] - chain).norm() / chain.norm())
                    worst = max(worst, rel)
                    assert rel <= 1e-5, (step, path, layer, rel)       # the same records, the same fp16 rows, folded in the same order
            # the verifier's verdict: a path per request
            paths = [PATHS[int(x)] for x in rng.integers(0, len(PATHS), B)]
            paths[step % B] = LEAF_PATHS[step % 2]
            keep += spec.append_path(ids, k_new, v_new, paths, PARENTS)
            for t in range(max(len(p) for p in paths)):                           # the single-token path: the accepted nodes one at a time
                members = [b for b in range(B) if len(paths[b]) > t]
                idx = torch.tensor(members, device="cuda")
                node = torch.tensor([paths[b][t] for b in members], device="cuda")
                keep += eager.append([ids_e[b] for b in members], k_new[idx, node], v_new[idx, node])
            accepted_total += sum(len(p) for p in paths)
            # after the commit: the same state, bit for bit
            qn = rnd(B, H, rows_per_pos, D)
            for rid, rid_e in zip(ids, ids_e):
                assert spec.length(rid) == eager.length(rid_e)
            for layer in range(layers):
                assert torch.equal(spec.attend(layer, ids, qn, sm), eager.attend(layer, ids_e, qn, sm)), (step, layer)
            torch.cuda.synchronize()
            keep = keep[-8:]
        result = {"steps": steps, "nodes": S, "accepted": accepted_total, "lengths": [spec.length(r) for r in ids],
                  "worst_relative_difference_to_chain_calls": float(f"{worst:.3g}")}
        if verbose:
            print(result)
            print("spec tree example ok")
        for rid, rid_e in zip(ids, ids_e):
            spec.free_request(rid); eager.free_request(rid_e)
        return result
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    a = ap.parse_args()
    run(a.steps, a.scheme)
