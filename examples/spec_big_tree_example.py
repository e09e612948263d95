#!/usr/bin/env python3
"""Speculative decoding with a LARGE draft tree over the compressed KV pool: 40 nodes verified in one launch per layer.

A toy loop on an MI355X.  Random K / V rows stand in for a model.  Per step every request drafts a tree of 40 nodes -- more than
`attend_spec(parents=...)` takes (16) -- and `SpeckvKVConnector.attend_chunk(parents=...)` verifies it: ONE
`speckv_ext_attend_chunk_masked` launch per layer, a node sees what the request holds, its ancestors and itself.  A root-to-leaf path is
then "accepted" and stored by `commit(nodes=path)` (one `speckv_ext_write_pairs` launch; without `parents` it has no bound on the tree's
size), and the next step drafts on top of it.

Every node's attention output is held to a float32 softmax attention over the rows the request holds and the node's ancestors.

    python examples/spec_big_tree_example.py [--scheme fp8] [--steps 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NODES = 40


def draft_tree(rng, n=NODES):
    """a tree of n nodes in an order where a parent precedes its children: 4 children of the context, every later node under a random
    earlier one"""
    return [-1] * 4 + [int(rng.integers(0, j)) for j in range(4, n)]


def path_to(parents, leaf):
    path = []
    while leaf >= 0:
        path.append(leaf)
        leaf = parents[leaf]
    return path[::-1]


def run(scheme="fp8", steps=3, batch=3, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 8
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(23)
        ids, keep = list(range(1, batch + 1)), []
        for rid, n in zip(ids, (64, 37, 1)):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, rnd(layers, n, H, D), rnd(layers, n, H, D))
        sm = 1.0 / np.sqrt(D)
        for step in range(steps):
            parents = [draft_tree(rng) for _ in ids]
            k_new, v_new = rnd(batch, NODES, layers, H, D), rnd(batch, NODES, layers, H, D)
            for layer in range(layers):
                q = rnd(batch, NODES, H, G, D)
                out = conn.attend_chunk(layer, ids, q, k_new, v_new, sm, parents=parents)
                for b, rid in enumerate(ids):
                    held = conn.length(rid)
                    kk = torch.cat((conn.kv_rows(rid, layer, 0), k_new[b, :, layer])).to(torch.float32)       # [held + nodes][H][D]
                    vv = torch.cat((conn.kv_rows(rid, layer, 1), v_new[b, :, layer])).to(torch.float32)
                    sees = torch.zeros((NODES, held + NODES), dtype=torch.bool, device="cuda")
                    sees[:, :held] = True
                    for j in range(NODES):
                        sees[j, [held + a for a in path_to(parents[b], j)]] = True
                    s = torch.einsum("nhgd,thd->nhgt", q[b].to(torch.float32), kk) * sm
                    want = torch.einsum("nhgt,thd->nhgd", torch.softmax(s.masked_fill(~sees[:, None, None, :], float("-inf")), dim=-1), vv)
                    err = float((out[b] - want).abs().max())
                    assert err < 2e-2, (step, layer, rid, err)
            accepted = [path_to(p, int(rng.integers(NODES // 2, NODES))) for p in parents]
            before = [conn.length(rid) for rid in ids]
            keep += conn.commit(ids, k_new, v_new, accepted)
            assert [conn.length(rid) for rid in ids] == [n + len(p) for n, p in zip(before, accepted)]
            if verbose:
                print(f"step {step}: trees of {NODES} nodes verified, paths of {[len(p) for p in accepted]} nodes accepted, "
                      f"lengths {[conn.length(rid) for rid in ids]}")
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: {steps} steps of {NODES}-node trees, one attention launch per layer and one commit launch per step")
        return [conn.length(rid) for rid in ids]
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    run(a.scheme, a.steps)
