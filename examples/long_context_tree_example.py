#!/usr/bin/env python3
"""A 40-node draft tree over ONE request with a long context: the stored positions split across the chip.

A toy step on an MI355X.  Random K / V rows stand in for a model.  One request holds a few thousand positions in the compressed pool and
drafts a tree of 40 nodes -- more than `attend_spec(parents=...)` takes.  `SpeckvKVConnector.attend_chunk(parents=...)` alone verifies it
with 5 query blocks x 8 kv heads = 40 workgroups, each walking the whole context: most of a 256-CU chip idles.  With `splits=0` the
library's rule (`SpeckvKVConnector.chunk_pieces`, `speckv_ext_chunk_split_plan`) cuts the stored positions into pieces that run side by
side and a second launch merges them (`speckv_ext_attend_chunk_split`).

The split result is held to the unsplit one (`splits=1`) within the project's bound of this kernel against float64, applied to both:
|a - b| <= 2 (2e-3 sum p|v| + 1e-6), with sum p|v| from a float64 softmax over the rows the request holds and the node's ancestors.  A
root-to-leaf path is then stored by `commit(nodes=path)`.

    python examples/long_context_tree_example.py [--scheme fp8] [--context 4001]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NODES = 40


def draft_tree(rng, n=NODES):
    """4 children of the context, every later node under a random earlier one (a parent precedes its children)"""
    return [-1] * 4 + [int(rng.integers(0, j)) for j in range(4, n)]


def path_to(parents, leaf):
    path = []
    while leaf >= 0:
        path.append(leaf)
        leaf = parents[leaf]
    return path[::-1]


def run(scheme="fp8", context=4001, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, G = 8, 128, 8
        T = (context + NODES + 63) & ~63
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(29)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(29)
        conn.add_request(1)
        keep = conn.write_prefill(1, rnd(layers, context, H, D), rnd(layers, context, H, D))
        sm = 1.0 / np.sqrt(D)
        parents = draft_tree(rng)
        pieces, tiles, _ = conn.chunk_pieces([NODES], [context], G, 0, torch.cuda.get_device_properties(0).multi_processor_count)
        assert pieces[0] > 1, "a context this short is not split: pass --context 4001 or more"
        k_new, v_new = rnd(1, NODES, layers, H, D), rnd(1, NODES, layers, H, D)
        worst = 0.0
        for layer in range(layers):
            q = rnd(1, NODES, H, G, D)
            split = conn.attend_chunk(layer, [1], q, k_new, v_new, sm, parents=parents, splits=0)
            whole = conn.attend_chunk(layer, [1], q, k_new, v_new, sm, parents=parents, splits=1)
            held = conn.length(1)
            kk = torch.cat((conn.kv_rows(1, layer, 0), k_new[0, :, layer])).to(torch.float64)       # [held + nodes][H][D]
            vv = torch.cat((conn.kv_rows(1, layer, 1), v_new[0, :, layer])).to(torch.float64)
            sees = torch.zeros((NODES, held + NODES), dtype=torch.bool, device="cuda")
            sees[:, :held] = True
            for j in range(NODES):
                sees[j, [held + a for a in path_to(parents, j)]] = True
            s = torch.einsum("nhgd,thd->nhgt", q[0].to(torch.float64), kk) * sm
            p = torch.softmax(s.masked_fill(~sees[:, None, None, :], float("-inf")), dim=-1)
            tol = 2e-3 * torch.einsum("nhgt,thd->nhgd", p, vv.abs()) + 1e-6
            ratio = float(((split[0] - whole[0]).abs().to(torch.float64) / (2 * tol)).max())
            assert ratio <= 1.0, (layer, ratio)
            worst = max(worst, ratio)
        path = path_to(parents, NODES - 1)
        keep += conn.commit([1], k_new, v_new, nodes=[path])
        torch.cuda.synchronize()
        assert conn.length(1) == context + len(path)
        if verbose:
            print(f"ok: {NODES}-node tree over {context} positions in {pieces[0]} pieces of {tiles[0]} tiles; split against whole: "
                  f"{worst:.3f} of the bound; a path of {len(path)} nodes committed, length {conn.length(1)}")
        return conn.length(1)
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--context", type=int, default=4001)
    a = ap.parse_args()
    run(a.scheme, a.context)
