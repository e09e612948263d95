#!/usr/bin/env python3
"""A draft TREE verified on sliding-window layers: tree speculation for a stack whose layers alternate local and global attention.

A toy loop on an MI355X.  Random K / V rows stand in for a model whose even layers are LOCAL (a position sees itself and the
`--window` - 1 positions in front of it) and whose odd layers are GLOBAL, as the Mistral family, Gemma 2 / 3 and gpt-oss interleave
them.  Every step brings a small tree of draft nodes.  A node's position is its DEPTH in the tree, not its index: node j of depth d sits
at the absolute position length + d and, on a local layer, sees the last W positions of ITS OWN root path -- stored positions, the odd
last position, its ancestors, itself.  ONE call per layer does the attention for the whole tree: `SpeckvKVConnector.attend_tree(...,
window=W)` on a local layer (`speckv_ext_attend_chunk_tree_window`), the same call without a window on a global one.  Then a
root-to-node path is "accepted" and stored by `commit(nodes=path)`, and the next tree follows over the longer request.

Every output is held to a float32 softmax attention in torch, on the device, over the rows the pool holds (`kv_rows`), the odd last
position and the nodes as they are, masked by a walk up the parents.

    python examples/sliding_window_tree_example.py [--scheme fp8] [--window 24] [--prompt 300] [--steps 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# 14 nodes: two roots, branches of unequal depth, and a deep node (5, depth 4) in front of a root (6)
TREE = [-1, 0, 1, 2, 0, 3, -1, 6, 6, 7, 9, 4, 10, 12]


def run(scheme="fp8", window=24, prompt=300, steps=4, layers=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G, S = 8, 128, 512, 4, len(TREE)
        assert prompt + steps * S <= T
        windows = [window if layer % 2 == 0 else None for layer in range(layers)]        # local, global, local, ...
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(29)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        req = 1
        conn.add_request(req)
        keep = conn.write_prefill(req, rnd(layers, prompt, H, D), rnd(layers, prompt, H, D))
        depth = SpeckvKVConnector.chunk_tree_depths(TREE)[0]
        paths = []
        for j in range(S):                                                     # root paths, by a walk up the parents
            path, a = [], j
            while a >= 0:
                path.append(a)
                a = TREE[a]
            paths.append(path[::-1])
        sm = 1.0 / np.sqrt(D)
        worst = {"local": 0.0, "global": 0.0}
        for step in range(steps):
            length = conn.length(req)
            k_new, v_new = rnd(1, S, layers, H, D), rnd(1, S, layers, H, D)
            for layer, w in enumerate(windows):
                q = rnd(1, S, H, G, D)
                out = conn.attend_tree(layer, [req], q, k_new, v_new, sm, TREE, splits=0, window=w)
                # what the request holds as the pool gives it back (the odd last position as it was given), then the nodes as they are
                kk = torch.cat((conn.kv_rows(req, layer, 0), k_new[0, :, layer])).to(torch.float32)
                vv = torch.cat((conn.kv_rows(req, layer, 1), v_new[0, :, layer])).to(torch.float32)
                sees = torch.zeros(S, length + S, dtype=torch.bool, device="cuda")
                for j in range(S):
                    lo = 0 if w is None else max(0, length + depth[j] + 1 - w)
                    sees[j, lo:length] = True
                    for a in paths[j]:
                        sees[j, length + a] = length + depth[a] >= lo
                s = torch.einsum("nhgd,thd->nhgt", q[0].to(torch.float32), kk) * sm
                want = torch.einsum("nhgt,thd->nhgd", torch.softmax(s.masked_fill(~sees[:, None, None, :], float("-inf")), dim=-1), vv)
                err = float((out[0] - want).abs().max())
                assert bool(torch.isfinite(out).all()) and err < 2e-2, (step, layer, w, err)
                kind = "global" if w is None else "local"
                worst[kind] = max(worst[kind], err)
            accepted = paths[(5, 13, 8, 11)[step % 4]]                       # the verifier's choice: some root-to-node path
            keep += conn.commit([req], k_new, v_new, [accepted])
            assert conn.length(req) == length + len(accepted)
            if verbose:
                print(f"tree step {step}: {S} nodes over {length} positions, path {accepted} accepted -> length {conn.length(req)}; "
                      f"worst |err| local (W = {window}) {worst['local']:.2e}, global {worst['global']:.2e}")
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: {layers} layers (local W = {window} / global alternating), {steps} tree steps of {S} nodes agree with the torch reference")
        del keep
        return conn.length(req)
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--window", type=int, default=24)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    run(a.scheme, a.window, a.prompt, a.steps)
