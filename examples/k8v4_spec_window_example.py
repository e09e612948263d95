#!/usr/bin/env python3
"""Draft and verify on the split pool of a model that interleaves LOCAL and GLOBAL attention:
`SpeckvSplitKVConnector.attend_spec(window=W)` -- the draft positions of every request verified on the decode kernel on the
sliding-window layers too, one launch per layer and group.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.  Layer 0 is a local layer (window W = 40), layer 1 a
global one.  Three requests of odd and even lengths go in through `write_prefill`; then rounds of two steps each:
  a CHAIN of S = 4 drafts per request -- `attend_spec(window=W)` on layer 0 (`speckv_ext_attend_kv_spec_window`: the stored positions are
        walked from the tile of the window's bound, each query row masked by its own node's depth inside the kernel), `attend_spec()`
        on layer 1 (`speckv_ext_attend_kv_spec`), a pretended accept count per request, `commit(n_accept)`;
  a small TREE (root, two branches of two) -- the same two calls with `parents=...`: a node's window follows its DEPTH, not its index;
        the accepted path's rows are gathered in path order and stored with `commit(n_accept)`.

Checked in the example itself, with torch in float64: every row of every layer against softmax attention over exactly the positions the
row may see -- the stored ones as the records decode (`speckv_ext_fetch_range`) from max(0, length + depth + 1 - W) on, scored with the
query as the kernel takes it (E4M3 x a row scale, kv_accuracy.quantize_query_e4m3), and the fp16 rows held outside the pool that lie on
the node's root path and inside its window, scored with the fp16 query.  Bound: (2e-3 + 2 delta) sum p|v| + 1e-6, delta = 3e-5 max sum
|q||k| sm.

    python examples/k8v4_spec_window_example.py [--rounds 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TREE = [-1, 0, 1, 0, 3]                  # node 0, the branch 1 - 2 and the branch 3 - 4
PATHS = [[0, 1, 2], [0, 3, 4], [0, 3]]   # the accepted path per request (pretended)
WINDOW = 40


def run(prompts=(37, 64, 130), rounds=3, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        layers, H, D, T, R = 2, 8, 128, 256, 4
        windows = [WINDOW, None]                                           # layer 0 local, layer 1 global
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(47)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm = list(range(1, len(prompts) + 1)), 1.0 / np.sqrt(D)
        B = len(rids)
        tails, keep = {}, []
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            keep += conn.write_prefill(rid, k, v)
            tails[rid] = (k[:, -1].clone(), v[:, -1].clone())              # the last row: held outside the pool while the length is odd

        def stored_rows(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim]"""
            out = torch.empty((n // 2, 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.double().reshape(n, H, D)

        def check(layer, got, q, k_new, v_new, parents):
            """every (request, node, head, row) of one layer against float64 over the visible set -> worst error / bound"""
            W, S, worst = windows[layer], q.shape[1], 0.0
            depths = SpeckvKVConnector.chunk_tree_depths(parents, B)
            words = SpeckvKVConnector.tree_masks(parents, [conn.length(r) & 1 for r in rids], window=W)
            for b, rid in enumerate(rids):
                r, n = conn.requests[rid], conn.length(rid)
                even = n & ~1
                ks, vs = stored_rows(r.k_handle, layer, even), stored_rows(r.v_handle, layer, even)
                held_k = torch.cat(([tails[rid][0][layer][None]] if n & 1 else []) + [k_new[b, :, layer]]).double()
                held_v = torch.cat(([tails[rid][1][layer][None]] if n & 1 else []) + [v_new[b, :, layer]]).double()
                q8 = torch.from_numpy(quantize_query_e4m3(q[b].cpu().numpy())).cuda()               # [S][heads][R][dim] float64
                q16 = q[b].double()
                for j in range(S):
                    lo = min(max(0, n + depths[b][j] + 1 - W), even) if W else 0
                    seen = [t for t in range(len(held_k)) if (words[b][j] >> t) & 1]
                    s = torch.cat((torch.einsum("hrd,thd->hrt", q8[j], ks[lo:]), torch.einsum("hrd,thd->hrt", q16[j], held_k[seen])), dim=2) * sm
                    reach = torch.cat((torch.einsum("hrd,thd->hrt", q8[j].abs(), ks[lo:].abs()), torch.einsum("hrd,thd->hrt", q16[j].abs(), held_k[seen].abs())), dim=2)
                    vals = torch.cat((vs[lo:], held_v[seen]))
                    p = torch.softmax(s, dim=2)
                    want = torch.einsum("hrt,thd->hrd", p, vals)
                    tol = (2e-3 + 2 * 3e-5 * float(reach.max()) * sm) * torch.einsum("hrt,thd->hrd", p, vals.abs()) + 1e-6
                    worst = max(worst, float(((got[b, j].double() - want).abs() / tol).max()))
            assert worst <= 1.0, (layer, worst)
            return worst

        def step(S, parents):
            q, k_new, v_new = rnd(layers, B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            worst = []
            for layer in range(layers):
                got = conn.attend_spec(layer, rids, q[layer], k_new, v_new, sm, parents=parents, window=windows[layer])
                torch.cuda.synchronize()
                worst.append(check(layer, got, q[layer], k_new, v_new, parents if parents is not None else list(range(-1, S - 1))))
            return k_new, v_new, worst

        def commit(k_new, v_new, picked):
            """store the picked rows of every request (in order) and remember the new last row"""
            nonlocal keep
            k_path, v_path = torch.zeros_like(k_new), torch.zeros_like(v_new)
            for b, rid in enumerate(rids):
                if picked[b]:
                    k_path[b, :len(picked[b])], v_path[b, :len(picked[b])] = k_new[b, picked[b]], v_new[b, picked[b]]
                    tails[rid] = (k_new[b, picked[b][-1]].clone(), v_new[b, picked[b][-1]].clone())
            keep += conn.commit(rids, k_path, v_path, [len(p) for p in picked])

        for rnd_no in range(rounds):
            k_new, v_new, chain = step(4, None)
            commit(k_new, v_new, [list(range((rnd_no + b) % 5)) for b in range(B)])
            k_new, v_new, tree = step(len(TREE), TREE)
            commit(k_new, v_new, [PATHS[(rnd_no + b) % len(PATHS)] for b in range(B)])
            if verbose:
                print(f"round {rnd_no}: lengths {[conn.length(r) for r in rids]}, worst error / bound: chain local {chain[0]:.3f} global {chain[1]:.3f}, "
                      f"tree local {tree[0]:.3f} global {tree[1]:.3f}")
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: {rounds} rounds of a chain and a tree step over {B} requests, local layer under W = {WINDOW}, one attention launch per layer and step")
        return rounds
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    run(rounds=a.rounds)
