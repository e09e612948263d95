#!/usr/bin/env python3
"""Draft and verify on the split pool: `SpeckvSplitKVConnector.attend_spec` -- the draft positions of every request verified on the decode
kernel, one launch per layer and group.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.  Three requests of different lengths go in through
`write_prefill`; then rounds of two steps each:
  a CHAIN of S = 4 drafts per request -- per layer ONE `attend_spec` (`speckv_ext_attend_kv_spec`: the stored positions are walked once for
        the 16 query rows of a kv head, the request's odd last position and the four new rows are folded in inside that launch), a
        pretended accept count per request, `commit(n_accept)`;
  a small TREE (root, two branches of two) -- `attend_spec(parents=...)`; the caller picks the accepted path, gathers its rows in path
        order and stores them with `commit(n_accept)`.
No state moves in `attend_spec`; `commit` stores what was accepted.

Checked in the example itself: every layer of every step against `attend_chunk` with the same step (the split pool's other route for
several positions, a different kernel: fp16 query, fp16 tiles).  The two routes differ by definition in the query of the stored part (E4M3
x a row scale here, kv_accuracy.quantize_query_e4m3); that known difference is taken from two float64 references over the rows as the
records decode (`speckv_ext_fetch_range`), and what remains between the two outputs is held to the sum of the two routes' bounds:
(2e-3 + 2 delta) sum p|v| + 1e-6 with delta = 3e-5 max sum |q||k| sm for this one, 2e-3 sum p|v| + 1e-6 for the chunk walk.

    python examples/k8v4_spec_example.py [--rounds 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TREE = [-1, 0, 1, 0, 3]                  # node 0, the branch 1 - 2 and the branch 3 - 4
PATHS = [[0, 1, 2], [0, 3, 4], [0, 3]]   # the accepted path per request (pretended)


def run(prompts=(37, 64, 130), rounds=3, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, R = 8, 128, 256, 4
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(31)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm = list(range(1, len(prompts) + 1)), 1.0 / np.sqrt(D)
        B = len(rids)
        rows, keep = {}, []
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            keep += conn.write_prefill(rid, k, v)
            rows[rid] = [k.cpu().numpy(), v.cpu().numpy()]                 # [layers][positions][heads][dim]: every row the request holds

        def stored_rows(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim]"""
            out = torch.empty((n // 2, 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.cpu().numpy().astype(np.float64).reshape(n, H, D)

        def references(layer, q, k_new, v_new, words):
            """float64 over the stored rows as the records decode and the fp16 rows held outside the pool: what attend_spec computes (the
            stored part with the E4M3 query), what attend_chunk computes (the fp16 query throughout), and the sum of the two bounds"""
            S = q.shape[1]
            want = np.zeros((2, B, S, H, R, D))
            tol = np.zeros((B, S, H, R, D))
            for b, rid in enumerate(rids):
                r, n = conn.requests[rid], conn.length(rid)
                even = n & ~1
                held_k = np.concatenate([rows[rid][0][layer, even:n], k_new[b, :, layer].cpu().numpy()]).astype(np.float64)
                held_v = np.concatenate([rows[rid][1][layer, even:n], v_new[b, :, layer].cpu().numpy()]).astype(np.float64)
                kk = np.concatenate([stored_rows(r.k_handle, layer, even), held_k])                             # [even + base + S][heads][dim]
                vv = np.concatenate([stored_rows(r.v_handle, layer, even), held_v])
                q16 = q[b].cpu().numpy()                                                                        # [S][heads][R][dim]
                s16 = np.einsum("jhrd,thd->jhrt", q16.astype(np.float64), kk) * sm
                s8 = s16.copy()
                s8[..., :even] = np.einsum("jhrd,thd->jhrt", quantize_query_e4m3(q16), kk[:even]) * sm
                reach = (np.einsum("jhrd,thd->jhrt", np.abs(q16.astype(np.float64)), np.abs(kk)) * sm).max()
                for j in range(S):
                    cols = list(range(even)) + [even + t for t in range(len(held_k)) if (words[b][j] >> t) & 1]
                    if len(cols) == even:
                        continue                                           # a dead node: not compared
                    for route, s in enumerate((s8, s16)):
                        p = np.exp(s[j][..., cols] - s[j][..., cols].max(-1, keepdims=True))
                        p /= p.sum(-1, keepdims=True)
                        want[route, b, j] = np.einsum("hrt,thd->hrd", p, vv[cols])
                        mag = np.einsum("hrt,thd->hrd", p, np.abs(vv[cols]))
                        tol[b, j] += ((2e-3 + 2 * 3e-5 * reach) if route == 0 else 2e-3) * mag + 1e-6
            return want, tol

        def verify(q, k_new, v_new, parents, n_new=None):
            """attend_spec against attend_chunk, layer by layer: what the two routes differ by beyond the E4M3 query of the stored part (known
            from the float64 references) within the sum of their bounds -> worst difference / bound, and how far the query moved the rows"""
            worst, moved = 0.0, 0.0
            base = [conn.length(r) & 1 for r in rids]
            words = SpeckvKVConnector.tree_masks(parents if parents is not None else list(range(-1, q.shape[2] - 1)), base, n_new)
            for layer in range(layers):
                spec = conn.attend_spec(layer, rids, q[layer], k_new, v_new, sm, n_new=n_new, parents=parents)
                chunk = conn.attend_chunk(layer, rids, q[layer], k_new, v_new, sm, n_new=n_new, parents=parents)
                torch.cuda.synchronize()
                want, tol = references(layer, q[layer], k_new, v_new, words)
                live = tol > 0
                apart = (spec.cpu().numpy().astype(np.float64) - chunk.cpu().numpy()) - (want[0] - want[1])
                worst = max(worst, float((np.abs(apart)[live] / tol[live]).max()))
                moved = max(moved, float(np.abs(want[0] - want[1]).max()))
            assert worst <= 1.0, worst
            return worst, moved

        def stored(b, rid, k_new, v_new, picked):
            for kind, new in enumerate((k_new, v_new)):
                rows[rid][kind] = np.concatenate([rows[rid][kind], new[b, picked].permute(1, 0, 2, 3).cpu().numpy()], axis=1)

        for rnd_no in range(rounds):
            # ---- a chain of four drafts; the "model" accepts a different count per request
            S = 4
            q, k_new, v_new = rnd(layers, B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            worst_chain, moved = verify(q, k_new, v_new, None)
            accept = [(rnd_no + b) % (S + 1) for b in range(B)]
            for b, rid in enumerate(rids):
                stored(b, rid, k_new, v_new, list(range(accept[b])))
            keep += conn.commit(rids, k_new, v_new, accept)
            # ---- a tree of five drafts; the accepted PATH's rows are gathered in path order and committed as a prefix
            S = len(TREE)
            q, k_new, v_new = rnd(layers, B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            worst_tree, _ = verify(q, k_new, v_new, TREE)
            paths = [PATHS[(rnd_no + b) % len(PATHS)] for b in range(B)]
            k_path, v_path = torch.zeros_like(k_new), torch.zeros_like(v_new)
            for b, rid in enumerate(rids):
                k_path[b, :len(paths[b])], v_path[b, :len(paths[b])] = k_new[b, paths[b]], v_new[b, paths[b]]
                stored(b, rid, k_new, v_new, paths[b])
            keep += conn.commit(rids, k_path, v_path, [len(p) for p in paths])
            assert [conn.length(r) for r in rids] == [rows[r][0].shape[1] for r in rids]
            if verbose:
                print(f"round {rnd_no}: lengths {[conn.length(r) for r in rids]}, attend_spec vs attend_chunk worst difference / bound: "
                      f"chain {worst_chain:.3f}, tree {worst_tree:.3f} (the E4M3 query of the stored part moves a row by up to {moved:.4f})")
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: {rounds} rounds of a chain and a tree step over {B} requests, one attention launch per layer and step")
        return rounds
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    run(rounds=a.rounds)
