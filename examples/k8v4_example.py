#!/usr/bin/env python3
"""The split pool ("K8V4"): FP8 keys and MXFP4 values in two allocations per request, one chunk-attention launch over both.

A toy loop on an MI355X.  Random K / V rows stand in for a model.  A prompt goes in through `write_prefill`, a chunk of further
positions through `attend_chunk` + `commit`, then a few decode steps -- `attend_chunk` with ONE new position -- each followed by
`commit`.  Every attention call is ONE `speckv_ext_attend_chunk_kv` launch per layer, every commit one `speckv_ext_write_pairs` call per
allocation.

Checked in the example itself: every call's output against a float64 softmax attention over the rows the request holds -- the stored K
rows as the FP8 records give them back and the stored V rows as the MXFP4 records give them back (`speckv_ext_fetch_range`), the odd
last position and the new rows as fp16 -- within 2e-3 of sum p|v|; and the pool's footprint: 2048 + 1088 bytes per position pair.

    python examples/k8v4_example.py [--prompt 101] [--chunk 33] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompt=101, chunk=33, steps=5, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 256, 4
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rid, sm = 1, 1.0 / np.sqrt(D)
        hk, hv = conn.add_request(rid)
        k, v = rnd(layers, prompt, H, D), rnd(layers, prompt, H, D)
        keep = conn.write_prefill(rid, k, v)
        rows_k, rows_v = k.cpu().numpy(), v.cpu().numpy()                    # [layers][positions][heads][dim]: every row the request holds

        def stored(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim]"""
            out = torch.empty((n // 2, 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.cpu().numpy().astype(np.float64).reshape(n, H, D)

        def check(layer, q, k_new, v_new, out, what):
            n, even = k_new.shape[1], conn.length(rid) & ~1
            held_k = np.concatenate([rows_k[layer, even:], k_new[0, :, layer].cpu().numpy()]).astype(np.float64)     # the tail, the new rows
            held_v = np.concatenate([rows_v[layer, even:], v_new[0, :, layer].cpu().numpy()]).astype(np.float64)
            kk, vv = np.concatenate([stored(hk, layer, even), held_k]), np.concatenate([stored(hv, layer, even), held_v])
            s = np.einsum("nhgd,thd->nhgt", q[0].cpu().numpy().astype(np.float64), kk) * sm
            sees = conn.length(rid) + np.arange(n)[:, None, None, None] >= np.arange(len(kk))[None, None, None, :]
            s = np.where(sees, s, -np.inf)
            p = np.exp(s - s.max(-1, keepdims=True))
            p /= p.sum(-1, keepdims=True)
            want, mag = np.einsum("nhgt,thd->nhgd", p, vv), np.einsum("nhgt,thd->nhgd", p, np.abs(vv))
            worst = float((np.abs(out[0].cpu().numpy() - want) / (2e-3 * mag + 1e-6)).max())
            assert worst <= 1.0, (what, layer, worst)
            return worst

        def step(n, what):
            nonlocal rows_k, rows_v, keep
            k_new, v_new = rnd(1, n, layers, H, D), rnd(1, n, layers, H, D)
            worst = 0.0
            for layer in range(layers):
                q = rnd(1, n, H, G, D)
                worst = max(worst, check(layer, q, k_new, v_new, conn.attend_chunk(layer, [rid], q, k_new, v_new, sm), what))
            keep += conn.commit([rid], k_new, v_new, [n])
            rows_k = np.concatenate([rows_k, k_new[0].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
            rows_v = np.concatenate([rows_v, v_new[0].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
            if verbose:
                print(f"{what}: length {conn.length(rid)}, worst err / tol {worst:.3f}")

        step(chunk, f"chunk of {chunk}")
        for i in range(steps):
            step(1, f"decode step {i}")
        torch.cuda.synchronize()
        total = prompt + chunk + steps
        assert conn.length(rid) == total
        # the footprint: a written page of the K allocation is a 2048-byte record, of the V allocation a 1088-byte record
        pages = (total & ~1) // 2
        for layer in range(layers):
            for page in (0, pages - 1):
                at = (layer * (T // 2) + page) * 4096
                assert lib.translate(hk, at).rec_bytes == 2048 and lib.translate(hv, at).rec_bytes == 1088
        if verbose:
            print(f"ok: {total} positions, {2048 + 1088} bytes per position pair, layer and kind pair ({2 * 4096 / (2048 + 1088):.2f} : 1 against fp16)")
        return total
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=101)
    ap.add_argument("--chunk", type=int, default=33)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    run(a.prompt, a.chunk, a.steps)
