#!/usr/bin/env python3
"""The split pool's decode step on a model that interleaves LOCAL and GLOBAL layers: `SpeckvSplitKVConnector.attend(window=W)`.

A toy loop on an MI355X.  Random K / V rows stand in for a model with one local (sliding-window) layer and one global layer, as Mistral,
Gemma 2 / 3 and gpt-oss interleave them.  Three requests of different lengths go in through `write_prefill`; then a few decode steps:
layer 0 is local -- ONE `attend(window=W)` (`speckv_ext_attend_kv_batch_window`: every request is walked from its window's tile in the
FP8 K allocation and in the MXFP4 V allocation, ceil((W + 31) / 32) tiles at most whatever its context) -- layer 1 is global, ONE
`attend` over everything (`speckv_ext_attend_kv_batch`); one `speckv_ext_attend_fold_tail` per layer while some request has an odd
length; then `commit` of the step's new position.

Checked in the example itself: every call's output against a torch float64 softmax attention over the dequantised window -- the query
as the kernel takes it (E4M3 x a row scale: kv_accuracy.quantize_query_e4m3; the fp16 query against the fp16 tail), the stored K rows
[lo, stored) as the FP8 records give them back and the stored V rows as the MXFP4 records give them back (`speckv_ext_fetch_range`),
lo = max(0, length - W) on the local layer and 0 on the global one -- within the project's bound for the kernels with an 8-bit query,
(2e-3 + 2 delta) sum p|v| + 1e-6 with delta = 3e-5 max sum |q||k| sm.

    python examples/k8v4_window_decode_example.py [--steps 6] [--window 40]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompts=(37, 70, 131), steps=6, window=40, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        layers, H, D, T, G = 2, 8, 128, 256, 4
        local = (True, False)                                              # layer 0 local, layer 1 global
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(31)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm = list(range(1, len(prompts) + 1)), 1.0 / np.sqrt(D)
        tails, keep = {}, []
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            keep += conn.write_prefill(rid, k, v)
            tails[rid] = (k[:, -1].double(), v[:, -1].double())             # the last position's fp16 rows [layers][heads][dim]: the tail while the length is odd

        def stored(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim] on the device"""
            out = torch.zeros((n // 2, 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.double().reshape(n, H, D)

        def check(layer, q, out):
            worst = 0.0
            for b, rid in enumerate(rids):
                r, n = conn.requests[rid], conn.length(rid)
                even = n & ~1
                lo = max(0, n - window) if local[layer] else 0
                kk, vv = stored(r.k_handle, layer, even)[lo:], stored(r.v_handle, layer, even)[lo:]
                qe = torch.from_numpy(quantize_query_e4m3(q[b].cpu().numpy())).cuda()
                s = torch.einsum("hgd,thd->hgt", qe, kk) * sm
                reach = torch.einsum("hgd,thd->hgt", qe.abs(), kk.abs()).amax(dim=(1, 2)) * sm if kk.shape[0] else torch.zeros(H, dtype=torch.float64, device="cuda")
                if n & 1:                                                  # the tail: fp16 rows, scored with the fp16 query; always inside the window
                    tk, tv = tails[rid][0][layer], tails[rid][1][layer]
                    s = torch.cat([s, (torch.einsum("hgd,hd->hg", q[b].double(), tk) * sm)[..., None]], dim=-1)
                    vv = torch.cat([vv, tv[None]])
                p = torch.softmax(s, dim=-1)
                want, mag = torch.einsum("hgt,thd->hgd", p, vv), torch.einsum("hgt,thd->hgd", p, vv.abs())
                tol = (2e-3 + 2 * 3e-5 * reach)[:, None, None] * mag + 1e-6
                worst = max(worst, float(((out[b].double() - want).abs() / tol).max()))
            assert worst <= 1.0, (layer, worst)
            return worst

        for step in range(steps):
            worst = 0.0
            for layer in range(layers):
                q = rnd(len(rids), H, G, D)
                worst = max(worst, check(layer, q, conn.attend(layer, rids, q, sm, window=window if local[layer] else None)))
            k_new, v_new = rnd(len(rids), 1, layers, H, D), rnd(len(rids), 1, layers, H, D)
            keep += conn.commit(rids, k_new, v_new, [1] * len(rids))
            for b, rid in enumerate(rids):
                tails[rid] = (k_new[b, 0].double(), v_new[b, 0].double())
            if verbose:
                print(f"decode step {step}: lengths {[conn.length(r) for r in rids]}, window {window} on layer 0, worst err / tol {worst:.3f}")
        torch.cuda.synchronize()
        assert [conn.length(r) for r in rids] == [n + steps for n in prompts]
        if verbose:
            print(f"ok: {steps} decode steps over {len(rids)} requests, one attention launch per layer and step, the local layer walks its window only")
        return steps
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--window", type=int, default=40)
    a = ap.parse_args()
    run(steps=a.steps, window=a.window)
