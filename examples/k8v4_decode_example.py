#!/usr/bin/env python3
"""The split pool's decode step: `SpeckvSplitKVConnector.attend` -- one batch launch over FP8 keys and MXFP4 values per layer.

A toy loop on an MI355X.  Random K / V rows stand in for a model.  Three requests of different lengths go in through `write_prefill`; then
a few decode steps: per layer ONE `attend` over everything the requests hold (`speckv_ext_attend_kv_batch`, and one
`speckv_ext_attend_fold_tail` while some request has an odd length), then `commit` of the step's new position.  No fp16 K or V tile is
materialised on this route: K feeds the FP8 matrix instruction as it lies in the record, V is widened from its MXFP4 record in registers.

Checked in the example itself: every call's output against a float64 softmax attention over the rows the requests hold -- the query as
the kernel takes it (E4M3 x a row scale: kv_accuracy.quantize_query_e4m3; the fp16 query against the fp16 tail), the stored K rows as the
FP8 records give them back and the stored V rows as the MXFP4 records give them back (`speckv_ext_fetch_range`) -- within the project's
bound for the kernels with an 8-bit query, (2e-3 + 2 delta) sum p|v| + 1e-6 with delta = 3e-5 max sum |q||k| sm.

    python examples/k8v4_decode_example.py [--steps 6]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompts=(37, 64, 130), steps=6, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 256, 4
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(29)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rids, sm = list(range(1, len(prompts) + 1)), 1.0 / np.sqrt(D)
        rows, keep = {}, []
        for rid, n in zip(rids, prompts):
            conn.add_request(rid)
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            keep += conn.write_prefill(rid, k, v)
            rows[rid] = [k.cpu().numpy(), v.cpu().numpy()]                 # [layers][positions][heads][dim]: every row the request holds

        def stored(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim]"""
            out = torch.empty((n // 2, 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.cpu().numpy().astype(np.float64).reshape(n, H, D)

        def check(layer, q, out):
            worst = 0.0
            for b, rid in enumerate(rids):
                r, n = conn.requests[rid], conn.length(rid)
                even = n & ~1
                kk, vv = stored(r.k_handle, layer, even), stored(r.v_handle, layer, even)
                q16 = q[b].cpu().numpy()
                s = np.einsum("hgd,thd->hgt", quantize_query_e4m3(q16), kk) * sm
                reach = np.einsum("hgd,thd->hgt", np.abs(quantize_query_e4m3(q16)), np.abs(kk)).max(axis=(1, 2), initial=0.0) * sm      # per head
                if n & 1:                                                  # the tail: fp16 rows, scored with the fp16 query
                    tk, tv = rows[rid][0][layer, n - 1].astype(np.float64), rows[rid][1][layer, n - 1].astype(np.float64)
                    s = np.concatenate([s, (np.einsum("hgd,hd->hg", q16.astype(np.float64), tk) * sm)[..., None]], axis=-1)
                    vv = np.concatenate([vv, tv[None]])
                p = np.exp(s - s.max(-1, keepdims=True))
                p /= p.sum(-1, keepdims=True)
                want, mag = np.einsum("hgt,thd->hgd", p, vv), np.einsum("hgt,thd->hgd", p, np.abs(vv))
                tol = (2e-3 + 2 * 3e-5 * reach)[:, None, None] * mag + 1e-6
                worst = max(worst, float((np.abs(out[b].cpu().numpy() - want) / tol).max()))
            assert worst <= 1.0, (layer, worst)
            return worst

        for step in range(steps):
            worst = 0.0
            for layer in range(layers):
                q = rnd(len(rids), H, G, D)
                worst = max(worst, check(layer, q, conn.attend(layer, rids, q, sm)))
            k_new, v_new = rnd(len(rids), 1, layers, H, D), rnd(len(rids), 1, layers, H, D)
            keep += conn.commit(rids, k_new, v_new, [1] * len(rids))
            for b, rid in enumerate(rids):
                rows[rid][0] = np.concatenate([rows[rid][0], k_new[b].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
                rows[rid][1] = np.concatenate([rows[rid][1], v_new[b].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
            if verbose:
                print(f"decode step {step}: lengths {[conn.length(r) for r in rids]}, worst err / tol {worst:.3f}")
        torch.cuda.synchronize()
        assert [conn.length(r) for r in rids] == [n + steps for n in prompts]
        if verbose:
            print(f"ok: {steps} decode steps over {len(rids)} requests, one attention launch per layer and step")
        return steps
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    run(steps=a.steps)
