#!/usr/bin/env python3
"""The split pool's decode step for all layers at once: `SpeckvSplitKVConnector.attend_layers` -- ONE `speckv_ext_attend_kv_layers` call, one
attention launch over layer x request x head quad (and one merge where requests are cut into pieces), the fp16 tails of odd lengths folded
inside it.

A toy loop on an MI355X.  Random K / V rows stand in for a model whose query rows of every layer exist at once (a draft model, a benchmark
harness, layers evaluated in parallel).  Three requests of different lengths go in through `write_prefill`; then a few decode steps: ONE
`attend_layers` for all layers, then `commit` of the step's new position.

Checked in the example itself: every layer's output against a float64 softmax attention over the rows the requests hold, as
examples/k8v4_decode_example.py checks `attend` (the stored part with the E4M3 query over the records' values, the tail with the fp16 query),
within the project's bound for the kernels with an 8-bit query; and against `attend` of that layer within twice that bound (the per-layer
route folds the tail in a launch of its own, after normalising: the same value, not the same bits).

    python examples/k8v4_layers_example.py [--steps 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompts=(37, 64, 130), steps=4, layers=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 256, 4
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(31)
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

        def bound(layer, q, out):
            """(worst err / tol of out [batch][heads][g][dim] against float64, the tolerance itself)"""
            worst, tols = 0.0, []
            for b, rid in enumerate(rids):
                r, n = conn.requests[rid], conn.length(rid)
                even = n & ~1
                kk, vv = stored(r.k_handle, layer, even), stored(r.v_handle, layer, even)
                q16 = q[b].cpu().numpy()
                q8 = quantize_query_e4m3(q16)
                s = np.einsum("hgd,thd->hgt", q8, kk) * sm
                reach = np.einsum("hgd,thd->hgt", np.abs(q8), np.abs(kk)).max(axis=(1, 2), initial=0.0) * sm
                if n & 1:                                                  # the tail: fp16 rows, scored with the fp16 query
                    tk, tv = rows[rid][0][layer, n - 1].astype(np.float64), rows[rid][1][layer, n - 1].astype(np.float64)
                    s = np.concatenate([s, (np.einsum("hgd,hd->hg", q16.astype(np.float64), tk) * sm)[..., None]], axis=-1)
                    vv = np.concatenate([vv, tv[None]])
                p = np.exp(s - s.max(-1, keepdims=True))
                p /= p.sum(-1, keepdims=True)
                want, mag = np.einsum("hgt,thd->hgd", p, vv), np.einsum("hgt,thd->hgd", p, np.abs(vv))
                tol = (2e-3 + 2 * 3e-5 * reach)[:, None, None] * mag + 1e-6
                worst = max(worst, float((np.abs(out[b].cpu().numpy() - want) / tol).max()))
                tols.append(tol)
            return worst, np.stack(tols)

        for step in range(steps):
            q = rnd(layers, len(rids), H, G, D)
            out = conn.attend_layers(0, layers, rids, q, sm)               # every layer of the step: one call
            worst = apart = 0.0
            for layer in range(layers):
                w, tol = bound(layer, q[layer], out[layer])
                one = conn.attend(layer, rids, q[layer], sm)               # the per-layer route: a batch call and a tail fold
                worst, apart = max(worst, w), max(apart, float(((out[layer] - one).abs().cpu().numpy() / tol).max()))
            assert worst <= 1.0 and apart <= 2.0, (step, worst, apart)
            k_new, v_new = rnd(len(rids), 1, layers, H, D), rnd(len(rids), 1, layers, H, D)
            keep += conn.commit(rids, k_new, v_new, [1] * len(rids))
            for b, rid in enumerate(rids):
                rows[rid][0] = np.concatenate([rows[rid][0], k_new[b].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
                rows[rid][1] = np.concatenate([rows[rid][1], v_new[b].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
            if verbose:
                print(f"decode step {step}: lengths {[conn.length(r) for r in rids]}, worst err / tol {worst:.3f}, apart from attend {apart:.3f} tol")
        torch.cuda.synchronize()
        assert [conn.length(r) for r in rids] == [n + steps for n in prompts]
        if verbose:
            print(f"ok: {steps} decode steps over {len(rids)} requests x {layers} layers, one library call per step")
        return steps
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    run(steps=a.steps)
