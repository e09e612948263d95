#!/usr/bin/env python3
"""Decode steps over a stack that alternates sliding-window and global layers, straight from the compressed KV pool.

A toy loop on an MI355X.  Random K / V rows stand in for a model whose even layers are LOCAL (the new position sees itself and the
`--window` - 1 positions in front of it) and whose odd layers are GLOBAL, as the Mistral family, Gemma 2 / 3 and gpt-oss interleave
them.  A batch of requests with prompts of different lengths decodes in lockstep: `append` stores the step's position, then every
layer's attention is ONE call, `SpeckvKVConnector.attend(layer, ids, q, sm, window=W)` on a local layer and the same call without a
window on a global one.  The connector keeps one launch plan per window value beside the global one (`plan_step(window=W)`), so a step
plans twice and launches once per layer; a local layer's launch walks the tiles its window covers
(`SpeckvKVConnector.decode_window_range`), never the context.

Every output is held to a float32 softmax attention in torch, on the device, over the rows `kv_rows` reads back from the pool, masked
to the layer's window.

    python examples/sliding_window_decode_example.py [--scheme fp8] [--window 48] [--prompts 100,33,260,48] [--steps 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(scheme="fp8", window=48, prompts=(100, 33, 260, 48), steps=8, layers=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 4
        assert max(prompts) + steps <= T
        windows = [window if layer % 2 == 0 else None for layer in range(layers)]        # local, global, local, ...
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(29)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        ids = list(range(1, len(prompts) + 1))
        keep = []
        for rid, n in zip(ids, prompts):
            conn.add_request(rid)
            keep += conn.write_prefill(rid, rnd(layers, n, H, D), rnd(layers, n, H, D))
        sm = 1.0 / np.sqrt(D)
        worst = {"local": 0.0, "global": 0.0}
        for step in range(steps):
            keep.append(conn.append(ids, rnd(len(ids), layers, H, D), rnd(len(ids), layers, H, D)))      # the step's own position
            for layer, w in enumerate(windows):
                q = rnd(len(ids), H, G, D)
                out = conn.attend(layer, ids, q, sm, window=w)
                for b, rid in enumerate(ids):
                    n = conn.length(rid)
                    lo = max(0, n - w) if w else 0                                          # the query at n - 1 sees [lo, n - 1]
                    kk = conn.kv_rows(rid, layer, 0, lo, n).to(torch.float32)               # [positions][heads][dim], the tail included
                    vv = conn.kv_rows(rid, layer, 1, lo, n).to(torch.float32)
                    s = torch.einsum("hgd,thd->hgt", q[b].to(torch.float32), kk) * sm
                    want = torch.einsum("hgt,thd->hgd", torch.softmax(s, dim=-1), vv)
                    err = float((out[b] - want).abs().max())
                    # (the reference takes the fp16 query as it is, the kernels quantise it to the pool's format: a few 1e-2 over a short window)
                    assert bool(torch.isfinite(out[b]).all()) and err < 8e-2, (step, layer, w, rid, err)
                    kind = "global" if w is None else "local"
                    worst[kind] = max(worst[kind], err)
            if verbose:
                walked = [SpeckvKVConnector.decode_window_range(conn.length(rid), window)[2] for rid in ids]
                print(f"step {step}: lengths {[conn.length(r) for r in ids]}, pages a local layer walks {walked} of "
                      f"{[conn.length(r) // 2 for r in ids]}, worst |err| local (W = {window}) {worst['local']:.2e}, global {worst['global']:.2e}")
        torch.cuda.synchronize()
        del keep
        if verbose:
            print(f"ok: {steps} decode steps of {len(ids)} requests over {layers} layers (local W = {window} / global alternating) agree "
                  f"with the torch reference")
        return steps
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--window", type=int, default=48)
    ap.add_argument("--prompts", default="100,33,260,48")
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    run(a.scheme, a.window, tuple(int(c) for c in a.prompts.split(",")), a.steps)
