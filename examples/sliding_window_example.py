#!/usr/bin/env python3
"""Sliding-window layers over the compressed KV pool: a stack whose layers alternate local and global attention.

A toy loop on an MI355X.  Random K / V rows stand in for a model whose even layers are LOCAL (a query position sees itself and the
`--window` - 1 positions in front of it) and whose odd layers are GLOBAL (it sees everything), as the Mistral family, Gemma 2 / 3 and
gpt-oss interleave them.  The prompt goes in through chunks of unequal length, then single positions follow as decode steps.  For every
chunk, every step and every layer ONE call does the attention: `SpeckvKVConnector.attend_chunk(..., window=W)` on a local layer
(`speckv_ext_attend_chunk_window`: the kernel walks only the tiles the window covers), the same call without a window on a global one;
S = 1 is the decode step -- the request's length may be odd or even.  `commit` stores the new positions afterwards; records below a
window stay in the pool.

Every output is held to a float32 softmax attention in torch, on the device, over the rows a `write_prefill` twin of the whole
sequence holds in the pool and the new rows as they are, masked to the layer's window.

    python examples/sliding_window_example.py [--scheme fp8] [--window 64] [--chunks 100,33,260,1] [--steps 6]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(scheme="fp8", window=64, chunks=(100, 33, 260, 1), steps=6, layers=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 4
        total = sum(chunks) + steps
        assert total <= T
        windows = [window if layer % 2 == 0 else None for layer in range(layers)]        # local, global, local, ...
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        k, v = rnd(layers, total, H, D), rnd(layers, total, H, D)
        req, twin = 1, 2
        conn.add_request(req)
        conn.add_request(twin)
        keep = conn.write_prefill(twin, k, v)
        stored = [[conn.kv_rows(twin, layer, kind).to(torch.float32) for kind in (0, 1)] for layer in range(layers)]    # [n][H][D]
        sm, at = 1.0 / np.sqrt(D), 0
        worst = {"local": 0.0, "global": 0.0}

        def attend(n):
            """one step of n new positions at `at`: every layer's attention against its torch reference"""
            k_new = k[:, at:at + n].permute(1, 0, 2, 3)[None]               # [1][n][layers][heads][dim], read in place
            v_new = v[:, at:at + n].permute(1, 0, 2, 3)[None]
            for layer, w in enumerate(windows):
                q = rnd(1, n, H, G, D)
                out = conn.attend_chunk(layer, [req], q, k_new, v_new, sm, splits=0, window=w)
                pool = conn.length(req) & ~1                                  # stored rows as the pool holds them, the rest as they are
                kk = torch.cat((stored[layer][0][:pool], k[layer, pool:at + n].to(torch.float32)))
                vv = torch.cat((stored[layer][1][:pool], v[layer, pool:at + n].to(torch.float32)))
                s = torch.einsum("nhgd,thd->nhgt", q[0].to(torch.float32), kk) * sm
                P = at + torch.arange(n, device="cuda")[:, None, None, None]
                t = torch.arange(at + n, device="cuda")[None, None, None, :]
                sees = (t <= P) if w is None else (t <= P) & (t > P - w)
                want = torch.einsum("nhgt,thd->nhgd", torch.softmax(s.masked_fill(~sees, float("-inf")), dim=-1), vv)
                err = float((out[0] - want).abs().max())
                assert bool(torch.isfinite(out).all()) and err < 2e-2, (n, layer, w, err)
                kind = "global" if w is None else "local"
                worst[kind] = max(worst[kind], err)
            return k_new, v_new

        for n in chunks:
            k_new, v_new = attend(n)
            keep += conn.commit([req], k_new, v_new, [range(n)])
            at += n
            if verbose:
                print(f"prefill chunk of {n:4d}: length {conn.length(req):4d}, worst |err| local (W = {window}) {worst['local']:.2e}, "
                      f"global {worst['global']:.2e}")
        for _ in range(steps):
            k_new, v_new = attend(1)
            keep += conn.commit([req], k_new, v_new, [range(1)])
            at += 1
            if verbose:
                print(f"decode step (S = 1): length {conn.length(req):4d}, worst |err| local {worst['local']:.2e}, global {worst['global']:.2e}")
        torch.cuda.synchronize()
        assert conn.length(req) == total
        for layer in range(layers):                                           # nothing was freed: the pool holds what the twin holds
            for kind in (0, 1):
                a, b = conn.kv_rows(req, layer, kind), conn.kv_rows(twin, layer, kind)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (layer, kind)
        if verbose:
            print(f"ok: {layers} layers (local W = {window} / global alternating), {sum(chunks)} prompt positions in chunks of "
                  f"{list(chunks)} and {steps} decode steps agree with the torch reference")
        return total
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--chunks", default="100,33,260,1")
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    run(a.scheme, a.window, tuple(int(c) for c in a.chunks.split(",")), a.steps)
