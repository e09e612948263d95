#!/usr/bin/env python3
"""Chunked prefill over the compressed KV pool: a prompt goes in through chunks of unequal length.

A toy loop on an MI355X.  Random K / V rows stand in for a model.  For every chunk and every layer
`SpeckvKVConnector.attend_chunk` computes the causal attention of the chunk's positions over everything the request holds already
-- ONE `speckv_ext_attend_chunk` launch, whatever the chunk's length -- and `commit` then stores the chunk (one
`speckv_ext_write_pairs` launch).  One `attend` decode step follows.

The request is checked against a twin that got the same prompt in one piece through `write_prefill`: lengths, every stored row
and the decode step's attention output must agree bit for bit, and the chunks' attention is held to a float32 softmax attention over
the rows the twin holds.

    python examples/chunked_prefill_example.py [--scheme fp8] [--chunks 100,33,260,1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(scheme="fp8", chunks=(100, 33, 260, 1), layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 4
        total = sum(chunks)
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(17)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        k, v = rnd(layers, total, H, D), rnd(layers, total, H, D)
        chunked, twin = 1, 2
        conn.add_request(chunked)
        conn.add_request(twin)
        keep = conn.write_prefill(twin, k, v)
        stored = [[conn.kv_rows(twin, layer, kind).to(torch.float32) for kind in (0, 1)] for layer in range(layers)]    # [n][H][D]
        sm, at = 1.0 / np.sqrt(D), 0
        for n in chunks:
            k_new = k[:, at:at + n].permute(1, 0, 2, 3)[None]               # [1][n][layers][heads][dim], read in place
            v_new = v[:, at:at + n].permute(1, 0, 2, 3)[None]
            for layer in range(layers):
                q = rnd(1, n, H, G, D)
                out = conn.attend_chunk(layer, [chunked], q, k_new, v_new, sm)
                # what the chunk should see: the stored rows in front of it as the pool holds them, the chunk's own rows as they are
                pool = conn.length(chunked) & ~1
                kk = torch.cat((stored[layer][0][:pool], k[layer, pool:at + n].to(torch.float32)))
                vv = torch.cat((stored[layer][1][:pool], v[layer, pool:at + n].to(torch.float32)))
                s = torch.einsum("nhgd,thd->nhgt", q[0].to(torch.float32), kk) * sm
                sees = at + torch.arange(n, device="cuda")[:, None, None, None] >= torch.arange(at + n, device="cuda")[None, None, None, :]
                want = torch.einsum("nhgt,thd->nhgd", torch.softmax(s.masked_fill(~sees, float("-inf")), dim=-1), vv)
                err = float((out[0] - want).abs().max())
                assert err < 2e-2, (n, layer, err)
            keep += conn.commit([chunked], k_new, v_new, [range(n)])
            at += n
            if verbose:
                print(f"chunk of {n:4d}: length {conn.length(chunked)}")
        assert conn.length(chunked) == conn.length(twin) == total
        for layer in range(layers):
            for kind in (0, 1):
                a, b = conn.kv_rows(chunked, layer, kind), conn.kv_rows(twin, layer, kind)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (layer, kind)
            q = rnd(1, H, G, D)
            x, y = conn.attend(layer, [chunked], q, sm), conn.attend(layer, [twin], q, sm)
            assert bool(torch.isfinite(x).all()) and torch.equal(x.view(torch.int32), y.view(torch.int32)), layer
        torch.cuda.synchronize()
        if verbose:
            print(f"ok: a prompt of {total} positions in chunks of {list(chunks)} equals its write_prefill twin bit for bit")
        return total
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--chunks", default="100,33,260,1")
    a = ap.parse_args()
    run(a.scheme, tuple(int(c) for c in a.chunks.split(",")))
