#!/usr/bin/env python3
"""Parallel sampling over the compressed KV pool: one prompt forked into four continuations.

A toy loop on an MI355X.  One request holds a prompt (random K / V rows stand in for a model).  `SpeckvKVConnector.fork` starts
four more requests from it -- ONE `speckv_ext_copy_runs` launch copies the prompt's stored records, nothing is decoded or
compressed again -- and every continuation then appends tokens of its own, one per step.

Every continuation is checked against an independently written twin: a request that got the same prompt through `write_prefill`
and the same tokens through `append`.  Lengths, tails, every stored row (bit for bit) and the attention output (bit for bit: the
records are the same) must agree, and the prompt's request must be untouched throughout.

    python examples/fork_example.py [--steps 6] [--scheme fp8] [--prompt 97]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(steps=6, scheme="fp8", prompt=97, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G, N = 8, 128, 512, 4, 4
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(13)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        k, v = rnd(layers, prompt, H, D), rnd(layers, prompt, H, D)
        root, forks, twins = 1, [11, 12, 13, 14], [21, 22, 23, 24]
        conn.add_request(root)
        keep = conn.write_prefill(root, k, v)
        for rid in twins:
            conn.add_request(rid)
            keep += conn.write_prefill(rid, k, v)
        keep += conn.fork([root] * N, forks)                    # one prompt, four continuations: one launch
        rows = lambda rid: [conn.kv_rows(rid, layer, kind).view(torch.int16) for layer in range(layers) for kind in (0, 1)]
        prompt_rows = rows(root)
        sm = 1.0 / np.sqrt(D)
        for step in range(steps):
            k_new, v_new = rnd(N, layers, H, D), rnd(N, layers, H, D)       # every continuation appends different tokens
            keep += conn.append(forks, k_new, v_new)
            keep += conn.append(twins, k_new, v_new)
            q = rnd(N, H, G, D)
            for layer in range(layers):
                x, y = conn.attend(layer, forks, q, sm), conn.attend(layer, twins, q, sm)
                assert bool(torch.isfinite(x).all())
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (step, layer)
            for fork, twin in zip(forks, twins):
                assert conn.length(fork) == conn.length(twin) == prompt + step + 1
                assert (conn.requests[fork].tail_k is None) == (conn.requests[twin].tail_k is None)
                assert all(torch.equal(a, b) for a, b in zip(rows(fork), rows(twin))), (step, fork)
            if verbose:
                print(f"step {step}: lengths {[conn.length(r) for r in forks]}")
        assert conn.length(root) == prompt and all(torch.equal(a, b) for a, b in zip(rows(root), prompt_rows))
        a, b = rows(forks[0]), rows(forks[1])
        assert not any(torch.equal(x[prompt:], y[prompt:]) for x, y in zip(a, b)), "the continuations did not diverge"
        conn.free_request(root)                                 # the continuations do not need the prompt's request
        assert all(torch.equal(x, y) for x, y in zip(rows(forks[0]), a))
        if verbose:
            print(f"ok: a prompt of {prompt} positions forked into {N} continuations of {steps} steps, each equal to its twin bit for bit")
        return steps
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--prompt", type=int, default=97)
    a = ap.parse_args()
    run(a.steps, a.scheme, a.prompt)
