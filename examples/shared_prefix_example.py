#!/usr/bin/env python3
"""Parallel sampling WITHOUT copies of the prompt: N samples share one stored prompt.

A toy loop on an MI355X.  One request holds a prompt (random K / V rows stand in for a model).  The N samples are ordinary requests
that start EMPTY and hold only what they generate; every decode step runs `SpeckvKVConnector.attend_shared`, which attends each
sample's own positions exactly as `attend` does and then folds in the prompt with ONE `speckv_ext_attend_prefix_fold` launch -- a
workgroup walks the prompt's records once for 64 query rows of the samples, where `fork` + `attend` stores the prompt N times and
reads it N times per step.

Every sample is compared with a forked twin (`fork` + the same tokens through `append` + `attend`).  The two routes are two
different roundings of the same softmax -- the twin's kernel may quantise the query for the prompt's positions too -- so the outputs
agree within a tolerance that follows the pool format, not bit for bit; lengths and tails agree exactly (prompt aside).

    python examples/shared_prefix_example.py [--scheme int4] [--prompt 98] [--samples 8] [--steps 6]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# largest |difference| of the two routes' outputs over the largest |output|: INT4 pools take the fp16 query on both routes; FP8 and
# MXFP4 pools quantise the query in attend() and not in the prefix part of attend_shared()
AGREE = {"int4": 2e-2, "fp8": 0.15, "mxfp4": 0.15}


def run(scheme="int4", prompt=98, samples=8, steps=6, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 4
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(17)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        k, v = rnd(layers, prompt, H, D), rnd(layers, prompt, H, D)
        root, members, twins = 1, list(range(100, 100 + samples)), list(range(200, 200 + samples))
        conn.add_request(root)
        keep = conn.write_prefill(root, k, v)
        for rid in members:                                     # a sample holds nothing yet: no copy of the prompt
            conn.add_request(rid)
        keep += conn.fork([root] * samples, twins)              # the route this one replaces: the prompt once per sample
        shared = prompt & ~1                                    # whole stored pairs can be shared ...
        if prompt & 1:                                          # ... an odd last position goes into every sample as its first own one
            keep += conn.append(members, k[:, -1][None].expand(samples, -1, -1, -1).contiguous(), v[:, -1][None].expand(samples, -1, -1, -1).contiguous())
        sm, checked = 1.0 / np.sqrt(D), 0
        for step in range(steps):
            q = rnd(samples, H, G, D)
            for layer in range(layers):
                x = conn.attend_shared(layer, members, [root] * samples, q, sm, prefix_lens=[shared] * samples)
                y = conn.attend(layer, twins, q, sm)
                assert bool(torch.isfinite(x).all())
                diff = float((x - y).abs().max() / y.abs().max())
                assert diff <= AGREE[scheme], (step, layer, diff)
            checked += samples
            k_new, v_new = rnd(samples, layers, H, D), rnd(samples, layers, H, D)       # every sample appends a token of its own
            keep += conn.append(members, k_new, v_new)
            keep += conn.append(twins, k_new, v_new)
            for m, t in zip(members, twins):
                assert conn.length(m) + shared == conn.length(t)
                assert (conn.requests[m].tail_k is None) == (conn.requests[t].tail_k is None)
            if verbose:
                print(f"step {step}: samples hold {conn.length(members[0])} positions of their own, twins {conn.length(twins[0])}; "
                      f"largest relative difference of the last layer {diff:.4f}")
        torch.cuda.synchronize()
        assert conn.length(root) == prompt
        if verbose:
            print(f"ok: {samples} samples over one stored prompt of {prompt} positions, {steps} steps, each within {AGREE[scheme]} of its forked twin")
        return checked
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="int4", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--prompt", type=int, default=98)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    run(a.scheme, a.prompt, a.samples, a.steps)
