#!/usr/bin/env python3
"""Optimistic commit and rollback over the compressed KV pool: commit the whole draft chain, cut back when the accept count arrives.

A toy loop on an MI355X.  Per step a "draft" proposes a chain of 4 tokens per request (random K / V rows and queries stand in for
a model).  The optimistic connector commits all 4 at once (`SpeckvKVConnector.commit`, one launch) without waiting for the
sampler; when the "verifier" answers -- a random accept count 0..4 per request -- `truncate` rolls every request back to the
accepted length.  A request that lands on an odd length inside pairs already stored gets its new last position back out of the
pool as its tail, one `speckv_ext_read_pairs` launch for the whole batch.

Every step is checked against the path that waits: a second connector commits only the accepted prefix (`append_tokens`).  The
two must agree on lengths and on which requests hold a tail; every position in front of a pair the rollback reopened must agree
bit for bit; and the next attention must agree closely (not bit for bit: a row read back has been through the format once, and
its pair is encoded again with its new partner).

    python examples/spec_rollback_example.py [--steps 6] [--scheme fp8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(steps=6, scheme="fp8", layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, S, G = 8, 128, 512, 4, 4
        optimistic = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        waiting = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(9)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(9)
        prompts = [64, 97, 150]
        ids, ids_w = [1, 2, 3], [101, 102, 103]
        keep = []
        for rid, rid_w, n in zip(ids, ids_w, prompts):
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            optimistic.add_request(rid); waiting.add_request(rid_w)
            keep += optimistic.write_prefill(rid, k, v) + waiting.write_prefill(rid_w, k, v)
        B, sm = len(ids), 1.0 / np.sqrt(D)
        rolled_back, worst = 0, 0.0
        reopened = [None] * B                                   # first position whose pair a rollback has had written again
        for step in range(steps):
            k_new, v_new = rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            keep += optimistic.commit(ids, k_new, v_new, [list(range(S))] * B)          # the whole chain, before the verifier answers
            n_accept = [int(rng.integers(0, S + 1)) for _ in range(B)]
            before = [optimistic.length(rid) for rid in ids]
            optimistic.truncate(ids, [n - S + a for n, a in zip(before, n_accept)])
            keep += waiting.append_tokens(ids_w, k_new, v_new, n_accept)
            rolled_back += sum(S - a for a in n_accept)
            for b, (rid, rid_w) in enumerate(zip(ids, ids_w)):
                n = optimistic.length(rid)
                assert n == waiting.length(rid_w), (step, rid)
                assert (optimistic.requests[rid].tail_k is None) == (waiting.requests[rid_w].tail_k is None) == (n % 2 == 0), (step, rid)
                if n & 1 and n_accept[b] < S:                   # a position came back out of the pool: its pair will be written again
                    reopened[b] = n - 1 if reopened[b] is None else min(reopened[b], n - 1)
                same = n if reopened[b] is None else min(n, reopened[b])
                for layer in range(layers):
                    for kind in (0, 1):
                        x, y = optimistic.kv_rows(rid, layer, kind, 0, same), waiting.kv_rows(rid_w, layer, kind, 0, same)
                        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (step, rid, layer, kind)
            q = rnd(B, H, G, D)
            for layer in range(layers):
                x, y = optimistic.attend(layer, ids, q, sm), waiting.attend(layer, ids_w, q, sm)
                assert bool(torch.isfinite(x).all())
                worst = max(worst, float((x - y).abs().max()))
            if verbose:
                print(f"step {step}: accepted {n_accept}, lengths {[optimistic.length(r) for r in ids]}")
        # the rows that differ went through a 4- or 8-bit format once more: the attention outputs (|v| ~ 1, averaged over the context) stay close
        assert worst < 0.1, worst
        if verbose:
            print(f"ok: {steps} steps, {rolled_back} positions rolled back, attention of the two connectors within {worst:.2e}")
        return rolled_back, worst
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    a = ap.parse_args()
    run(a.steps, a.scheme)
