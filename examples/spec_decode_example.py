#!/usr/bin/env python3
"""Speculative decoding over the compressed KV pool: verify S draft positions per request in ONE pass over the records.

A toy loop on an MI355X.  Per step a "draft" proposes S tokens per request (random K / V rows and queries stand in for a
model), `SpeckvKVConnector.attend_spec` computes the attention of all S positions causally -- position j sees the request's
stored context and the drafts 0..j -- from one pass over the compressed records, a random prefix of the drafts is
"accepted", and `append_tokens` commits exactly that prefix.

Every step is checked against the single-token path the library had before: a second connector receives the accepted
positions one `append` at a time and answers each with `attend`.  The two agree within the pool format's quantisation
(a draft position is fp16 while it is verified, compressed once committed), and after the commit both connectors hold
the same bits: lengths, rows, and the next attention.

    python examples/spec_decode_example.py [--steps 6] [--draft 4] [--scheme fp8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(steps=6, S=4, scheme="fp8", layers=2, rows_per_pos=4, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T = 8, 128, 512
        spec = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        eager = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(3)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(3)
        prompts = [64, 97, 150]
        ids, ids_e = [1, 2, 3], [101, 102, 103]
        keep = []
        for rid, rid_e, n in zip(ids, ids_e, prompts):
            k, v = rnd(layers, n, H, D), rnd(layers, n, H, D)
            spec.add_request(rid); eager.add_request(rid_e)
            keep += spec.write_prefill(rid, k, v) + eager.write_prefill(rid_e, k, v)
        B, sm = len(ids), 1.0 / np.sqrt(D)
        accepted_total, worst = 0, 0.0
        for step in range(steps):
            k_new, v_new = rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)       # the draft's S positions per request
            q = rnd(layers, B, S, H, rows_per_pos, D)
            out = [spec.attend_spec(layer, ids, q[layer], k_new, v_new, sm) for layer in range(layers)]     # [B][S][H][rows][D] each
            n_accept = [int(x) for x in rng.integers(0, S + 1, B)]                # the verifier's verdict: a prefix per request
            n_accept[step % B] = S if step % 2 else 1
            # the single-token path: the accepted positions one at a time
            for j in range(max(n_accept)):
                members = [b for b in range(B) if n_accept[b] > j]
                idx = torch.tensor(members, device="cuda")
                keep += eager.append([ids_e[b] for b in members], k_new[idx, j], v_new[idx, j])
                for layer in range(layers):
                    one = eager.attend(layer, [ids_e[b] for b in members], q[layer][idx, j].contiguous(), sm)     # [n][H][rows][D]
                    got = out[layer][idx, j]
                    rel = float((got - one).norm() / one.norm())
                    worst = max(worst, rel)
                    assert rel <= 0.05, (step, j, layer, rel)
            keep += spec.append_tokens(ids, k_new, v_new, n_accept)
            accepted_total += sum(n_accept)
            # after the commit: the same state, bit for bit
            qn = rnd(B, H, rows_per_pos, D)
            for rid, rid_e in zip(ids, ids_e):
                assert spec.length(rid) == eager.length(rid_e)
            for layer in range(layers):
                assert torch.equal(spec.attend(layer, ids, qn, sm), eager.attend(layer, ids_e, qn, sm)), (step, layer)
            torch.cuda.synchronize()
            keep = keep[-8:]
        result = {"steps": steps, "draft": S, "accepted": accepted_total, "lengths": [spec.length(r) for r in ids],
                  "worst_relative_difference": round(worst, 5)}
        if verbose:
            print(result)
            print("spec decode example ok")
        for rid, rid_e in zip(ids, ids_e):
            spec.free_request(rid); eager.free_request(rid_e)
        return result
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--draft", type=int, default=4)
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "int4", "mxfp4"])
    a = ap.parse_args()
    run(a.steps, a.draft, a.scheme)
