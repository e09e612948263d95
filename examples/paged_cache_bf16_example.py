#!/usr/bin/env python3
"""bf16 paged caches and the compressed KV pool: a chunked prefill with an odd seam, two decode steps, a load into fresh blocks.

A toy on an MI355X.  The "model" keeps its KV cache in bf16 ([2, blocks, block_size, 8, 128]: vLLM's layout).  The prompt is stored
in two chunks, the first of odd length: `store_paged(..., fused=True)` is ONE launch per chunk (`speckv_ext_write_slots_ex`) -- the
encoder reads the bf16 rows where their slots are and rounds each element once to fp16; the odd last position of the first chunk
comes back as a held fp16 row (the connector's tail), and the second chunk's launch pairs that row with its first cache row.  Two
decode `append`s follow.  `load_paged(..., fused=True)` then decodes everything into other bf16 blocks with ONE launch
(`speckv_ext_read_slots_ex`), the tail included, and the blocks are compared with `kv_rows(...).to(bfloat16)` bit for bit.

    python examples/paged_cache_bf16_example.py [--scheme fp8]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(scheme="fp8", layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, BS, NB = 8, 128, 256, 16, 32
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(11)
        caches = [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16, device="cuda") for _ in range(layers)]
        n_prompt, seam = 75, 37                                     # chunks of 37 and 38 positions: the seam falls inside a pair
        blocks = torch.randperm(NB, generator=torch.Generator().manual_seed(11)).tolist()
        slots = [blocks[t // BS] * BS + t % BS for t in range(n_prompt)]             # vLLM's rule: block * block_size + offset
        idx = torch.tensor(slots, device="cuda")
        for cache in caches:                                        # the forward pass of the prefill fills the blocks
            cache.view(2, NB * BS, H, D)[:, idx] = torch.randn((2, n_prompt, H, D), generator=gen, device="cuda").to(torch.bfloat16)
        conn.add_request(1)
        keep = []
        for lo, hi in ((0, seam), (seam, n_prompt)):
            mapping = torch.tensor(slots[lo:hi], dtype=torch.int64, device="cuda")
            keep += conn.store_paged([1], [hi - lo], mapping, caches, fused=True)        # ONE launch per chunk, all layers
            keep.append(mapping)
        for _ in range(2):                                          # two decode steps: the first completes the pair of position 74
            k_new = torch.randn((1, layers, H, D), generator=gen, device="cuda").to(torch.float16)
            v_new = torch.randn((1, layers, H, D), generator=gen, device="cuda").to(torch.float16)
            keep.append(conn.append([1], k_new, v_new))
        torch.cuda.synchronize()
        n = conn.length(1)
        assert n == n_prompt + 2
        fresh = [torch.full((2, NB, BS, H, D), -1.0, dtype=torch.bfloat16, device="cuda") for _ in range(layers)]
        back = blocks[::-1]
        into = torch.tensor([back[t // BS] * BS + t % BS for t in range(n)], dtype=torch.int64, device="cuda")
        conn.load_paged([1], [0], [n], into, fresh, fused=True)     # ONE launch, the held last position included
        torch.cuda.synchronize()
        for layer, cache in enumerate(fresh):
            got = cache.view(2, NB * BS, H, D)[:, into]
            for kind in (0, 1):
                want = conn.kv_rows(1, layer, kind).to(torch.bfloat16)
                assert torch.equal(got[kind].view(torch.int16), want.view(torch.int16)), (layer, kind)
        if verbose:
            print(f"paged cache bf16 example ok: {n_prompt} positions in chunks of {seam} and {n_prompt - seam}, 2 appended, x {layers} "
                  f"layers stored from and loaded into bf16 blocks with one launch per call ({scheme})")
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp16", "fp8", "int4", "mxfp4"])
    run(ap.parse_args().scheme)
