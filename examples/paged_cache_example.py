#!/usr/bin/env python3
"""Paged caches and the compressed KV pool: store two prompts from vLLM-style blocks, free the blocks, load them into other blocks.

A toy on an MI355X.  The "model" has filled per-layer paged caches ([2, blocks, block_size, 8, 128] fp16: vLLM's layout) with the
K / V rows of two prompts, scattered over blocks by a slot mapping.  `SpeckvKVConnector.store_paged` encodes both prompts into the
pool with ONE launch (`speckv_ext_write_slots`: the encoder reads every row where its slot is, no gathered copy of the prompt
exists); the blocks are then "freed" (overwritten); `load_paged` decodes the prompts into a different set of blocks with ONE launch
(`speckv_ext_read_slots`).  What arrives is compared with the rows the pool returns by the row route (`kv_rows`), bit for bit, and
with the rows that were stored, within the format's error.

    python examples/paged_cache_example.py [--scheme fp8]
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
        gen = torch.Generator(device="cuda"); gen.manual_seed(3)
        caches = [torch.zeros((2, NB, BS, H, D), dtype=torch.float16, device="cuda") for _ in range(layers)]
        prompts = {1: 75, 2: 128}                                   # an odd length (its last position is held as the tail) and an even one
        perm = torch.randperm(NB, generator=torch.Generator().manual_seed(3)).tolist()

        def slots_of(blocks, n):                                    # vLLM's rule: block * block_size + offset
            return [blocks[t // BS] * BS + t % BS for t in range(n)]

        # the forward pass of the prefill fills the blocks
        truth, stored_in, at = {}, {}, 0
        for rid, n in prompts.items():
            need = (n + BS - 1) // BS
            stored_in[rid] = slots_of(perm[at:at + need], n)
            at += need
            idx = torch.tensor(stored_in[rid], device="cuda")
            for layer, cache in enumerate(caches):
                rows = torch.randn((2, n, H, D), generator=gen, device="cuda").to(torch.float16)
                cache.view(2, NB * BS, H, D)[:, idx] = rows
                truth[(rid, layer)] = rows
            conn.add_request(rid)
        ids = list(prompts)
        mapping = torch.tensor([s for rid in ids for s in stored_in[rid]], dtype=torch.int64, device="cuda")
        conn.store_paged(ids, [prompts[r] for r in ids], mapping, caches)               # ONE launch for both prompts and all layers
        torch.cuda.synchronize()
        assert [conn.length(r) for r in ids] == [prompts[r] for r in ids]
        # the blocks are freed and used by somebody else
        for cache in caches:
            cache.fill_(-1.0)
        # ... and the prompts come back into other blocks
        back = perm[::-1]
        loaded_in, at = {}, 0
        for rid, n in prompts.items():
            need = (n + BS - 1) // BS
            loaded_in[rid] = slots_of(back[at:at + need], n)
            at += need
        mapping = torch.tensor([s for rid in ids for s in loaded_in[rid]], dtype=torch.int64, device="cuda")
        conn.load_paged(ids, [0] * len(ids), [prompts[r] for r in ids], mapping, caches)   # ONE launch again
        torch.cuda.synchronize()
        worst = 0.0
        for rid, n in prompts.items():
            idx = torch.tensor(loaded_in[rid], device="cuda")
            for layer, cache in enumerate(caches):
                got = cache.view(2, NB * BS, H, D)[:, idx]
                for kind in (0, 1):
                    rows = conn.kv_rows(rid, layer, kind)                                 # the row route: fetch + decompress
                    assert torch.equal(got[kind].view(torch.int16), rows.view(torch.int16)), (rid, layer, kind)
                err = float((got.float() - truth[(rid, layer)].float()).abs().max() / truth[(rid, layer)].float().abs().max())
                worst = max(worst, err)
        assert worst < 0.3, worst                                    # 4-bit formats: a quantisation step of the largest group
        if verbose:
            print(f"paged cache example ok: {sum(prompts.values())} positions x {layers} layers stored and loaded with one launch each way "
                  f"({scheme}, largest relative error {worst:.3f})")
        return worst
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="fp8", choices=["fp16", "fp8", "int4", "mxfp4"])
    run(ap.parse_args().scheme)
