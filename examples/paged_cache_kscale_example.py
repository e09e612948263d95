#!/usr/bin/env python3
"""A 4-bit pool with the K pre-scale, fed from paged caches by the one launch: chunked prefill with an odd seam, load, decode.

A toy on an MI355X.  The pool is INT4_G32, and what makes a 4-bit pool usable is the per-channel power-of-two K pre-scale
(`calibrate_k_channel_scale`: K / scale in the pool, q * scale against it), here calibrated from the prompt's K, which has a few
outlier channels.  The "model" keeps its KV cache in fp16 blocks ([2, blocks, block_size, 8, 128]: vLLM's layout).  The prompt is
stored in two chunks, the first of odd length: `store_paged(..., fused=True, kscale=True)` is ONE launch per chunk
(`speckv_ext_write_slots_kmul`) -- the encoder reads the rows where their slots are and multiplies every K element by its channel's
inverse scale on the way; the odd last position of the first chunk comes back as a held row (the connector's tail, pre-scaled like
every tail), and the second chunk's launch pairs that row with its first cache row.  `load_paged(..., fused=True, kscale=True)` then
decodes everything into other blocks with ONE launch (`speckv_ext_read_slots_kmul`), scaled back.  The twin is a connector with the
same pre-scale on the row route (`write_prefill` of the gathered prompt): the loaded blocks, and the attention output of a decode
step after an `append`, are equal to the bit.

    python examples/paged_cache_kscale_example.py [--scheme int4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(scheme="int4", layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, BS, NB, G = 8, 128, 256, 16, 32, 4
        conn, twin = SpeckvKVConnector(lib, layers, H, D, T, scheme), SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(11)
        caches = [torch.zeros((2, NB, BS, H, D), dtype=torch.float16, device="cuda") for _ in range(layers)]
        n_prompt, seam = 75, 37                                     # chunks of 37 and 38 positions: the seam falls inside a pair
        blocks = torch.randperm(NB, generator=torch.Generator().manual_seed(11)).tolist()
        slots = [blocks[t // BS] * BS + t % BS for t in range(n_prompt)]             # vLLM's rule: block * block_size + offset
        idx = torch.tensor(slots, device="cuda")
        for cache in caches:                                        # the forward pass of the prefill fills the blocks
            kv = torch.randn((2, n_prompt, H, D), generator=gen, device="cuda")
            kv[0, :, :, 5::32] *= 12.0                              # K has outlier channels: what the pre-scale is for
            cache.view(2, NB * BS, H, D)[:, idx] = kv.to(torch.float16)
        k = torch.stack([c.view(2, NB * BS, H, D)[0, idx] for c in caches])          # [layers][tokens][heads][dim]
        v = torch.stack([c.view(2, NB * BS, H, D)[1, idx] for c in caches])
        scale = conn.calibrate_k_channel_scale(k)
        twin.set_k_channel_scale(scale)
        assert float(scale.max()) > 1.0
        conn.add_request(1)
        twin.add_request(1)
        keep = []
        for lo, hi in ((0, seam), (seam, n_prompt)):
            mapping = torch.tensor(slots[lo:hi], dtype=torch.int64, device="cuda")
            keep += conn.store_paged([1], [hi - lo], mapping, caches, fused=True, kscale=True)     # ONE launch per chunk, all layers
            keep.append(mapping)
        keep += twin.write_prefill(1, k.contiguous(), v.contiguous())                # the row route: gathered, scaled by torch, written
        torch.cuda.synchronize()
        assert conn.length(1) == twin.length(1) == n_prompt
        fresh = [torch.full((2, NB, BS, H, D), -1.0, dtype=torch.float16, device="cuda") for _ in range(layers)]
        back = blocks[::-1]
        into = torch.tensor([back[t // BS] * BS + t % BS for t in range(n_prompt)], dtype=torch.int64, device="cuda")
        conn.load_paged([1], [0], [n_prompt], into, fresh, fused=True, kscale=True)  # ONE launch, the held last position included
        torch.cuda.synchronize()
        for layer, cache in enumerate(fresh):
            got = cache.view(2, NB * BS, H, D)[:, into]
            for kind in (0, 1):
                want = twin.kv_rows(1, layer, kind)
                assert torch.equal(got[kind].view(torch.int16), want.view(torch.int16)), (layer, kind)
        k_new = torch.randn((1, layers, H, D), generator=gen, device="cuda").to(torch.float16)      # a decode step on both
        v_new = torch.randn((1, layers, H, D), generator=gen, device="cuda").to(torch.float16)
        keep.append(conn.append([1], k_new, v_new))
        keep.append(twin.append([1], k_new, v_new))
        for layer in range(layers):
            q = torch.randn((1, H, G, D), generator=gen, device="cuda").to(torch.float16)
            a, b = conn.attend(layer, [1], q, D ** -0.5), twin.attend(layer, [1], q, D ** -0.5)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all()), layer
        if verbose:
            print(f"paged cache kscale example ok: {n_prompt} positions in chunks of {seam} and {n_prompt - seam} x {layers} layers stored "
                  f"from and loaded into paged blocks with one launch per call, K pre-scale up to {float(scale.max()):g} ({scheme})")
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="int4", choices=["fp8", "int4", "mxfp4"])
    run(ap.parse_args().scheme)
