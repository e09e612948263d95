#!/usr/bin/env python3
"""The split pool ("K8V4": FP8 keys, MXFP4 values) behind bf16 paged caches: out of the pool, through the blocks, into a second request.

A toy on an MI355X.  Request A gets a prompt of 37 positions by `write_prefill`.  `load_paged` decodes all of it into bf16 blocks
([2, blocks, block_size, 8, 128]: vLLM's layout) with ONE launch (`speckv_ext_read_slots_kv`): the K plane from A's FP8_E4M3
allocation, the V plane from its MXFP4 allocation, the odd last position from the fp16 tail as a held row.  `store_paged` then builds
request B from those blocks in two calls of 19 and 18 positions -- ONE launch each (`speckv_ext_write_slots_kv`), the seam inside a
position pair: the first call's last position comes back as a held fp16 row, the second call's launch pairs it with its first cache
row, and the new odd last position becomes B's tail.  `attend` on A and on B then gives the same bits, with and without a window.

The prompt is made of values both formats hold exactly (K: four significant bits under a power-of-two page scale, V: bf16 values),
so that the walk through bf16 blocks changes nothing and "the same" can mean bit for bit.  On arbitrary rows a bf16 cache rounds
each decoded K value once (include/speckv_ext.h), and B's records are those of the rounded rows.

    python examples/k8v4_paged_cache_example.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, BS, NB = 8, 128, 256, 16, 32
        n, seam = 37, 19
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        # K: per position pair (an FP8 page) E4M3-exact values q, one of them 448, times a power of two
        host = torch.Generator().manual_seed(23)
        q = (torch.randn((layers, (n + 1) // 2, 2 * H * D), generator=host) * 100.0).clamp(-448.0, 448.0)
        m, e = torch.frexp(q)
        q = torch.ldexp(torch.round(m * 16.0) / 16.0, e)
        q[q.abs() < 1.0] = 0.0
        q[:, :, 0] = 448.0
        scale = torch.exp2(torch.randint(-8, -5, (layers, (n + 1) // 2, 1), generator=host).float())
        k = (q * scale).view(layers, n + 1, H, D)[:, :n].to(torch.float16).contiguous().cuda()
        v = torch.randn((layers, n, H, D), generator=gen, device="cuda").to(torch.bfloat16).to(torch.float16).contiguous()
        conn.add_request("A")
        conn.add_request("B")
        keep = conn.write_prefill("A", k, v)

        caches = [torch.zeros((2, NB, BS, H, D), dtype=torch.bfloat16, device="cuda") for _ in range(layers)]
        blocks = torch.randperm(NB, generator=torch.Generator().manual_seed(23)).tolist()
        slots = [blocks[t // BS] * BS + t % BS for t in range(n)]                    # vLLM's rule: block * block_size + offset
        mapping = torch.tensor(slots, dtype=torch.int64, device="cuda")
        conn.load_paged(["A"], [0], [n], mapping, caches)                            # ONE launch: both allocations, every layer, the tail
        torch.cuda.synchronize()
        for layer, cache in enumerate(caches):
            got = cache.view(2, NB * BS, H, D)[:, mapping]
            for kind in (0, 1):
                want = conn.kv_rows("A", layer, kind).to(torch.bfloat16)
                assert torch.equal(got[kind].view(torch.int16), want.view(torch.int16)), (layer, kind)
        for lo, hi in ((0, seam), (seam, n)):                                        # ONE launch per call; the seam falls inside a pair
            part = torch.tensor(slots[lo:hi], dtype=torch.int64, device="cuda")
            keep += conn.store_paged(["B"], [hi - lo], part, caches)
            keep.append(part)
        torch.cuda.synchronize()
        assert conn.length("B") == conn.length("A") == n
        sm = 1.0 / D ** 0.5
        worst = 0.0
        for window in (None, 16):
            for layer in range(layers):
                query = torch.randn((1, H, 4, D), generator=gen, device="cuda").to(torch.float16)
                a = conn.attend(layer, ["A"], query, sm, window=window)
                b = conn.attend(layer, ["B"], query, sm, window=window)
                torch.cuda.synchronize()
                worst = max(worst, float((a - b).abs().max()))
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (window, layer)
                assert bool(torch.isfinite(a).all()) and bool(a.any())
        if verbose:
            print(f"k8v4 paged cache example ok: {n} positions x {layers} layers out of the split pool into bf16 blocks with one launch, back "
                  f"into a second request in calls of {seam} and {n - seam} positions with one launch each; attend on both requests, with and "
                  f"without a window: the outputs are equal (largest difference {worst})")
    finally:
        lib.finalize()


if __name__ == "__main__":
    run()
