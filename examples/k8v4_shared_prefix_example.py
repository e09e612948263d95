#!/usr/bin/env python3
"""A system prompt held ONCE in the split pool: `SpeckvSplitKVConnector.attend_shared` / `attend_chunk_shared`.

A toy loop on an MI355X.  Random K / V rows stand in for a model.  The system prompt is one ordinary request of the split pool (FP8
keys, MXFP4 values).  Eight members hold only what is their own: each takes a suffix of a different length through
`attend_chunk_shared` + `commit`, then a few decode steps run `attend_shared` + `commit`.  Per layer and step that is the members' own
`attend` (one `speckv_ext_attend_kv_batch`, one tail fold while some member has an odd length) and ONE
`speckv_ext_attend_prefix_fold_kv` launch that reads the prompt's records once per 64 query rows and folds them in.

Beside every member stands a TWIN that holds a full copy -- prompt + suffix in one request -- and decodes through `attend`: the only
route before this one.  Checked in the example itself, at every step and layer: both routes against a float64 softmax over the rows
as the records give them back (`speckv_ext_fetch_range`), within the project's bound for the kernels with an 8-bit query,
(2e-3 + 2 delta) sum p|v| + 1e-6; and the two routes against each other.  They differ where the query enters -- the twin quantises it
to E4M3 over the prompt too, the shared route keeps it fp16 there -- so they agree as two quantisations of one step do, not bit for
bit: their relative L2 distance stays far below the 0.25 the project asks of the pool's decode-regime error (kv_accuracy).

Pool bytes, as arithmetic: a copy of the prompt costs prompt / 2 pairs x 3136 B per layer and member; the shared route stores it once,
(members - 1) x prompt / 2 x 3136 B per layer less.

    python examples/k8v4_shared_prefix_example.py [--prompt 1024] [--members 8] [--steps 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(prompt=1024, members=8, steps=4, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_accuracy import quantize_query_e4m3
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    assert prompt % 2 == 0, "only whole stored pairs can be shared"
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, G = 8, 128, 4
        suffix = [1 + (5 * m) % 12 for m in range(members)]
        T = (prompt + max(suffix) + steps + 31) // 32 * 32
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(31)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        sm = 1.0 / np.sqrt(D)
        P, rids, twins = 1000, list(range(members)), [100 + m for m in range(members)]
        pk, pv = rnd(layers, prompt, H, D), rnd(layers, prompt, H, D)
        conn.add_request(P)
        keep = conn.write_prefill(P, pk, pv)
        # the suffixes: one chunk step over the shared prompt, then commit into the MEMBER; the twin takes prompt + suffix as a prompt
        S = max(suffix)
        k_suf, v_suf = rnd(members, S, layers, H, D), rnd(members, S, layers, H, D)
        for rid in rids:
            conn.add_request(rid)
        for layer in range(layers):
            out = conn.attend_chunk_shared(layer, rids, [P] * members, rnd(members, S, H, G, D), k_suf, v_suf, sm, n_new=suffix)
            assert bool(torch.isfinite(out).all())
        keep += conn.commit(rids, k_suf, v_suf, suffix)
        rows = {}
        for m, (rid, twin) in enumerate(zip(rids, twins)):
            own = [k_suf[m, :suffix[m]].permute(1, 0, 2, 3).contiguous(), v_suf[m, :suffix[m]].permute(1, 0, 2, 3).contiguous()]
            conn.add_request(twin)
            keep += conn.write_prefill(twin, torch.cat([pk, own[0]], dim=1), torch.cat([pv, own[1]], dim=1))
            rows[rid] = [own[0].cpu().numpy(), own[1].cpu().numpy()]        # [layers][positions][heads][dim]: what the member holds

        def stored(handle, layer, n):
            """the first n (even) positions of a layer as the allocation's records decode: float64 [n][heads][dim]"""
            out = torch.empty((max(n // 2, 1), 2 * H * D), dtype=torch.float16, device="cuda")
            if n:
                lib.fetch_range(handle, layer * (T // 2), n // 2, out.data_ptr(), False, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return out.cpu().numpy().astype(np.float64).reshape(-1, H, D)[:n]

        def softmax(parts):
            """parts: [(scores [H][G][n], V [n][H][D])] -> (out [H][G][D], sum p|v|)"""
            s, vv = np.concatenate([p[0] for p in parts], axis=-1), np.concatenate([p[1] for p in parts])
            p = np.exp(s - s.max(-1, keepdims=True))
            p /= p.sum(-1, keepdims=True)
            return np.einsum("hgt,thd->hgd", p, vv), np.einsum("hgt,thd->hgd", p, np.abs(vv))

        def reference(layer, q16, req, n_fp16_prefix, tail):
            """float64 over what request `req` holds (its stored part under the E4M3 query), behind n_fp16_prefix positions of the prompt
            request under the fp16 query, in front of the fp16 tail (k [H][D], v [H][D]) or None -> (want, tol)"""
            qf, qe = q16.astype(np.float64), quantize_query_e4m3(q16)
            r, even = conn.requests[req], conn.length(req) & ~1
            parts, reach = [], np.zeros(H)
            if n_fp16_prefix:
                p = conn.requests[P]
                parts.append((np.einsum("hgd,thd->hgt", qf, stored(p.k_handle, layer, n_fp16_prefix)) * sm, stored(p.v_handle, layer, n_fp16_prefix)))
            if even:
                kk = stored(r.k_handle, layer, even)
                parts.append((np.einsum("hgd,thd->hgt", qe, kk) * sm, stored(r.v_handle, layer, even)))
                reach = np.einsum("hgd,thd->hgt", np.abs(qe), np.abs(kk)).max(axis=(1, 2)) * sm
            if tail is not None:
                parts.append(((np.einsum("hgd,hd->hg", qf, tail[0].astype(np.float64)) * sm)[..., None], tail[1].astype(np.float64)[None]))
            want, mag = softmax(parts)
            return want, (2e-3 + 2 * 3e-5 * reach)[:, None, None] * mag + 1e-6

        checked = 0
        for step in range(steps):
            worst = apart = 0.0
            for layer in range(layers):
                q = rnd(members, H, G, D)
                shared = conn.attend_shared(layer, rids, [P] * members, q, sm).cpu().numpy()
                copies = conn.attend(layer, twins, q, sm).cpu().numpy()
                for m, (rid, twin) in enumerate(zip(rids, twins)):
                    q16, n = q[m].cpu().numpy(), conn.length(rid)
                    tail = (rows[rid][0][layer, n - 1], rows[rid][1][layer, n - 1]) if n & 1 else None
                    want_s, tol_s = reference(layer, q16, rid, prompt, tail)
                    want_c, tol_c = reference(layer, q16, twin, 0, tail)
                    worst = max(worst, float((np.abs(shared[m] - want_s) / tol_s).max()), float((np.abs(copies[m] - want_c) / tol_c).max()))
                    # the two routes against each other: one step under two roundings of the query over the prompt
                    apart = max(apart, float(np.linalg.norm(shared[m] - copies[m]) / np.linalg.norm(copies[m])))
                    checked += layer == 0
            assert worst <= 1.0 and apart <= 0.25, (step, worst, apart)
            k_new, v_new = rnd(members, 1, layers, H, D), rnd(members, 1, layers, H, D)
            keep += conn.commit(rids, k_new, v_new, [1] * members)
            keep += conn.commit(twins, k_new, v_new, [1] * members)
            for m, rid in enumerate(rids):
                rows[rid][0] = np.concatenate([rows[rid][0], k_new[m].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
                rows[rid][1] = np.concatenate([rows[rid][1], v_new[m].permute(1, 0, 2, 3).cpu().numpy()], axis=1)
            if verbose:
                print(f"decode step {step}: members hold {[conn.length(r) for r in rids]} behind a prompt of {prompt}; worst err / tol {worst:.3f}, "
                      f"shared against copies rel. L2 {apart:.4f}")
        torch.cuda.synchronize()
        assert [conn.length(r) for r in rids] == [s + steps for s in suffix] and conn.length(P) == prompt
        if verbose:
            saved = (members - 1) * (prompt // 2) * 3136
            print(f"ok: {steps} decode steps over {members} members; the prompt is stored once: {saved} bytes per layer less than {members} copies "
                  f"(arithmetic: (members - 1) x prompt pairs x 3136 B)")
        return checked
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    run(prompt=a.prompt, members=a.members, steps=a.steps)
