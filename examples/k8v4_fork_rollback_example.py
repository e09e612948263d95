#!/usr/bin/env python3
"""Parallel samples on the split pool: `SpeckvSplitKVConnector.fork`, `commit(nodes=path)` and `truncate`.

A toy loop on an MI355X.  Random K / V rows stand in for a model and its drafter.
  1. one prompt goes in through `write_prefill` (FP8_E4M3 keys in one allocation, MXFP4 values in another);
  2. `fork` starts three samples from it: ONE `speckv_ext_copy_runs_kv` launch copies the stored records of both allocations, the odd last
     position is cloned -- nothing is prefilled again;
  3. every sample verifies a draft TREE (`attend_chunk(parents=...)`), picks its own accepted path and stores it with
     `commit(nodes=path, parents=...)`: the two `speckv_ext_write_pairs` calls read the path's rows where they lie;
  4. the samples are rolled back with `truncate` (ONE `speckv_ext_read_pairs_kv` launch brings the new odd last positions back as tails),
     and a fourth sample is forked from the first few positions of one of them (`fork(lengths=...)`);
  5. a continued chain step on all four, `commit(n_accept)`.

Checked in the example itself: every layer of every step against an fp32 torch softmax attention over what the requests hold -- `kv_rows`
(the stored rows as the records decode, the tail behind them) and the step's new rows.  `attend_chunk` takes the query in fp16, as the
reference does; `kv_rows` hands the FP8 keys over rounded to fp16 (2^-11 relative), so the bound is (2e-3 + 2 * 2^-11 * max sum |q||k| sm)
sum p|v| + 1e-6.  The prompt is untouched by everything its forks do, and that is checked too.

    python examples/k8v4_fork_rollback_example.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TREE = [-1, 0, 0, 1, 1, 2]                       # node 0, two children, three grandchildren
PATHS = [[0, 1, 3], [0, 2, 5], [0, 1]]           # the accepted path per sample (pretended)


def run(prompt=37, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_split_connector import SpeckvSplitKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, R = 8, 128, 128, 4
        assert prompt & 1 and 3 <= prompt <= T - 8, "the walk below is written for an odd prompt (a tail to clone) that leaves room for the steps"
        conn = SpeckvSplitKVConnector(lib, layers, H, D, T)
        gen = torch.Generator(device="cuda"); gen.manual_seed(47)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        sm = 1.0 / np.sqrt(D)
        checks, keep = 0, []

        def held(rid, layer):
            """everything a request holds of a layer, fp32 [positions][heads][dim] per kind: the records as they decode, then the tail"""
            return conn.kv_rows(rid, layer, 0).float(), conn.kv_rows(rid, layer, 1).float()

        def step(rids, S, parents):
            """one draft step on `rids`, every layer held to the fp32 reference -> (k_new, v_new, worst error / bound)"""
            nonlocal checks
            B = len(rids)
            q, k_new, v_new = rnd(layers, B, S, H, R, D), rnd(B, S, layers, H, D), rnd(B, S, layers, H, D)
            tree = parents if parents is not None else list(range(-1, S - 1))
            sees = torch.zeros((S, S), dtype=torch.bool, device="cuda")                  # node j sees its ancestors and itself
            for j in range(S):
                up = j
                while up >= 0:
                    sees[j, up] = True
                    up = tree[up]
            worst = 0.0
            for layer in range(layers):
                got = conn.attend_chunk(layer, rids, q[layer], k_new, v_new, sm, parents=parents)
                for b, rid in enumerate(rids):
                    k_old, v_old = held(rid, layer)
                    n = k_old.shape[0]
                    assert n == conn.length(rid)
                    kk, vv = torch.cat([k_old, k_new[b, :, layer].float()]), torch.cat([v_old, v_new[b, :, layer].float()])
                    qf = q[layer, b].float()                                             # [S][heads][R][dim]
                    s = torch.einsum("jhrd,thd->jhrt", qf, kk) * sm
                    reach = float((torch.einsum("jhrd,thd->jhrt", qf.abs(), kk.abs()) * sm).max())
                    mask = torch.cat([torch.ones((S, n), dtype=torch.bool, device="cuda"), sees], dim=1)[:, None, None, :]
                    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
                    want, mag = torch.einsum("jhrt,thd->jhrd", p, vv), torch.einsum("jhrt,thd->jhrd", p, vv.abs())
                    tol = (2e-3 + 2 * 2.0 ** -11 * reach) * mag + 1e-6
                    worst = max(worst, float(((got[b] - want).abs() / tol).max()))
                    checks += 1
            assert worst <= 1.0, worst
            return k_new, v_new, worst

        # 1. the prompt
        conn.add_request(1)
        keep += conn.write_prefill(1, rnd(layers, prompt, H, D), rnd(layers, prompt, H, D))
        prompt_rows = [[x.clone() for x in held(1, layer)] for layer in range(layers)]
        # 2. three samples of it
        samples = [11, 12, 13]
        keep += conn.fork([1] * len(samples), samples)
        for rid in samples:
            for layer in range(layers):
                assert all(torch.equal(a, b) for a, b in zip(held(rid, layer), prompt_rows[layer]))     # the prompt's bits, tail included
        # 3. a draft tree, an accepted path each
        k_new, v_new, worst_tree = step(samples, len(TREE), TREE)
        keep += conn.commit(samples, k_new, v_new, nodes=PATHS, parents=TREE)
        lengths = [prompt + len(p) for p in PATHS]
        assert [conn.length(r) for r in samples] == lengths
        # 4. roll back: one sample by one position, one by its whole path, one not at all; and a fourth sample from the middle of the first
        cut = [lengths[0] - 1, prompt, lengths[2]]
        conn.truncate(samples, cut)
        keep += conn.fork([samples[0]], [14], [prompt - 2])
        samples, cut = samples + [14], cut + [prompt - 2]
        assert [conn.length(r) for r in samples] == cut
        for layer in range(layers):
            # cut back to the prompt's length: its stored pairs again, bit for bit; the odd last position was committed into a page with a
            # draft and has come back through FP8 / MXFP4 once -- close to the prompt's fp16 row, not equal to it
            assert all(torch.equal(a[:prompt - 1], b[:prompt - 1]) for a, b in zip(held(12, layer), prompt_rows[layer]))
            assert all(0 < float((a[prompt - 1] - b[prompt - 1]).abs().max()) < 1.0 for a, b in zip(held(12, layer), prompt_rows[layer]))
            assert all(torch.equal(a, b[:prompt - 2]) for a, b in zip(held(14, layer), prompt_rows[layer]))
        # 5. go on: a chain of two drafts on all four
        k_new, v_new, worst_chain = step(samples, 2, None)
        accept = [2, 1, 2, 1]
        keep += conn.commit(samples, k_new, v_new, accept)
        assert [conn.length(r) for r in samples] == [n + a for n, a in zip(cut, accept)]
        _, _, worst_after = step(samples, 1, None)
        for layer in range(layers):                                                      # the source saw none of it
            assert all(torch.equal(a, b) for a, b in zip(held(1, layer), prompt_rows[layer]))
        torch.cuda.synchronize()
        if verbose:
            print(f"lengths {[conn.length(r) for r in samples]}; worst error / bound: tree step {worst_tree:.3f}, chain step after the rollback "
                  f"{worst_chain:.3f}, step after its commit {worst_after:.3f}")
            print(f"ok: {checks} layer checks over a fork, a path commit, a rollback and a second fork")
        return checks
    finally:
        lib.finalize()


if __name__ == "__main__":
    run()
