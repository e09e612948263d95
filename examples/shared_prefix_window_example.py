#!/usr/bin/env python3
"""One system prompt in front of N users on a model that INTERLEAVES local and global layers, without copies of the prompt.

A toy loop on an MI355X.  One request holds the system prompt (random K / V rows stand in for a model); the N users are ordinary
requests that hold only their own positions.  Such a user holds nothing of the prompt on ANY layer, so every layer goes through the
shared route: the even layers are sliding-window layers (`attend_shared(window=W)`: the query sees the last W positions of prompt +
own, the fold walks only the prompt's tiles inside the window), the odd ones global (`attend_shared`).  After the decode steps comes
one speculative step: a draft tree per user, `attend_tree_shared` on every layer (by depth under the window on the local ones), and
`commit(nodes=accepted path)`.

Every user is compared with a forked twin that holds a copy of the prompt (`fork` + the same tokens + `attend(window=W)` /
`attend_tree(window=W)`).  The two routes are two roundings of the same softmax -- the twin's decode kernel may quantise the query for
the prompt's positions too -- so they agree within a tolerance that follows the pool format, not bit for bit.

    python examples/shared_prefix_window_example.py [--scheme int4] [--prompt 98] [--users 8] [--steps 6] [--window 40]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# largest |difference| of the two routes' outputs over the largest |output| (examples/shared_prefix_example.py)
AGREE = {"int4": 2e-2, "fp8": 0.15, "mxfp4": 0.15}
TREE = [-1, 0, 1, 1, 0, 4, 5, -1, 7]                            # two branches under node 0, a second root
PATH = [0, 4, 5, 6]                                             # the accepted root-to-node path


def run(scheme="int4", prompt=98, users=8, steps=6, window=40, layers=2, verbose=True):
    import torch
    import cxl_speckv_amd as pkg
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector

    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        H, D, T, G = 8, 128, 512, 4
        conn = SpeckvKVConnector(lib, layers, H, D, T, scheme)
        gen = torch.Generator(device="cuda"); gen.manual_seed(23)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        local = lambda layer: window if layer % 2 == 0 else None           # alternating local / global layers
        k, v = rnd(layers, prompt, H, D), rnd(layers, prompt, H, D)
        root, members, twins = 1, list(range(100, 100 + users)), list(range(200, 200 + users))
        conn.add_request(root)
        keep = conn.write_prefill(root, k, v)
        for rid in members:                                     # a user holds nothing yet: no copy of the prompt on any layer
            conn.add_request(rid)
        keep += conn.fork([root] * users, twins)                # the route this one replaces: the prompt once per user
        shared = prompt & ~1                                    # whole stored pairs can be shared ...
        if prompt & 1:                                          # ... an odd last position goes into every user as its first own one
            keep += conn.append(members, k[:, -1][None].expand(users, -1, -1, -1).contiguous(), v[:, -1][None].expand(users, -1, -1, -1).contiguous())
        sm, checked = 1.0 / np.sqrt(D), 0
        pids, plens = [root] * users, [shared] * users

        def agree(x, y, what):
            assert bool(torch.isfinite(x).all())
            diff = float((x - y).abs().max() / y.abs().max())
            assert diff <= AGREE[scheme], (what, diff)
            return diff

        for step in range(steps):
            k_new, v_new = rnd(users, layers, H, D), rnd(users, layers, H, D)          # every user appends a token of its own ...
            keep += conn.append(members, k_new, v_new)
            keep += conn.append(twins, k_new, v_new)
            q = rnd(users, H, G, D)                                                    # ... and attends from it
            for layer in range(layers):
                x = conn.attend_shared(layer, members, pids, q, sm, prefix_lens=plens, window=local(layer))
                y = conn.attend(layer, twins, q, sm, window=local(layer))
                diff = agree(x, y, (step, layer))
            checked += users
            if verbose:
                print(f"step {step}: users hold {conn.length(members[0])} positions of their own, twins {conn.length(twins[0])}; "
                      f"largest relative difference of the last layer {diff:.4f}")
        # the speculative step: a draft tree per user on every layer, then the accepted path
        S = len(TREE)
        q, k_new, v_new = rnd(users, S, H, G, D), rnd(users, S, layers, H, D), rnd(users, S, layers, H, D)
        for layer in range(layers):
            x = conn.attend_tree_shared(layer, members, pids, q, k_new, v_new, sm, TREE, prefix_lens=plens, window=local(layer))
            y = conn.attend_tree(layer, twins, q, k_new, v_new, sm, TREE, window=local(layer))
            diff = agree(x, y, ("tree", layer))
        keep += conn.commit(members, k_new, v_new, [PATH] * users)
        keep += conn.commit(twins, k_new, v_new, [PATH] * users)
        checked += users
        for m, t in zip(members, twins):
            assert conn.length(m) + shared == conn.length(t)
            assert (conn.requests[m].tail_k is None) == (conn.requests[t].tail_k is None)
        torch.cuda.synchronize()
        assert conn.length(root) == prompt
        if verbose:
            print(f"tree step: {S} nodes per user, {len(PATH)} accepted; largest relative difference of the last layer {diff:.4f}")
            print(f"ok: {users} users behind one stored prompt of {prompt} positions, window {window} on the even layers, "
                  f"each within {AGREE[scheme]} of its forked twin")
        return checked
    finally:
        lib.finalize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", default="int4", choices=["fp8", "int4", "mxfp4"])
    ap.add_argument("--prompt", type=int, default=98)
    ap.add_argument("--users", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--window", type=int, default=40)
    a = ap.parse_args()
    run(a.scheme, a.prompt, a.users, a.steps, a.window)
