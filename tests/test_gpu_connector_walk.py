"""-m gpu: SpeckvKVConnector over its LIFETIME -- the seeded walks of tests/_connector_shadow.py mix every operation of the connector on
one instance (8 kv heads x 128, L = 2, T = 256, at most 6 live requests) and hold it to the float64 shadow model after every step.

After every mutating operation: the lengths of all live requests, `tail_k is None` exactly for the even ones, kv_rows of every request
the operation named and of one it did not (a fork's source or a source's fork first) BIT FOR BIT the shadow's rows, both layers, K and
V, and `_epoch` moved.  Every read operation meets float64 over the shadow with the reference and the bound of its route's own file,
imported from there: attend / attend_layers / attend(window=) by HeadChecker.check_rows (tests/test_gpu_decode_window.py), attend_spec
as a chain and as a tree by HeadChecker.want + chained_folds with the bound of tests/test_gpu_rollback.py, attend_chunk (causal,
window=) by tests/test_gpu_chunk_window.py::_check, attend_chunk(parents=) and attend_tree(window=) by
tests/test_gpu_chunk_tree_window.py::_check, attend_shared and attend_chunk_shared by _decode_ref / _assert_decode / _chunk_ref of
tests/test_gpu_shared_prefix.py.  No tolerance of its own.

What the walks are for: a step cache (plan, fold rows, mask words, held-row indices, shared-prefix arguments) that outlives a mutation,
a tail that is a view of a tensor somebody else changes, a row that goes through the pool format twice, a record behind a cut that is
seen again.  tests/test_connector_walk_cpu.py asserts that the committed seeds reach those cases.

A failure names the walk, its seed, the step, the operation and the operations so far; replay(ops, **walk) runs such a list (cut it
down by hand).  The walk issues valid calls only and stops at its first failed assertion."""
import time
import types

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests import test_gpu_shared_prefix as shared
from tests._connector_shadow import L, T, WALKS, Shadow, ancestors, is_read, k_scales, named, queries, rows_of, walk
from tests._gpu import D, H, HeadChecker, torch_mod
from tests.test_gpu_chunk_tree_window import _check as _check_tree
from tests.test_gpu_chunk_window import _check as _check_chain
from tests.test_gpu_round2 import open_lib
from tests.test_gpu_spec_step import SCHEMES, _region, chained_folds

pytestmark = pytest.mark.gpu
SM = 1.0 / np.sqrt(D)
NO_WINDOW = 4 * T                                  # a window of tests/test_gpu_chunk_window.py::_check that cuts nothing


class _Run:
    """one connector, its shadow, and the checks"""

    def __init__(self, torch, oracle, lib, w, wrong_shadow=False):
        self.torch, self.oracle, self.w, self.scheme = torch, oracle, w, w["scheme"]
        kscale = k_scales(w["seed"]) if w["prescale"] else None
        self.conn = SpeckvKVConnector(lib, L, H, D, T, self.scheme)
        if kscale is not None:
            self.conn.set_k_channel_scale(torch.from_numpy(kscale).cuda())
        self.sh = Shadow(oracle, self.scheme, kscale, as_given_on_read_back=wrong_shadow)
        self.R = w["rpp"]
        self.worst, self.kin, self.checkers, self.step = {}, {}, {}, 0

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def host(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()

    def note(self, route, x):
        self.worst[route] = max(self.worst.get(route, 0.0), float(x))

    def checker(self, rid, layer):
        """float64 K / V of what request rid has stored at `layer`: the oracle's records of the shadow's page images"""
        key = (rid, layer, self.sh.req[rid].version)
        if key not in self.checkers:
            if len(self.checkers) >= 32:
                self.checkers.clear()
            self.checkers[key] = HeadChecker(self.oracle, SCHEMES[self.scheme], _region(*self.sh.region(rid, layer), T), T)
        return self.checkers[key]

    # ------------------------------------------------------------------------- mutating operations
    def mutate(self, op):
        conn, sh, torch, kind = self.conn, self.sh, self.torch, op["op"]
        epoch = conn._epoch
        keep = None
        if kind in ("prefill", "reuse"):
            if kind == "reuse":
                conn.free_request(op["rid"])
            conn.add_request(op["rid"])
            k, v = rows_of(op)
            keep = conn.write_prefill(op["rid"], self.dev(k[0].transpose(1, 0, 2, 3)), self.dev(v[0].transpose(1, 0, 2, 3)))
        elif kind == "free":
            conn.free_request(op["rid"])
        elif kind == "truncate":
            conn.truncate(op["ids"], op["new"])
        elif kind == "fork":
            keep = conn.fork(op["srcs"], op["news"], op["lengths"])
            for s, r in zip(op["srcs"], op["news"]):
                self.kin.setdefault(s, set()).add(r)
                self.kin.setdefault(r, set()).add(s)
        else:
            k, v = rows_of(op)
            if kind == "append":
                keep = conn.append(op["ids"], self.dev(k[:, 0]), self.dev(v[:, 0]))
            elif kind == "append_tokens":
                keep = conn.append_tokens(op["ids"], self.dev(k), self.dev(v), op["accept"])
            elif kind == "append_path":
                keep = conn.append_path(op["ids"], self.dev(k), self.dev(v), op["paths"], parents=op["parents"])
            else:
                keep = conn.commit(op["ids"], self.dev(k), self.dev(v), op["nodes"], parents=op["parents"])
        torch.cuda.synchronize()
        del keep
        sh.apply(op)
        if kind in ("free", "reuse"):
            for other in self.kin.pop(op["rid"], ()):
                self.kin[other].discard(op["rid"])
        lens = sh.lengths()
        assert sorted(conn.requests) == sorted(lens), ("live requests", sorted(conn.requests), sorted(lens))
        for rid, n in lens.items():
            assert conn.length(rid) == n, ("length", rid, conn.length(rid), n)
            assert (conn.requests[rid].tail_k is None) == (conn.requests[rid].tail_v is None) == (n % 2 == 0), ("tail", rid, n)
        assert conn._epoch != epoch, "_epoch did not move"
        look = [r for r in dict.fromkeys(named(op)) if r in lens]
        others = [r for r in sorted(lens) if r not in look]
        if others:
            related = [r for r in others if any(r in self.kin.get(x, ()) for x in look)]
            look.append(related[0] if related else others[self.step % len(others)])
        for rid in look:
            for layer in range(L):
                for k_or_v in (0, 1):
                    got = self.host(conn.kv_rows(rid, layer, k_or_v))
                    want, ok = sh.rows(rid, layer, k_or_v)
                    assert got.shape == want.shape, ("kv_rows shape", rid, got.shape, want.shape)
                    bad = (got.view(np.uint16) != want.view(np.uint16)) & ok
                    assert not bad.any(), ("kv_rows", "request", rid, "layer", layer, "kind", k_or_v, "length", lens[rid], int(bad.sum()),
                                           "first [pos, head, dim]", [int(x) for x in np.argwhere(bad)[0]],
                                           "named" if rid in named(op) else "not named")

    # ------------------------------------------------------------------------- read operations
    def read(self, op):
        conn, sh, kind = self.conn, self.sh, op["op"]
        epoch, lens = conn._epoch, sh.lengths()
        getattr(self, "_" + {"attend_layers": "attend", "attend_window": "attend", "spec_chain": "spec", "spec_tree": "spec",
                             "chunk_window": "chunk", "chunk_parents": "tree", "tree_window": "tree"}.get(kind, kind))(op)
        assert conn._epoch == epoch and {r: conn.length(r) for r in lens} == lens, "a read changed the state"

    def _attend(self, op):
        ids, layer, W, R = op["ids"], op["layer"], op.get("W"), self.R
        if op["op"] == "attend_layers":
            q = queries(op["seed"], L, len(ids), H, R, D)
            got = self.host(self.conn.attend_layers(0, L, ids, self.dev(q), SM))
            layers = list(range(L))
        else:
            q = queries(op["seed"], 1, len(ids), H, R, D)
            got = self.host(self.conn.attend(layer, ids, self.dev(q[0]), SM, window=W))[None]
            layers = [layer]
        assert np.isfinite(got).all(), "not finite"
        for at, layer in enumerate(layers):
            qk, w = self.sh.query(q[at], layer), []
            for b, rid in enumerate(ids):
                n = self.sh.length(rid)
                even, lo = n & ~1, 0
                if W:
                    begin, skip, _ = SpeckvKVConnector.decode_window_range(n, W)
                    lo = begin + skip
                chk, tail = self.checker(rid, layer), self.sh.tail(rid)
                for head in range(H):
                    tl = None if tail is None else (tail[0][layer, head][None], tail[1][layer, head][None])
                    chk.check_rows(got[at, b, head][None], None, qk[b, head][None], head, [max(0, even - lo)], SM,
                                   (op["op"], "request", rid, "length", n, "layer", layer, "head", head), tl, pos_begin=lo, worst=w)
            self.note(op["op"], max(w))

    def _spec(self, op):
        """the reference and the bound of tests/test_gpu_rollback.py::test_stale_records_behind_the_cut_are_never_seen"""
        ids, layer, S, R, parents, n_new = op["ids"], op["layer"], op["S"], self.R, op.get("parents"), op.get("n_new")
        q = queries(op["seed"], len(ids), S, H, R, D)
        k_new, v_new = rows_of(op)
        got = self.host(self.conn.attend_spec(layer, ids, self.dev(q), self.dev(k_new), self.dev(v_new), SM, n_new=n_new, parents=parents))
        assert np.isfinite(got).all(), "not finite"
        qk, ks, worst = self.sh.query(q, layer), self.sh.stored_k(k_new), 0.0
        for b, rid in enumerate(ids):
            n = self.sh.length(rid)
            even, chk, tail = n & ~1, self.checker(rid, layer), self.sh.tail(rid)
            for head in range(H):
                q_head = qk[b, :, head].reshape(S * R, D)
                w_out, w_lse, w_mag, delta = chk.want(q_head, head, even, SM)
                for j in range(S if n_new is None else n_new[b]):
                    r = slice(j * R, (j + 1) * R)
                    sees = list(range(j + 1)) if parents is None else ancestors(parents, j)
                    kh = np.stack(([tail[0][layer, head]] if n & 1 else []) + [ks[b, t, layer, head] for t in sees])
                    vh = np.stack(([tail[1][layer, head]] if n & 1 else []) + [v_new[b, t, layer, head] for t in sees])
                    want, _, mag = chained_folds((w_out[r], w_mag[r]), w_lse[r], q_head[r], kh, vh, SM)
                    err = np.abs(got[b, j, head] - want)
                    tol = (2e-3 + 2 * delta) * mag + 1e-6 + len(kh) * (2e-5 * np.abs(want) + 2e-6)
                    worst = max(worst, float((err / tol).max()))
                    assert np.all(err <= tol), (op["op"], "request", rid, "length", n, "head", head, "position", j, float((err / tol).max()), delta)
        self.note(op["op"], worst)

    def _held_view(self, ids):
        """what the chunk files' checks read of a connector and its prompts, from the shadow"""
        reqs, prompts = {}, {}
        for rid in ids:
            n, tail = self.sh.length(rid), self.sh.tail(rid)
            as_tensor = lambda x: None if x is None else self.torch.from_numpy(x)
            reqs[rid] = types.SimpleNamespace(length=n, tail_k=as_tensor(tail and tail[0]), tail_v=as_tensor(tail and tail[1]))
            prompts[rid] = (np.zeros((1, n, 1, 1), np.float16),) * 2
        return types.SimpleNamespace(requests=reqs), prompts

    def _step_inputs(self, op):
        q = queries(op["seed"], len(op["ids"]), op["S"], H, self.R, D)
        k_new, v_new = rows_of(op)
        return q, k_new, v_new, self.sh.query(q, op["layer"]), (self.sh.stored_k(k_new), v_new)

    def _chunk(self, op):
        ids, layer, S, W = op["ids"], op["layer"], op["S"], op.get("W")
        q, k_new, v_new, qk, new = self._step_inputs(op)
        got = self.host(self.conn.attend_chunk(layer, ids, self.dev(q), self.dev(k_new), self.dev(v_new), SM, n_new=op["n_new"], splits=op["splits"],
                                               window=W))
        view, prompts = self._held_view(ids)
        live = op["n_new"] or [S] * len(ids)
        for b, rid in enumerate(ids):
            assert not got[b, live[b]:].any(), ("a row of a position that is not live is not zero", rid)
            if live[b]:
                chk = self.checker(rid, layer)
                worst = _check_chain(lambda k, v, head: chk.kv(head), view, b, rid, prompts[rid], qk, new, live[b], [(W or NO_WINDOW, got, None)],
                                     (op["op"], "request", rid, "length", self.sh.length(rid)), layer=layer)
                self.note(op["op"], max(worst.values()))

    def _tree(self, op):
        ids, layer, S, W, parents = op["ids"], op["layer"], op["S"], op.get("W"), op["parents"]
        q, k_new, v_new, qk, new = self._step_inputs(op)
        if W:
            got = self.conn.attend_tree(layer, ids, self.dev(q), self.dev(k_new), self.dev(v_new), SM, parents, splits=op["splits"], window=W)
        else:
            got = self.conn.attend_chunk(layer, ids, self.dev(q), self.dev(k_new), self.dev(v_new), SM, parents=parents, splits=op["splits"])
        got = self.host(got)
        view, prompts = self._held_view(ids)
        for b, rid in enumerate(ids):
            chk = self.checker(rid, layer)
            worst = _check_tree(lambda k, v, head: chk.kv(head), view, b, rid, prompts[rid], qk, new, parents, S, [(W or 0, got, None)],
                                (op["op"], "request", rid, "length", self.sh.length(rid)), layer=layer)
            self.note(op["op"], max(worst.values()))

    def _members(self, op):
        prefix = self.sh.held(op["prefix"])
        lens = op["plens"] if op["plens"] is not None else [self.sh.length(op["prefix"])] * len(op["ids"])
        return [(prefix, n, self.sh.held(rid)) for rid, n in zip(op["ids"], lens)]

    def _shared(self, op):
        ids, layer = op["ids"], op["layer"]
        q = queries(op["seed"], len(ids), H, self.R, D)
        got = self.host(self.conn.attend_shared(layer, ids, [op["prefix"]] * len(ids), self.dev(q), SM, prefix_lens=op["plens"], splits=op["splits"]))
        ref = shared._decode_ref(self.oracle, self.scheme, layer, self.sh.query(q, layer), self._members(op))
        self.note(op["op"], shared._assert_decode(got, None, ref, f"step {self.step} attend_shared {ids} of {op['prefix']} lens {op['plens']}"))

    def _chunk_shared(self, op):
        ids, layer, S = op["ids"], op["layer"], op["S"]
        q, k_new, v_new, qk, new = self._step_inputs(op)
        got = self.host(self.conn.attend_chunk_shared(layer, ids, [op["prefix"]] * len(ids), self.dev(q), self.dev(k_new), self.dev(v_new), SM,
                                                      n_new=op["n_new"], prefix_lens=op["plens"], splits=op["splits"]))
        assert np.isfinite(got).all(), "not finite"
        live = op["n_new"] or [S] * len(ids)
        want, mag = shared._chunk_ref(self.oracle, self.scheme, layer, qk, new, live, self._members(op))
        for m, n in enumerate(live):
            err, tol = np.abs(got[m, :n] - want[m, :n]), 2e-3 * mag[m, :n] + 1e-6
            self.note(op["op"], float((err / tol).max(initial=0.0)))
            assert np.all(err <= tol), (op["op"], "request", ids[m], float((err / tol).max(initial=0.0)))
            assert not got[m, n:].any(), ("a row of a position that is not live is not zero", ids[m])


def replay(ops, oracle=None, wrong_shadow=False, **w):
    """Run a list of operations (tests/_connector_shadow.py: walk) on a connector of its own and hold every step to the shadow.
    w: the walk's profile (an entry of WALKS; the first one where nothing is given).  Returns the worst err / tol per route; an
    AssertionError names the step.  wrong_shadow: the shadow installs a read-back row as it was given -- the walk must fail then."""
    torch = torch_mod()
    w = dict(WALKS[0], **w)
    if oracle is None:
        from oracle.bindings import Oracle, build_oracle
        build_oracle()
        oracle = Oracle()
    lib = open_lib(SPECKV_POOL_DEVICES="0,0,0") if w["striped"] else pkg.SpeckvLib(pkg.library_path(), "hip:0")
    began = time.perf_counter()
    try:
        run = _Run(torch, oracle, lib, w, wrong_shadow)
        try:
            for i, op in enumerate(ops):
                run.step = i
                try:
                    (run.read if is_read(op) else run.mutate)(op)
                except AssertionError as e:
                    raise AssertionError(f"walk {w['name']} (seed {w['seed']}), step {i}: {op}\n{e}\noperations so far: {ops[:i + 1]}") from e
        finally:
            torch.cuda.synchronize()
            print(f"connector walk {w['name']} seed {w['seed']}: {run.step + 1} of {len(ops)} operations in {time.perf_counter() - began:.1f} s; "
                  "worst err / tol " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(run.worst.items())))
        return run.worst
    finally:
        shared._checkers.clear()
        lib.finalize()


@pytest.mark.parametrize("w", WALKS, ids=[w["name"] for w in WALKS])
def test_connector_walk_against_the_shadow(oracle, w):
    """one seeded walk per pool format and placement (fp8, int4, mxfp4 on one pool and on a pool striped over three; fp8 and int4 with
    a K pre-scale of powers of two in 2**-2 .. 2**2), each on a library instance of its own"""
    ops = walk(w["seed"], w["n_ops"], w)
    worst = replay(ops, oracle=oracle, **w)
    assert set(worst) >= {o["op"] for o in ops if is_read(o)}
    assert all(x <= 1.0 for x in worst.values()), worst


# What the first walks found.  Not a stale cache: the FP8 chunk routes themselves.  k_attend_chunk and k_attend_prefix staged the K rows
# of an FP8 pool as fp16(E4M3 value x block scale), a relative 2^-12 per element that the float64 reference (the records' values as
# they are) does not share; the score error it makes grows with |k|.  Measured on a fresh connector with no history, worst err / tol
# of attend_chunk and attend_chunk(parents=): 0.33 / 0.34 over rows of magnitude 1, 1.17 / 1.00 over rows of magnitude 3, 1.23 / 1.37
# over the walks' mix of 0.3, 1 and 3 -- the list below gave 1.37.  The kernels now stage the E4M3 values themselves (exact in fp16)
# and multiply the score by the block scale in fp32 (csrc/chunk_device.hpp: decode_pool, pool_k_scale): 0.26 - 0.34 in the walks.
PARENTS_20 = [-1, 0, 0, -1, 1, 1, 2, 4, 7, 8, 7, 8, 11, 12, 12, 11, 14, 13, 17, 16]
FP8_ROWS_OF_MAGNITUDE_3 = [
    dict(op="prefill", rid=4, n=98, seed=1003), dict(op="prefill", rid=5, n=37, seed=2003), dict(op="prefill", rid=6, n=5, seed=3003),
    dict(op="chunk_parents", layer=0, seed=30, ids=[4, 5], S=20, parents=PARENTS_20, splits=1),
    dict(op="chunk", layer=1, seed=31, ids=[4, 5], S=17, n_new=None, splits=1),
    dict(op="tree_window", layer=0, seed=32, ids=[4, 5], S=20, parents=PARENTS_20, splits=2, W=64),
    dict(op="shared", layer=0, seed=33, ids=[5, 6], prefix=4, plens=None, splits=1),
    dict(op="chunk_shared", layer=1, seed=34, ids=[5, 6], prefix=4, plens=[98, 64], S=17, n_new=None, splits=0),
]


def test_fp8_chunk_routes_hold_their_bound_over_rows_of_magnitude_3(oracle):
    """the shortest list that showed it (a prefill and one tree step), and the same rows through the other routes that stage an FP8
    prefix or pool for an fp16 query: the causal chunk, the tree under a window in pieces, and both shared-prefix folds"""
    worst = replay(FP8_ROWS_OF_MAGNITUDE_3, oracle=oracle, **dict(WALKS[0], name="fp8 rows of magnitude 3", seed=0))
    assert all(x <= 1.0 for x in worst.values()), worst
