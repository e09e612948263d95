"""The connector walks on the host (tests/_connector_shadow.py; tests/test_gpu_connector_walk.py replays the same lists on the GPU):
the generator emits valid calls only and is a pure function of its arguments, the shadow's tail and pair decisions are those of the
connector's pure plan functions at every step, and the committed seeds COVER what the walks are for -- asserted, so that a change of
the generator or of a seed cannot quietly lose a case."""
import copy

import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests._connector_shadow import (EXTRA_READS, H, D, L, MAX_LIVE, MUTATING, PAIRS, READS, T, WALKS, WINDOWS, Shadow, ancestors, hostile_of,
                                     is_read, k_scales, named, rows_of, sandwiches, walk)

TRANSITIONS = ("truncate read", "truncate tail kept", "truncate tail dropped", "fork held", "fork read", "fork even",
               "fork read after its source changed", "source read after its fork changed", "freed id reused", "read back, re-paired by append",
               "read back, re-paired by commit", "cut to 0 and read", "read at T - 1", "read at T", "member cut to 0",
               "default prefix length after the prefix changed")


def _ops(w):
    return walk(w["seed"], w["n_ops"], w)


def _valid(op, lens):
    """what the connector would refuse, or what would leave the layout: asserted not to occur"""
    kind = op["op"]
    ids = named(op)
    if kind == "prefill":
        assert op["rid"] not in lens and 0 <= op["n"] <= T and len(lens) < MAX_LIVE
        return
    if kind == "fork":
        assert len(lens) + len(op["news"]) <= MAX_LIVE and len(set(op["news"])) == len(op["news"])
        assert all(s in lens for s in op["srcs"]) and not any(r in lens for r in op["news"])
        assert all(0 <= n <= lens[s] for s, n in zip(op["srcs"], op["lengths"]))
        return
    assert all(r in lens for r in ids), (op, sorted(lens))
    if kind in ("free", "reuse"):
        return
    assert len(set(op["ids"])) == len(op["ids"]) >= 1
    S = op.get("S", 0)
    if kind == "append":
        assert all(lens[r] < T for r in ids)
    elif kind == "append_tokens":
        assert all(0 <= n <= S and lens[r] + n <= T for r, n in zip(ids, op["accept"])) and any(op["accept"])
    elif kind in ("append_path", "commit"):
        paths = op["paths"] if kind == "append_path" else op["nodes"]
        assert any(paths)
        for r, path in zip(ids, paths):
            assert lens[r] + len(path) <= T and all(0 <= j < S for j in path)
            if op["parents"] is not None:
                assert len(op["parents"]) == S <= 15 and (not path or path == ancestors(op["parents"], path[-1]))
            else:
                assert all(a < b for a, b in zip(path, path[1:]))
    elif kind == "truncate":
        assert all(0 <= n <= lens[r] for r, n in zip(ids, op["new"])) and any(n != lens[r] for r, n in zip(ids, op["new"]))
    elif is_read(op):
        assert 0 <= op["layer"] < L and all(lens[r] + S <= T for r in op["ids"])
        if "W" in op:
            assert op["W"] in WINDOWS
        if "parents" in op:
            assert len(op["parents"]) == S and all(-1 <= p < j for j, p in enumerate(op["parents"]))
            assert kind != "spec_tree" or S <= 15
        if kind == "spec_chain":
            assert 1 <= S <= 15
        if op.get("n_new") is not None:
            assert all(0 <= n <= S for n in op["n_new"])
        if "prefix" in op:
            assert op["prefix"] not in op["ids"] and 2 <= len(op["ids"]) <= 3
            if op["plens"] is None:
                assert lens[op["prefix"]] % 2 == 0
            else:
                assert all(n % 2 == 0 and 0 <= n <= (lens[op["prefix"]] & ~1) for n in op["plens"])
    else:
        raise AssertionError(("an unknown operation", op))


def _trace(oracle, w, ops):
    """the walk through the shadow: (operation kinds with their counts, transitions seen)"""
    sh = Shadow(oracle, w["scheme"], k_scales(w["seed"]) if w["prescale"] else None)
    seen, kinds = set(), {}
    forks = []                                         # [source, fork, source changed, fork changed]
    zeroed, shared_members, defaults = set(), set(), {}
    for i, op in enumerate(ops):
        kind = op["op"]
        kinds[kind] = kinds.get(kind, 0) + 1
        lens = sh.lengths()
        _valid(op, lens)
        if is_read(op):
            for r in op["ids"]:
                if lens[r] == T - 1:
                    seen.add("read at T - 1")
                if lens[r] == T:
                    seen.add("read at T")
                if r in zeroed and lens[r] == 0:
                    seen.add("cut to 0 and read")
                    if kind == "shared" and r in shared_members:
                        seen.add("member cut to 0")
            if kind == "shared":
                shared_members |= set(op["ids"])
                if op["plens"] is None:                # the call takes the prefix's length itself: the same call again, the prefix longer or shorter
                    was = defaults.get((tuple(op["ids"]), op["prefix"]))
                    if was is not None and was != lens[op["prefix"]] and i >= 2 and not is_read(ops[i - 1]) and ops[i - 2] == dict(op, seed=ops[i - 2]["seed"]):
                        seen.add("default prefix length after the prefix changed")
                    defaults[(tuple(op["ids"]), op["prefix"])] = lens[op["prefix"]]
            for f in forks:
                if f[1] in op["ids"] and f[2]:
                    seen.add("fork read after its source changed")
                if f[0] in op["ids"] and f[3]:
                    seen.add("source read after its fork changed")
            continue
        before = {r: q.version for r, q in sh.req.items()}
        mark = len(sh.events)
        decided = sh.apply(op)
        after = sh.lengths()
        assert all(0 <= n <= T for n in after.values()) and len(after) <= MAX_LIVE, (i, op)
        # ---- the shadow's decisions against the connector's pure plan functions
        if kind == "truncate":
            drops, reads = SpeckvKVConnector.truncate_plan([lens[r] for r in op["ids"]], op["new"])
            want = ["read" if b in {x for x, _ in reads} else "drop" if b in drops else "same" if n == lens[r] else "even"
                    for b, (r, n) in enumerate(zip(op["ids"], op["new"]))]
            assert decided == want, (i, op, decided, want)
            assert all(page == (op["new"][b] - 1) // 2 for b, page in reads)
            for how, r, n in zip(decided, op["ids"], op["new"]):
                if how == "read":
                    seen.add("truncate read")
                if how == "drop":
                    seen.add("truncate tail dropped")
                if how == "same" and n & 1:
                    seen.add("truncate tail kept")
                if n == 0 and how != "same":
                    zeroed.add(r)
        elif kind == "fork":
            n_pages, tails = SpeckvKVConnector.fork_plan([lens[s] for s in op["srcs"]], op["lengths"])
            assert decided == list(zip(n_pages, tails)), (i, op, decided)
            for (_, how), s, r in zip(decided, op["srcs"], op["news"]):
                seen.add({None: "fork even", "held": "fork held", "read": "fork read"}[how])
                forks.append([s, r, False, False])
        elif kind in ("append_tokens", "append_path", "commit"):
            counts = [len(p) for p in (op["paths"] if kind == "append_path" else op["nodes"])] if kind != "append_tokens" else op["accept"]
            pairs, tails = SpeckvKVConnector.commit_plan([lens[r] for r in op["ids"]], counts)
            want_pairs = [[] for _ in op["ids"]]
            for p, group in enumerate(pairs):
                for b, page, s0, s1 in group:
                    assert page == (lens[op["ids"][b]] & ~1) // 2 + p and len(want_pairs[b]) == p
                    want_pairs[b].append((s0, s1))
            want_tails = [None] * len(op["ids"])
            for b, s in tails:
                want_tails[b] = s
            assert decided == (want_pairs, want_tails), (i, op, decided)
        for r in list(zeroed):
            if r not in after or after[r] != 0:
                zeroed.discard(r)
        for name, *rest in sh.events[mark:]:
            if name == "reused":
                seen.add("freed id reused")
            if name == "repaired" and rest[0] in ("append", "commit"):
                seen.add("read back, re-paired by " + rest[0])
        if kind == "prefill" and any(o["op"] in ("free", "reuse") and o["rid"] == op["rid"] for o in ops[:i]):
            seen.add("freed id reused")
        if kind == "fork" and any(o["op"] == "free" and o["rid"] in op["news"] for o in ops[:i]):
            seen.add("freed id reused")
        gone = {op["rid"]} if kind in ("free", "reuse") else set()
        forks = [f for f in forks if f[0] not in gone and f[1] not in gone]
        if kind != "fork":
            for f in forks:
                f[2] = f[2] or sh.req[f[0]].version != before.get(f[0])
                f[3] = f[3] or sh.req[f[1]].version != before.get(f[1])
        shared_members -= gone
    return kinds, seen


def test_the_generator_is_a_pure_function_of_its_arguments():
    w = WALKS[0]
    a, b = _ops(w), _ops(w)
    assert a == b and len(a) == w["n_ops"]
    frozen = copy.deepcopy(a)
    for op in a:
        if "seed" in op and not is_read(op):
            k1, v1 = rows_of(op)
            k2, v2 = rows_of(op)
            assert np.array_equal(k1.view(np.uint16), k2.view(np.uint16)) and np.array_equal(v1.view(np.uint16), v2.view(np.uint16))
            assert np.isfinite(k1.astype(np.float32)).all() and k1.shape[2:] == (L, H, D)
            for b_, j in hostile_of(op):
                assert np.all(np.abs(v1[b_, j].astype(np.float32)) == 1000.0)
            break
    assert a == frozen
    assert _ops(dict(w, seed=w["seed"] + 1)) != a


def test_the_walks_differ_and_hold_the_issues_table():
    assert len(WALKS) == 8 and len({w["seed"] for w in WALKS}) == 8 and len({w["name"] for w in WALKS}) == 8
    assert sorted((w["scheme"], w["striped"], w["prescale"]) for w in WALKS) == sorted(
        [(s, p, False) for s in ("fp8", "int4", "mxfp4") for p in (False, True)] + [("fp8", False, True), ("int4", False, True)])
    for s in ("fp8", "int4", "mxfp4"):
        assert {1, 16} <= {w["rpp"] for w in WALKS if w["scheme"] == s}


@pytest.fixture(scope="module")
def traces(oracle):
    return {w["name"]: (_ops(w),) + _trace(oracle, w, _ops(w)) for w in WALKS}


@pytest.mark.parametrize("w", WALKS, ids=[w["name"] for w in WALKS])
def test_every_operation_kind_occurs_at_least_twice_per_walk(traces, w):
    """... and every step of the walk is a valid call whose tail and pair decisions are the plan functions' (_trace asserts both)"""
    _, kinds, _ = traces[w["name"]]
    few = {k: kinds.get(k, 0) for k in MUTATING + READS if kinds.get(k, 0) < 2}
    assert not few, (w["name"], few)


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_the_walks_of_a_scheme_cover_every_transition(traces, scheme):
    seen = set()
    for w in WALKS:
        if w["scheme"] == scheme:
            seen |= traces[w["name"]][2]
    assert not [t for t in TRANSITIONS if t not in seen], (scheme, [t for t in TRANSITIONS if t not in seen])


def test_every_mutation_is_sandwiched_between_two_reads_of_every_kind(traces):
    """for every mutating kind M and every read kind R: "R over ids, M on a subset of ids, R over the same ids" occurs in a committed
    walk, with nothing in between -- the pattern that shows a step cache that outlived a mutation"""
    have = {}
    for w in WALKS:
        for m, r, _ in sandwiches(traces[w["name"]][0]):
            have[(m, r)] = have.get((m, r), 0) + 1
    missing = [p for p in PAIRS if p not in have]
    assert not missing, missing
    # the reads outside the table (attend_chunk(window=), attend_chunk_shared) run between the sandwiches
    for w in WALKS:
        assert any(o["op"] in EXTRA_READS for o in traces[w["name"]][0]), w["name"]
