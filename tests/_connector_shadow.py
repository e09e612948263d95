"""The shadow model of SpeckvKVConnector and the generator of its random walks (tests/test_connector_walk_cpu.py checks the walks'
coverage on the host, tests/test_gpu_connector_walk.py replays them on the MI355X).  numpy and the oracle only: no torch, no product code.

The shadow restates the connector's DOCUMENTED behaviour.  A live request is its length, the ENCODER INPUTS of its stored pairs -- the
two fp16 rows of every (layer, kind) in the stored scaling, K / scale under a K pre-scale -- and the tail rows it holds outside the
pool.  Rows arrive one by one; a row that completes a pair stores (tail, row); an odd remainder is the tail as given.  truncate drops
the pairs from new // 2 on and, for an odd shorter length, takes the even row of pair (new - 1) // 2 THROUGH THE FORMAT ONCE (the
oracle's decode of its encode of the pair's page) as the tail; fork copies pairs as records and takes its tail from the source's tail
(an odd length equal to the source's) or through the format once (an odd shorter one).  Records behind a cut are not in the shadow.

An operation is a dict of ints, lists and None; walk() makes a list of them from (seed, n_ops, profile) alone and consults nothing but
the lengths they lead to, so the same list replays on the host and on the GPU.  The rows of an operation come from its own seed
(step_rows); the rows an operation drops -- rejected draft positions, tree nodes off the committed path, positions at or behind a
ragged step's live count, the end of an optimistic commit that the next truncate takes back -- are HOSTILE: K x 200, V = +-1000."""
import numpy as np

H, D = 8, 128
L, T = 2, 256
MAX_LIVE = 6
WINDOWS = (33, 64)
SCHEME_CODES = {"fp8": 4, "int4": 3, "mxfp4": 5}
K_HOSTILE, V_HOSTILE = 200.0, 1000.0
MAGNITUDES = (0.3, 1.0, 3.0)

MUTATING = ("append", "append_tokens", "append_path", "commit", "truncate", "fork", "reuse")
READS = ("attend", "attend_layers", "attend_window", "spec_chain", "spec_tree", "chunk", "chunk_parents", "tree_window", "shared")
EXTRA_READS = ("chunk_window", "chunk_shared")
OTHER = ("prefill", "free")
PAIRS = [(m, r) for m in MUTATING for r in READS]

# the committed walks: tests/test_gpu_connector_walk.py runs exactly these, tests/test_connector_walk_cpu.py asserts their coverage.
# slot: where in the table of (read, mutation) pairs the walk starts (walk()); rpp: query rows per kv head and position.
# 72 operations: a sandwich and what runs between two of them take about four, and a walk needs 14 sandwiches in a row to hold every
# mutating kind twice; the seeds were searched on the host until the coverage assertions of tests/test_connector_walk_cpu.py held.
N_OPS = 72
WALKS = [
    dict(name="fp8-one", scheme="fp8", striped=False, prescale=False, rpp=4, slot=0, seed=24101, n_ops=N_OPS),
    dict(name="fp8-striped3", scheme="fp8", striped=True, prescale=False, rpp=1, slot=1, seed=2102, n_ops=N_OPS),
    dict(name="fp8-prescale", scheme="fp8", striped=False, prescale=True, rpp=16, slot=2, seed=15103, n_ops=N_OPS),
    dict(name="int4-one", scheme="int4", striped=False, prescale=False, rpp=4, slot=3, seed=2104, n_ops=N_OPS),
    dict(name="int4-striped3", scheme="int4", striped=True, prescale=False, rpp=16, slot=4, seed=19105, n_ops=N_OPS),
    dict(name="int4-prescale", scheme="int4", striped=False, prescale=True, rpp=1, slot=5, seed=50106, n_ops=N_OPS),
    dict(name="mxfp4-one", scheme="mxfp4", striped=False, prescale=False, rpp=1, slot=6, seed=35107, n_ops=N_OPS),
    dict(name="mxfp4-striped3", scheme="mxfp4", striped=True, prescale=False, rpp=16, slot=7, seed=81108, n_ops=N_OPS),
]


# ----------------------------------------------------------------------------- the rows of an operation
def step_rows(seed, B, S, hostile=()):
    """(k, v) fp16 [B][S][L][H][D] of an operation: randn x a magnitude per position from MAGNITUDES; hostile = [(b, j)]: the positions
    the operation drops, K x 200 and V = +-1000"""
    rng = np.random.default_rng(seed)
    mag = rng.choice(np.asarray(MAGNITUDES, np.float32), size=(B, S))[:, :, None, None, None]
    k = rng.standard_normal((B, S, L, H, D), dtype=np.float32) * mag
    v = rng.standard_normal((B, S, L, H, D), dtype=np.float32) * mag
    for b, j in hostile:
        k[b, j] *= K_HOSTILE
        v[b, j] = np.where(v[b, j] < 0, -V_HOSTILE, V_HOSTILE)
    return k.astype(np.float16), v.astype(np.float16)


def queries(seed, *shape):
    """the fp16 query rows of a read operation"""
    return np.random.default_rng([seed, 7]).standard_normal(shape, dtype=np.float32).astype(np.float16)


def k_scales(seed):
    """a K pre-scale [L][H][D] of powers of two in 2**-2 .. 2**2"""
    return np.exp2(np.random.default_rng([seed, 11]).integers(-2, 3, size=(L, H, D))).astype(np.float32)


def hostile_of(op):
    """[(b, j)] of the positions the operation drops (see the module's docstring)"""
    kind = op["op"]
    if kind == "append_tokens":
        return [(b, j) for b, n in enumerate(op["accept"]) for j in range(n, op["S"])]
    if kind in ("append_path", "commit"):
        keep = op["paths"] if kind == "append_path" else op["nodes"]
        cut = op.get("hostile_from") or [None] * len(keep)            # an optimistic commit: the next truncate takes these back
        return [(b, j) for b, path in enumerate(keep) for j in range(op["S"])
                if j not in path or (cut[b] is not None and path.index(j) >= cut[b])]
    if kind in ("spec_chain", "chunk", "chunk_window", "chunk_shared") and op.get("n_new") is not None:
        return [(b, j) for b, n in enumerate(op["n_new"]) for j in range(n, op["S"])]
    return []


def rows_of(op):
    """(k, v) [B][S][L][H][D] of an operation that brings rows: the batch of an append has S = 1, a prefill is one request of n rows"""
    kind = op["op"]
    if kind in ("prefill", "reuse"):
        return step_rows(op["seed"], 1, op["n"])
    if kind == "append":
        return step_rows(op["seed"], len(op["ids"]), 1)
    return step_rows(op["seed"], len(op["ids"]), op["S"], hostile_of(op))


def ancestors(parents, j):
    """node j and its ancestors, root first"""
    path = []
    while j >= 0:
        path.append(j)
        j = parents[j]
    return path[::-1]


# ----------------------------------------------------------------------------- the shadow
class _Pair:
    """one stored pair: the encoder input [L][kind][2 rows][H][D] fp16 and, once asked for, the same through the format"""
    __slots__ = ("inp", "dec")

    def __init__(self, inp):
        self.inp, self.dec = inp, None


class _Req:
    __slots__ = ("n", "pairs", "tail", "tail_read", "version")

    def __init__(self):
        self.n, self.pairs, self.tail, self.tail_read, self.version = 0, [], None, False, 0


class Shadow:
    """scheme: a name of SCHEME_CODES; kscale: the K pre-scale [L][H][D] (powers of two) or None.  as_given_on_read_back: a WRONG
    shadow for the walk's self-test -- a tail read back is the row as it was given, not the decoded one."""

    def __init__(self, oracle, scheme, kscale=None, as_given_on_read_back=False):
        self.oracle, self.scheme, self.code = oracle, scheme, SCHEME_CODES[scheme]
        self.kscale = None if kscale is None else np.asarray(kscale, np.float32)
        self.req = {}
        self.clock = 0                       # a request's version is the clock at its last change: never the same for two states
        self.events = []                     # what the coverage assertions count: (name, ...) tuples
        self.wrong_read_back = as_given_on_read_back

    # ---- values
    def stored_k(self, k):
        """K rows [...][L][H][D] in the stored scaling: k / scale, rounded to fp16 once"""
        return k if self.kscale is None else (k.astype(np.float32) / self.kscale).astype(np.float16)

    def query(self, q, layer):
        """query rows [...][H][rows][D] as the kernels are given them: q x scale, rounded to fp16 once"""
        return q if self.kscale is None else (q.astype(np.float32) * self.kscale[layer][:, None, :]).astype(np.float16)

    def once(self, pair):
        if pair.dec is None:
            sc, lens, recs = self.oracle.compress_blocks_f16(np.ascontiguousarray(pair.inp).reshape(2 * L, 2 * H * D), self.code, 0)
            pair.dec = self.oracle.decompress_blocks_f16(recs, lens, sc, self.code, 0).reshape(L, 2, 2, H, D)
        return pair.dec

    def _even_row(self, pair):
        src = pair.inp if self.wrong_read_back else self.once(pair)
        return src[:, 0, 0].copy(), src[:, 1, 0].copy()

    def _touch(self, r):
        self.clock += 1
        r.version = self.clock

    def _push(self, rid, k_row, v_row, by):
        """one more row [L][H][D] (K in the stored scaling)"""
        r = self.req[rid]
        if r.tail is None:
            r.tail, r.tail_read = (k_row.copy(), v_row.copy()), False
        else:
            if r.tail_read:
                self.events.append(("repaired", by))
            r.pairs.append(_Pair(np.stack((np.stack((r.tail[0], k_row), axis=1), np.stack((r.tail[1], v_row), axis=1)), axis=1)))
            r.tail = None
        r.n += 1
        self._touch(r)

    # ---- transitions
    def lengths(self):
        return {rid: r.n for rid, r in self.req.items()}

    def apply(self, op):
        """a mutating operation (reads and unknown kinds change nothing).  Returns what the operation decided, for the comparison with
        the connector's pure plan functions: truncate -> [per request "same" | "read" | "drop" | "even"], fork -> [(pairs, None |
        "held" | "read")], append_tokens / append_path / commit -> ([per request [(first, second)] sources of its pairs, -1 = the held
        tail], [per request the source of its new tail or None])"""
        kind = op["op"]
        if kind in ("prefill", "reuse"):
            if kind == "reuse":
                del self.req[op["rid"]]
                self.events.append(("reused", op["rid"]))
            self.req[op["rid"]] = _Req()
            self._touch(self.req[op["rid"]])
            k, v = rows_of(op)
            k = self.stored_k(k)
            for j in range(op["n"]):
                self._push(op["rid"], k[0, j], v[0, j], kind)
        elif kind == "free":
            del self.req[op["rid"]]
        elif kind == "append":
            k, v = rows_of(op)
            k = self.stored_k(k)
            for b, rid in enumerate(op["ids"]):
                self._push(rid, k[b, 0], v[b, 0], kind)
        elif kind in ("append_tokens", "append_path", "commit"):
            k, v = rows_of(op)
            k = self.stored_k(k)
            taken = {"append_tokens": lambda: [list(range(n)) for n in op["accept"]], "append_path": lambda: op["paths"],
                     "commit": lambda: op["nodes"]}[kind]()
            pairs, tails = [], []
            for b, rid in enumerate(op["ids"]):
                held = ([-1] if self.req[rid].n & 1 else []) + list(range(len(taken[b])))
                pairs.append([(held[2 * p], held[2 * p + 1]) for p in range(len(held) // 2)])
                tails.append(held[-1] if len(held) & 1 and taken[b] else None)
                for j in taken[b]:
                    self._push(rid, k[b, j], v[b, j], kind)
            return pairs, tails
        elif kind == "truncate":
            out = []
            for rid, new in zip(op["ids"], op["new"]):
                r = self.req[rid]
                assert 0 <= new <= r.n
                if new == r.n:
                    out.append("same")
                    continue
                if new & 1:
                    r.tail, r.tail_read = self._even_row(r.pairs[new // 2]), True
                    out.append("read")
                else:
                    out.append("drop" if r.n & 1 else "even")
                    r.tail = None
                r.pairs = r.pairs[:new // 2]
                r.n = new
                self._touch(r)
                if new == 0:
                    self.events.append(("cut_to_zero", rid))
            return out
        elif kind == "fork":
            out = []
            for src, new, n in zip(op["srcs"], op["news"], op["lengths"]):
                s, r = self.req[src], _Req()
                assert 0 <= n <= s.n and new not in self.req
                r.pairs, r.n = list(s.pairs[:n // 2]), n
                how = None
                if n & 1 and n == s.n:
                    r.tail, r.tail_read, how = (s.tail[0].copy(), s.tail[1].copy()), s.tail_read, "held"
                elif n & 1:
                    r.tail, r.tail_read, how = self._even_row(s.pairs[n // 2]), True, "read"
                self.req[new] = r
                self._touch(r)
                out.append((n // 2, how))
            return out
        return None

    # ---- views
    def length(self, rid):
        return self.req[rid].n

    def tail(self, rid):
        """(k, v) [L][H][D] fp16 in the stored scaling, or None"""
        return self.req[rid].tail

    def rows(self, rid, layer, kind):
        """(rows [n][H][D] fp16 as kv_rows must report them, comparable [n][H][D] bool): a stored pair is the oracle's round trip of its
        page, a tail is as held, K is multiplied back by the scale; an element whose STORED value is an fp16 subnormal is not
        comparable bit for bit (the multiply back may flush it)"""
        r = self.req[rid]
        parts = [self.once(p)[layer, kind] for p in r.pairs]
        if r.tail is not None:
            parts.append(r.tail[kind][layer][None])
        x = np.concatenate(parts) if parts else np.zeros((0, H, D), np.float16)
        a = np.abs(x.astype(np.float32))
        ok = ~((a > 0) & (a < 2.0 ** -14))
        if kind == 0 and self.kscale is not None:
            x = (x.astype(np.float32) * self.kscale[layer]).astype(np.float16)
        return x, ok

    def held(self, rid):
        """(k, v) [L][n][H][D] fp16: the encoder inputs of the stored pairs in order and, for an odd length, the tail as its last row"""
        r = self.req[rid]
        out = []
        for kind in (0, 1):
            parts = [p.inp[:, kind] for p in r.pairs] + ([r.tail[kind][:, None]] if r.tail is not None else [])
            out.append(np.ascontiguousarray(np.concatenate(parts, axis=1)) if parts else np.zeros((L, 0, H, D), np.float16))
        return out[0], out[1]

    def region(self, rid, layer):
        """(k_even, v_even) [stored positions][H][D]: the page images of the stored part of one layer, from which the float64
        dequantised K / V come (HeadChecker over _region(k_even, v_even, T))"""
        k, v = self.held(rid)
        even = self.req[rid].n & ~1
        return k[layer, :even], v[layer, :even]


# ----------------------------------------------------------------------------- the generator
def advance(lens, op):
    """the lengths after a mutating operation (the generator's whole view of the state)"""
    kind = op["op"]
    if kind in ("prefill", "reuse"):
        lens[op["rid"]] = op["n"]
    elif kind == "free":
        del lens[op["rid"]]
    elif kind == "append":
        for rid in op["ids"]:
            lens[rid] += 1
    elif kind == "append_tokens":
        for rid, n in zip(op["ids"], op["accept"]):
            lens[rid] += n
    elif kind in ("append_path", "commit"):
        for rid, path in zip(op["ids"], op["paths"] if kind == "append_path" else op["nodes"]):
            lens[rid] += len(path)
    elif kind == "truncate":
        for rid, n in zip(op["ids"], op["new"]):
            lens[rid] = n
    elif kind == "fork":
        for rid, n in zip(op["news"], op["lengths"]):
            lens[rid] = n


def is_read(op):
    return op["op"] in READS or op["op"] in EXTRA_READS


def named(op):
    """the request ids an operation names"""
    kind = op["op"]
    if kind in ("prefill", "reuse", "free"):
        return [op["rid"]]
    if kind == "fork":
        return list(op["srcs"]) + list(op["news"])
    return list(op["ids"]) + ([op["prefix"]] if "prefix" in op else [])


PROMPTS = (1, 2, 5, 33, 37, 64, 98, 131)


def walk(seed, n_ops, profile):
    """n_ops operations from (seed, profile) alone.  The body is a run of SANDWICHES "read R over ids, ONE mutation M on a subset of
    ids, the same read again" (the stale-cache pattern); sandwich t takes R = READS[t % 9], M = MUTATING[t % 7] with t counted from
    profile["slot"] * 8 -- 9 and 7 have no common factor, so 63 sandwiches in a row are the 63 pairs, any 18 in a row hold every kind
    twice, and eight walks whose slots differ cover the table more than twice.  Between sandwiches: requests come (a freed id first)
    and go, a long request is appended to towards T, an optimistic commit is taken back by a truncate, and the reads outside the
    table (attend_chunk(window=), attend_chunk_shared) run."""
    rng = np.random.default_rng(seed)
    lens, ops, freed, fresh = {}, [], [], [1]
    readback, kin = set(), []                 # requests whose tail was read back; (source, fork) pairs

    def new_seed():
        return int(rng.integers(1, 2 ** 31 - 1))

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    def emit(op):
        ops.append(op)
        advance(lens, op)
        kind = op["op"]
        if kind == "truncate":
            for rid, n in zip(op["ids"], op["new"]):
                readback.add(rid) if n & 1 else readback.discard(rid)
        elif kind == "fork":
            for s, r, n in zip(op["srcs"], op["news"], op["lengths"]):
                kin.append((s, r))
                if n & 1 and n < lens[s]:
                    readback.add(r)
        elif kind in ("free", "reuse"):
            readback.discard(op["rid"])
        elif kind in MUTATING:
            for rid in named(op):
                if not lens[rid] & 1:
                    readback.discard(rid)

    def new_id():
        if freed and rng.random() < 0.8:
            return freed.pop(0)
        fresh[0] += 1
        return fresh[0] - 1

    def tree(S, near=False):
        return [int(rng.integers(max(-1, j - 4) if near else -1, j)) for j in range(S)]

    def choose_ids(room=0, least=1, most=3, without=()):
        """distinct live ids with `room` positions left, a fork and its source or a request with a read-back tail preferred"""
        live = [r for r in sorted(lens) if lens[r] + room <= T and r not in without]
        if len(live) < least:
            return None
        n = int(rng.integers(least, min(most, len(live)) + 1))
        first = []
        pairs = [p for p in kin if p[0] in live and p[1] in live]
        if pairs and rng.random() < 0.6:
            first = list(pairs[-1])
        back = [r for r in live if r in readback and r not in first]
        if back and rng.random() < 0.6:
            first.append(pick(back))
        rest = [r for r in live if r not in first]
        order = first + [rest[i] for i in rng.permutation(len(rest))]
        ids = order[:max(n, min(len(first), most))]
        return [ids[i] for i in rng.permutation(len(ids))]

    def ragged(ids, S):
        if rng.random() < 0.5:
            return None
        n = [int(rng.integers(0, S + 1)) for _ in ids]
        n[int(rng.integers(len(ids)))] = S
        return n

    # ---- reads
    def make_read(kind):
        R = profile["rpp"]
        op = dict(op=kind, layer=int(rng.integers(L)), seed=new_seed())
        if kind in ("attend", "attend_layers", "attend_window"):
            op["ids"] = choose_ids(most=4)
            if kind == "attend_window":
                op["W"] = pick(WINDOWS)
        elif kind in ("spec_chain", "spec_tree"):
            S = int(rng.integers(1, 7)) if kind == "spec_chain" else int(rng.integers(2, 9))
            op["ids"] = choose_ids(room=S)
            op["S"] = S
            if kind == "spec_tree":
                op["parents"] = tree(S)
            elif op["ids"]:
                op["n_new"] = ragged(op["ids"], S)
        elif kind in ("chunk", "chunk_window"):
            S = pick((1, 5, 17, 33, 40))
            op["ids"] = choose_ids(room=S)
            op.update(S=S, splits=pick((1, 2, 3)))
            if op["ids"]:
                op["n_new"] = ragged(op["ids"], S)
            if kind == "chunk_window":
                op["W"] = pick(WINDOWS)
        elif kind in ("chunk_parents", "tree_window"):
            S = pick((3, 9, 20, 35))
            op["ids"] = choose_ids(room=S)
            op.update(S=S, parents=tree(S, near=True), splits=pick((1, 2, 3)))
            if kind == "tree_window":
                op["W"] = pick(WINDOWS)
        elif kind in ("shared", "chunk_shared"):
            prefixes = [r for r in sorted(lens) if lens[r] >= 2]
            if not prefixes:
                return None
            op["prefix"] = pick(prefixes)
            S = pick((1, 5, 17)) if kind == "chunk_shared" else 0
            op["ids"] = choose_ids(room=S, least=2, most=3, without=(op["prefix"],))
            if op["ids"]:
                even = lens[op["prefix"]] & ~1
                op["plens"] = [even if rng.random() < 0.6 else 2 * int(rng.integers(0, even // 2 + 1)) for _ in op["ids"]]
                if lens[op["prefix"]] == even and rng.random() < 0.6:
                    op["plens"] = None                                 # the call's default: all the prefix holds, taken from its length
                op["splits"] = pick((0, 1, 2))
                if kind == "chunk_shared":
                    op.update(S=S, n_new=ragged(op["ids"], S))
        return op if op["ids"] else None

    def again(read):
        """the same read over the same tuple of ids at the lengths of now: new query rows, the structure kept; None where the
        lengths no longer allow it"""
        if any(r not in lens for r in named(read)) or any(lens[r] + read.get("S", 0) > T for r in read["ids"]):
            return None
        op = dict(read, seed=new_seed())
        if "plens" in op:
            even = lens[op["prefix"]] & ~1
            if op["plens"] is not None:
                op["plens"] = [min(n, even) for n in op["plens"]]
            elif lens[op["prefix"]] != even:                          # the default takes an even prefix only
                op["plens"] = [even] * len(op["ids"])
        return op

    # ---- mutations on a subset of `ids`
    preferred = [None]                        # a shared read that takes its prefix's length by default: the mutation goes to the prefix

    def subset(ids, ok=lambda r: True, most=None):
        can = [r for r in ids if ok(r)]
        if not can:
            return None
        if preferred[0] in can and rng.random() < 0.6:
            return [preferred[0]]
        n = int(rng.integers(1, min(most or len(can), len(can)) + 1))
        first = [r for r in can if r in readback]
        order = first + [r for r in can if r not in first]
        if not first or rng.random() < 0.4:
            order = [can[i] for i in rng.permutation(len(can))]
        return order[:n]

    def path_in(parents, room):
        nodes = [j for j in range(len(parents)) if len(ancestors(parents, j)) <= room]
        return ancestors(parents, pick(nodes)) if nodes and rng.random() < 0.9 else []

    def make_mut(kind, ids, zero=()):
        op = dict(op=kind)
        if kind == "append":
            sub = subset(ids, lambda r: lens[r] < T)
            return sub and dict(op, ids=sub, seed=new_seed())
        if kind in ("append_tokens", "append_path", "commit"):
            sub = subset(ids, lambda r: lens[r] < T)
            if not sub:
                return None
            room = [T - lens[r] for r in sub]
            op.update(ids=sub, seed=new_seed())
            if kind == "append_tokens":
                S = int(rng.integers(1, 6))
                accept = [int(rng.integers(0, min(S, m) + 1)) for m in room]
                at = int(rng.integers(len(sub)))
                accept[at] = max(accept[at], 1)
                return dict(op, S=S, accept=accept)
            form = "chain" if kind == "commit" and rng.random() < 0.35 else "tree"
            if form == "chain":                                       # a prompt chunk: every position in order
                S = min(pick((2, 7, 18, 33)), max(room))
                return dict(op, S=S, nodes=[list(range(min(S, m))) for m in room], parents=None)
            S = int(rng.integers(2, 9)) if kind == "append_path" or rng.random() < 0.6 else pick((17, 24))
            parents = tree(S, near=S > 16)
            paths = [path_in(parents, m) for m in room]
            if not any(paths):
                paths[0] = [0]
            if kind == "append_path":
                return dict(op, S=S, parents=parents, paths=paths)
            return dict(op, S=S, nodes=paths, parents=parents if S <= 15 and rng.random() < 0.5 else None)
        if kind == "truncate":
            sub = subset(ids, lambda r: lens[r] > 0)
            if not sub:
                return None
            stays = None
            if len(sub) < len(ids) and rng.random() < 0.5:            # ... and a member that stays as it is
                stays = pick([r for r in ids if r not in sub])
                sub = sub + [stays]
            new = []
            for r in sub:
                n, u = lens[r], rng.random()
                if r == stays:
                    new.append(n)
                elif r in zero and rng.random() < 0.7:
                    new.append(0)
                elif u < 0.15:
                    new.append(n)
                elif u < 0.3:
                    new.append(0)
                elif u < 0.7:
                    new.append(2 * int(rng.integers(0, (n + 1) // 2)) + 1 if n > 1 else 0)       # an odd length <= n
                else:
                    new.append(2 * int(rng.integers(0, n // 2 + 1)))                               # an even one
            if all(n == lens[r] for r, n in zip(sub, new)):
                at = [i for i, r in enumerate(sub) if lens[r] > 0][0]
                new[at] = lens[sub[at]] - 1
            return dict(op, ids=sub, new=new)
        if kind == "fork":
            if len(lens) >= MAX_LIVE:
                return None
            sub = subset(ids, most=min(2, MAX_LIVE - len(lens)))
            if not sub:
                return None
            lengths = []
            for r in sub:
                n, u = lens[r], rng.random()
                lengths.append(n if u < 0.4 or n == 0 else 2 * int(rng.integers(0, (n + 1) // 2)) + 1 if u < 0.75 and n > 1
                               else 2 * int(rng.integers(0, n // 2 + 1)))
            return dict(op, srcs=sub, news=[new_id() for _ in sub], lengths=lengths)
        if kind == "reuse":
            return dict(op, rid=pick(ids), n=pick(PROMPTS), seed=new_seed())
        raise ValueError(kind)

    # ---- what runs between the sandwiches
    def housekeeping():
        while len(lens) > MAX_LIVE - 2:
            last = kin[-1] if kin else ()
            rid = pick([r for r in sorted(lens) if r not in last] or sorted(lens))
            emit(dict(op="free", rid=rid))
            freed.append(rid)
        while len(lens) < 3:
            emit(dict(op="prefill", rid=new_id(), n=pick(PROMPTS), seed=new_seed()))
        u = rng.random()
        long = [r for r in sorted(lens) if T - 3 <= lens[r] < T]
        if long and u < 0.5:
            emit(dict(op="append", ids=[long[0]], seed=new_seed()))
            r = again(dict(op="attend", layer=int(rng.integers(L)), ids=[long[0]] + [x for x in sorted(lens) if x != long[0]][:1]))
            emit(r)
        elif u < 0.65:                                                # the whole draft committed, then the accept counts arrive
            ids = choose_ids(room=4)
            if ids:
                accept = [int(rng.integers(0, 4)) for _ in ids]
                before = [lens[r] for r in ids]
                emit(dict(op="commit", ids=ids, S=4, nodes=[[0, 1, 2, 3] for _ in ids], parents=None, hostile_from=accept, seed=new_seed()))
                emit(dict(op="truncate", ids=ids, new=[n + a for n, a in zip(before, accept)]))
                emit(dict(op=pick(("attend", "attend_layers")), layer=int(rng.integers(L)), ids=ids, seed=new_seed()))
        elif u < 0.85:
            r = make_read(pick(EXTRA_READS))
            if r:
                emit(r)

    emit(dict(op="prefill", rid=new_id(), n=T - 3, seed=new_seed()))
    for n in (pick(PROMPTS), pick(PROMPTS), 64):
        emit(dict(op="prefill", rid=new_id(), n=n, seed=new_seed()))
    t = profile["slot"] * 8
    while len(ops) < n_ops:
        housekeeping()
        R, M = READS[t % len(READS)], MUTATING[t % len(MUTATING)]
        t += 1
        read = make_read(R)
        if read is None:
            continue
        pool = list(read["ids"]) + ([read["prefix"]] if "prefix" in read and M != "fork" else [])
        preferred[0] = read["prefix"] if "plens" in read and read["plens"] is None and M != "fork" else None
        mut = make_mut(M, pool, zero=read["ids"] if R == "shared" else ())
        preferred[0] = None
        if not mut:
            continue
        emit(read)
        emit(mut)
        if mut["op"] == "reuse":
            freed[:] = [r for r in freed if r != mut["rid"]]
        second = again(read)
        if second:
            emit(second)
    return ops[:n_ops]


def sandwiches(ops):
    """[(M, R, index of the second read)] of every "read, ONE mutation that names one of the read's requests, the same read kind over
    the same tuple of ids" in a list of operations"""
    found = []
    for i in range(len(ops) - 2):
        a, m, b = ops[i], ops[i + 1], ops[i + 2]
        if is_read(a) and m["op"] in MUTATING and b["op"] == a["op"] and b["ids"] == a["ids"] and b.get("prefix") == a.get("prefix"):
            touched = m["srcs"] if m["op"] == "fork" else named(m)
            if set(touched) & set(named(a)) and set(touched) <= set(named(a)) | set(m.get("news", ())):
                found.append((m["op"], a["op"], i + 2))
    return found
