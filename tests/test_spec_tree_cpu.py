"""-m "not gpu": tree-shaped drafts in the multi-position decode step (speckv_ext_attend_fold_masked, SpeckvKVConnector.tree_masks /
attend_spec(parents=...) / append_path) as far as they can be judged without a device -- the entry in header, library and binding, its
argument checks on the "/dev/null" library, the mask words of tree_masks against a brute-force walk up the ancestors, and the pair /
tail bookkeeping of append_path against a loop of single append() calls on a library stand-in that records what would be written."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_connector
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import EXT_ABI_VERSION, HELD_MAX, SpeckvError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, DRIVER = -4, -2                                       # SPECKV_ERR_INVAL, SPECKV_ERR_DRIVER (include/speckv.h)
tree_masks = SpeckvKVConnector.tree_masks


@pytest.fixture()
def nulllib():
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    yield lib
    lib.finalize()


def test_entry_is_declared_exported_and_bound():
    """include/speckv_ext.h declares speckv_ext_attend_fold_masked with the mask arguments in the place of d_base / d_n_q, the library
    exports it, the binding registers it; an additive entry: the ABI version is still 6"""
    src = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    m = re.search(r"speckv_status_t\s+speckv_ext_attend_fold_masked\(([^;]*)\);", src)
    assert m, "the header does not declare speckv_ext_attend_fold_masked"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["uint32_t n_rows", "const uint32_t* d_rows", "uint32_t heads", "uint32_t g", "uint32_t rows_per_pos", "const void* d_q_f16",
                    "const void* d_k_held", "const void* d_v_held", "uint64_t seq_stride_elems", "uint64_t pos_stride_elems", "const uint32_t* d_mask",
                    "uint32_t mask_stride", "float sm_scale", "float* d_out", "float* d_lse", "void* stream"]
    assert re.search(r"#define SPECKV_EXT_ABI_VERSION 6u", src) and EXT_ABI_VERSION == 6
    lib = C.CDLL(pkg.build_library())
    assert hasattr(lib, "speckv_ext_attend_fold_masked")
    assert hasattr(lib, "speckv_ext_attend_fold_held")                    # (and its neighbour stays)
    assert callable(getattr(pkg.SpeckvLib, "attend_fold_masked"))


# heads, g, rows_per_pos, seq_stride, pos_stride, mask given, mask_stride, lse given
BAD = {
    "no d_mask": (8, 8, 4, 17 * 1024, 1024, False, 2, True),
    "mask_stride below the query positions": (8, 8, 4, 17 * 1024, 1024, True, 1, True),
    "mask_stride 0": (8, 16, 1, 17 * 1024, 1024, True, 0, True),
    # the sets speckv_ext_attend_fold_held refuses (tests/test_spec_step_cpu.py)
    "g not a multiple of rows_per_pos": (8, 8, 3, 17 * 1024, 1024, True, 16, True),
    "g above 16": (8, 32, 2, 17 * 1024, 1024, True, 16, True),
    "more than 16 query positions": (8, 17, 1, 17 * 1024, 1024, True, 17, True),
    "rows_per_pos 0": (8, 8, 0, 17 * 1024, 1024, True, 16, True),
    "no d_lse": (8, 8, 4, 17 * 1024, 1024, True, 2, False),
    "position stride not a multiple of 8": (8, 8, 4, 17 * 1024, 1028, True, 2, True),
    "position stride below one row of heads": (8, 8, 4, 17 * 1024, 1016, True, 2, True),
    "sequence stride not a multiple of 8": (8, 8, 4, 17 * 1024 + 4, 1024, True, 2, True),
    "sequence stride below the query positions": (8, 8, 4, 1024, 1024, True, 2, True),
    "no heads": (0, 8, 4, 17 * 1024, 1024, True, 2, True),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_fold_masked_refuses_bad_arguments_without_a_device(nulllib, case):
    """every bad argument set is SPECKV_ERR_INVAL on the library without a data path -- judged before any device is asked for"""
    heads, g, rpp, seq_stride, pos_stride, with_mask, mask_stride, with_lse = BAD[case]
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    with pytest.raises(SpeckvError) as e:
        nulllib.attend_fold_masked(1, 0, heads, g, rpp, p, p, p, seq_stride, pos_stride, p if with_mask else 0, mask_stride, 0.1, p,
                                   p if with_lse else 0, 1)
    assert e.value.status == INVAL, case


def test_fold_masked_has_no_cpu_fallback(nulllib):
    """a good argument set on the fake device fails loudly (no data path) and leaves the buffers alone"""
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    for g, rpp, mask_stride in ((8, 4, 2), (8, 4, 5), (16, 1, 16)):
        with pytest.raises(SpeckvError) as e:
            nulllib.attend_fold_masked(1, 0, 8, g, rpp, p, p, p, 17 * 1024, 1024, p, mask_stride, 0.1, p, p, 1)
        assert e.value.status == DRIVER
    assert bytes(buf) == bytes(4096)


def brute_masks(parents, base, n_new):
    """the definition, one node at a time: walk up from the node; visible = the base positions, the node and everything met on the
    way; a node or an ancestor at or past the live count kills the node"""
    words = []
    for j in range(len(parents)):
        word, a, dead = (1 << base) - 1, j, False
        while a != -1:
            dead |= a >= n_new
            word |= 1 << (base + a)
            a = parents[a]
        words.append(0 if dead else word)
    return words


def test_tree_masks_chain_and_star():
    for base in (0, 1):
        for S in (1, 2, 4, 16):
            chain = list(range(-1, S - 1))
            assert tree_masks(chain, [base]) == [[(1 << (base + j + 1)) - 1 for j in range(S)]]      # the rule of speckv_ext_attend_fold_held
            assert tree_masks([-1] * S, [base]) == [[((1 << base) - 1) | 1 << (base + j) for j in range(S)]]   # the base bits and the node's own
    # a trunk of 2 with two branches of 2, behind an odd last position
    assert tree_masks([-1, 0, 1, 2, 1, 4], [1]) == [[0b11, 0b111, 0b1111, 0b11111, 0b100111, 0b1100111]]
    # one tree for every request of a batch: a row per request, each with its own base
    assert tree_masks([-1, 0, 0], [0, 1, 0]) == [[0b1, 0b11, 0b101], [0b11, 0b111, 0b1011], [0b1, 0b11, 0b101]]
    assert tree_masks([-1, 0], []) == []
    assert all(0 <= w < 1 << HELD_MAX for row in tree_masks(list(range(-1, 15)), [1]) for w in row)


def test_tree_masks_random_trees_against_an_ancestor_walk():
    rng = np.random.default_rng(17)
    for _ in range(300):
        B, S = int(rng.integers(1, 6)), int(rng.integers(1, 17))
        trees = [[int(rng.integers(-1, j)) for j in range(S)] for _ in range(B)]
        base = [int(x) for x in rng.integers(0, 2, B)]
        n_new = [int(x) for x in rng.integers(0, S + 1, B)]
        assert tree_masks(trees, base) == [brute_masks(t, x, S) for t, x in zip(trees, base)]
        got = tree_masks(trees, base, n_new)
        assert got == [brute_masks(t, x, n) for t, x, n in zip(trees, base, n_new)]
        for row, tree, x, n in zip(got, trees, base, n_new):
            assert all(w == 0 for w in row[n:])                            # nodes at or above the live count
            assert all((w >> (x + j)) & 1 for j, w in enumerate(row) if w)  # a live node sees itself ...
            assert all(w >> (x + j + 1) == 0 for j, w in enumerate(row))     # ... and nothing behind it
        assert tree_masks(trees[0], base) == [brute_masks(trees[0], x, S) for x in base]          # one tree for all


def test_tree_masks_cut_offs():
    # a dead ancestor makes the node dead, wherever the node itself lies: node 1 hangs below node 2's sibling ...
    assert tree_masks([-1, -1, 0, 1], [0], [2]) == [[0b1, 0b10, 0, 0]]
    assert tree_masks([-1, 0, 1, 2], [1], [0]) == [[0, 0, 0, 0]]
    assert tree_masks([-1, 0, 1, 2], [1], [4]) == [[0b11, 0b111, 0b1111, 0b11111]]
    # per-request trees with per-request counts
    assert tree_masks([[-1, 0, 0], [-1, -1, 1]], [0, 1], [3, 2]) == [[0b1, 0b11, 0b101], [0b11, 0b101, 0]]


@pytest.mark.parametrize("parents,base,n_new", [
    ([0, 0], [0], None),                      # a node its own parent
    ([-1, 1], [0], None),                     # ... likewise
    ([-1, 2, 1], [0], None),                  # a parent behind its child
    ([-2, 0], [0], None),                     # below -1
    ([-1, 0.5], [0], None),                   # not an integer
    ([-1, True], [0], None),
    ([], [0], None),                          # no node
    (list(range(-1, 16)), [0], None),         # 17 nodes
    (list(range(-1, 15)), [2], None),         # 16 nodes behind 2 held positions: past SPECKV_HELD_MAX
    ([-1, 0], [-1], None),                    # base below 0
    ([[-1, 0], [-1, 0]], [0], None),          # two trees, one request
    ([[-1, 0], [-1]], [0, 0], None),          # trees of different sizes
    ([-1, 0], [0], [3]),                      # n_new above S
    ([-1, 0], [0], [-1]),
    ([-1, 0], [0, 1], [1]),                   # one count, two requests
])
def test_tree_masks_refuses_malformed_input(parents, base, n_new):
    with pytest.raises(ValueError):
        tree_masks(parents, base, n_new)


class _RecordingLib:
    """what the connector asks of the library, recorded: every page image a write would store, by (handle, first page)"""

    def __init__(self):
        self.handles, self.writes = 0, []

    def set_compression_scheme(self, scheme): pass
    def set_layout(self, *a): pass
    def bind_request(self, *a): pass

    def alloc(self, nbytes):
        self.handles += 1
        return self.handles

    def write_strided(self, handle, first, step, n_pages, src, stream):
        self.writes.append((int(handle), int(first), int(step), int(n_pages), C.string_at(int(src), int(n_pages) * 4096)))

    def write_strided_batch(self, handles, firsts, srcs, step, n_each, stream):
        srcs = [int(x) for x in srcs]
        assert all(b - a == n_each * 4096 for a, b in zip(srcs, srcs[1:]))      # source offsets: image i at i * step bytes
        for h, f, s in zip(handles, firsts, srcs):
            self.write_strided(h, f, step, n_each, s, stream)


class _Stream:
    cuda_stream = 1

    def wait_stream(self, other): pass


def _paths_of(parents):
    """every root-to-node chain of a tree, the empty one first"""
    paths = [[]]
    for j, p in enumerate(parents):
        paths.append(([] if p < 0 else next(x for x in paths if x and x[-1] == p)) + [j])
    return paths


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_append_path_writes_what_single_appends_write(monkeypatch, seed):
    """SpeckvKVConnector.append_path against a loop of SpeckvKVConnector.append over the path's rows on a recording library (host
    tensors stand in for device buffers): the same page numbers with the same page images per request, the same lengths and the same
    tails.  A path that is not a chain of `parents` raises and changes nothing."""
    import torch
    st = _Stream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    L, H, D, T, B, S = 2, 8, 128, 64, 5, 6
    ids = [11, 12, 13, 14, 15]
    a, b = SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8"), SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8")
    for conn in (a, b):
        for rid in ids:
            conn.add_request(rid)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    shared = [-1, 0, 1, 2, 1, 4]                                            # a trunk of 2 with two branches of 2
    keep = []
    for step in range(6):
        k = torch.randn((B, S, L, H, D), generator=gen).to(torch.float16)
        v = torch.randn((B, S, L, H, D), generator=gen).to(torch.float16)
        if step % 2:                                                        # one tree per request
            parents = [[int(rng.integers(-1, j)) for j in range(S)] for _ in range(B)]
            trees = parents
        else:
            parents, trees = shared, [shared] * B
        paths = []
        for i in range(B):
            choice = _paths_of(trees[i])
            paths.append(choice[int(rng.integers(0, len(choice)))])
        if step == 0:
            paths = [[], [0], [0, 1, 4, 5], [0, 1, 2, 3], [0, 1]]           # empty, a lone node, the second branch, the first, the trunk
        keep.append(a.append_path(ids, k, v, paths, parents if step != 2 else None, stream=st))
        for t in range(S):                                                  # the same rows one position at a time
            members = [i for i in range(B) if len(paths[i]) > t]
            if members:
                rows = torch.tensor([paths[i][t] for i in members])
                keep.append(b.append([ids[i] for i in members], k[torch.tensor(members), rows], v[torch.tensor(members), rows], stream=st))
        for rid in ids:
            assert a.length(rid) == b.length(rid)
            ra, rb = a.requests[rid], b.requests[rid]
            assert (ra.tail_k is None) == (rb.tail_k is None) == (a.length(rid) % 2 == 0)
            if ra.tail_k is not None:
                assert torch.equal(ra.tail_k, rb.tail_k) and torch.equal(ra.tail_v, rb.tail_v)
    wa, wb = sorted(a.lib.writes), sorted(b.lib.writes)
    assert len(wa) == len(wb) > 10
    assert [w[:4] for w in wa] == [w[:4] for w in wb]                       # handle, first page, page step, pages
    assert all(x[4] == y[4] for x, y in zip(wa, wb))                        # the page images
    # refusals: nothing is written, no length or tail moves
    state = lambda: ([a.length(rid) for rid in ids], [id(a.requests[rid]._tail) for rid in ids], len(a.lib.writes), a._epoch)
    before = state()
    for bad, tree in (([[0, 1, 2, 5], [], [], [], []], shared),             # node 5 hangs below 4, not 2
                      ([[1, 2], [], [], [], []], shared),                   # does not start at a child of the context
                      ([[0, 1], [0], [0], [4, 1], [0]], shared),            # a later request's path runs upwards
                      ([[0, 4], [], [], [], []], shared),                   # skips a node
                      ([[0, 6], [], [], [], []], None),                     # no such node
                      ([[0, -1], [], [], [], []], None),
                      ([[2, 1], [], [], [], []], None),                     # without a tree: nodes ascend
                      ([[1, 1], [], [], [], []], None),
                      ([[0], [0]], shared),                                 # one path per request
                      ([[0], [], [], [], []], [-1, 0, 0])):                 # a tree of another size
        with pytest.raises(ValueError):
            a.append_path(ids, k, v, bad, tree, stream=st)
        assert state() == before
    assert a.append_path(ids, k, v, [[]] * B, shared, stream=st) == [] and state() == before       # nothing accepted: nothing happens
