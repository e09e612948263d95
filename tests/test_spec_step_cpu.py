"""-m "not gpu": the multi-position decode step (speckv_ext_attend_fold_held, SpeckvKVConnector.attend_spec / append_tokens) as far as
it can be judged without a device -- the argument checks of the C entry on the "/dev/null" library, the constant shared by header and
binding, the rule that cuts a step into passes of at most 16 query rows, and the pair / tail bookkeeping of append_tokens against a
loop of single append() calls on a library stand-in that records what would be written where."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_connector
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import HELD_MAX, SpeckvError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, DRIVER = -4, -2                                       # SPECKV_ERR_INVAL, SPECKV_ERR_DRIVER (include/speckv.h)


@pytest.fixture()
def nulllib():
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    yield lib
    lib.finalize()


def test_held_max_is_one_constant():
    src = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    m = re.search(r"#define\s+SPECKV_HELD_MAX\s+(\d+)u", src)
    assert m and int(m.group(1)) == HELD_MAX == 17
    hip = open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", "attend.hip")).read()
    assert re.search(r"constexpr uint32_t kHeldMax = %d;" % HELD_MAX, hip)
    assert re.search(r"#define SPECKV_EXT_ABI_VERSION 6u", src)           # an additive entry: the ABI version stays


# heads, g, rows_per_pos, seq_stride, pos_stride, base given, lse given
BAD = {
    "g not a multiple of rows_per_pos": (8, 8, 3, 17 * 1024, 1024, True, True),
    "g above 16": (8, 32, 2, 17 * 1024, 1024, True, True),
    "more than 16 query positions": (8, 17, 1, 17 * 1024, 1024, True, True),
    "rows_per_pos 0": (8, 8, 0, 17 * 1024, 1024, True, True),
    "no d_base": (8, 8, 4, 17 * 1024, 1024, False, True),
    "no d_lse": (8, 8, 4, 17 * 1024, 1024, True, False),
    "position stride not a multiple of 8": (8, 8, 4, 17 * 1024, 1028, True, True),
    "position stride below one row of heads": (8, 8, 4, 17 * 1024, 1016, True, True),
    "sequence stride not a multiple of 8": (8, 8, 4, 17 * 1024 + 4, 1024, True, True),
    "sequence stride below the query positions": (8, 8, 4, 1024, 1024, True, True),
    "no heads": (0, 8, 4, 17 * 1024, 1024, True, True),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_fold_held_refuses_bad_arguments_without_a_device(nulllib, case):
    """every bad argument set is SPECKV_ERR_INVAL on the library without a data path -- judged before any device is asked for"""
    heads, g, rpp, seq_stride, pos_stride, with_base, with_lse = BAD[case]
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    with pytest.raises(SpeckvError) as e:
        nulllib.attend_fold_held(1, 0, heads, g, rpp, p, p, p, seq_stride, pos_stride, p if with_base else 0, 0, 0.1, p, p if with_lse else 0, 1)
    assert e.value.status == INVAL, case


def test_fold_held_has_no_cpu_fallback(nulllib):
    """a good argument set on the fake device fails loudly (no data path) and leaves the buffers alone"""
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    with pytest.raises(SpeckvError) as e:
        nulllib.attend_fold_held(1, 0, 8, 8, 4, p, p, p, 17 * 1024, 1024, p, 0, 0.1, p, p, 1)
    assert e.value.status == DRIVER
    assert bytes(buf) == bytes(4096)


def test_grouping_rule():
    """S new positions x rows_per_pos query rows go through the kernels 16 rows per kv head at a time: groups of 16 // rows_per_pos
    positions; every position in exactly one group, in order; a group's held positions fit SPECKV_HELD_MAX"""
    groups = SpeckvKVConnector.spec_groups
    assert groups(4, 4) == [(0, 4)]
    assert groups(4, 8) == [(0, 2), (2, 2)]
    assert groups(16, 1) == [(0, 16)]
    assert groups(5, 4) == [(0, 4), (4, 1)]
    assert groups(3, 16) == [(0, 1), (1, 1), (2, 1)]
    assert groups(1, 5) == [(0, 1)]
    for S in range(1, 17):
        for R in range(1, 17):
            gs = groups(S, R)
            assert [j0 for j0, _ in gs] == [sum(n for _, n in gs[:i]) for i in range(len(gs))] and sum(n for _, n in gs) == S
            assert all(1 <= n * R <= 16 for _, n in gs)
            assert all(n == 16 // R for _, n in gs[:-1])                  # only the last group may be short
            assert all(1 + j0 + n <= HELD_MAX for j0, n in gs)            # d_base (<= 1 + j0) + n_q
    for S, R in ((0, 4), (17, 1), (4, 0), (4, 17)):
        with pytest.raises(ValueError):
            groups(S, R)


def test_commit_plan_equals_single_appends():
    """append_tokens' bookkeeping in pure python: for random lengths and accepted counts, the (request, page, sources) of every pair and
    the position left in the tail equal what single appends come to -- append()'s rule: a position at an odd index is written with
    its predecessor to page index // 2, one at an even index waits in the tail"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        B, S = int(rng.integers(1, 7)), int(rng.integers(1, 17))
        lengths = [int(x) for x in rng.integers(0, 9, B)]
        n_accept = [int(x) for x in rng.integers(0, S + 1, B)]
        pairs, tails = SpeckvKVConnector.commit_plan(lengths, n_accept)
        want_pairs, want_tails = set(), {}
        for b in range(B):
            tail = -1 if lengths[b] & 1 else None                          # source of the position waiting in the tail
            for t in range(n_accept[b]):
                pos = lengths[b] + t
                if pos & 1:
                    want_pairs.add((b, pos // 2, tail, t)); tail = None
                else:
                    tail = t
            if n_accept[b] and tail is not None:
                want_tails[b] = tail
        assert {x for group in pairs for x in group} == want_pairs
        assert sum(len(g) for g in pairs) == len(want_pairs)
        assert dict(tails) == want_tails
        assert len(pairs) <= S // 2 + 1                                     # launches of one commit
        for p, group in enumerate(pairs):                                   # one call per pair index: a request at most once in it
            assert len({b for b, *_ in group}) == len(group)
            assert all(pg == (lengths[b] & ~1) // 2 + p for b, pg, _, _ in group)


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


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_append_tokens_writes_what_single_appends_write(monkeypatch, seed):
    """SpeckvKVConnector.append_tokens against a loop of SpeckvKVConnector.append on a recording library (host tensors stand in for
    device buffers): the same page numbers with the same page images per request, the same lengths and the same tails"""
    import torch
    st = _Stream()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: st)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(kv_connector, "_device_index", lambda v: torch.tensor(v, dtype=torch.int32))
    L, H, D, T, B, S = 2, 8, 128, 64, 5, 4
    ids = [11, 12, 13, 14, 15]
    a, b = SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8"), SpeckvKVConnector(_RecordingLib(), L, H, D, T, "fp8")
    for conn in (a, b):
        for rid in ids:
            conn.add_request(rid)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    keep = []
    for step in range(6):
        k = torch.randn((B, S, L, H, D), generator=gen).to(torch.float16)
        v = torch.randn((B, S, L, H, D), generator=gen).to(torch.float16)
        n_accept = [0, 1, 2, 3, S] if step == 0 else [int(x) for x in rng.integers(0, S + 1, B)]
        n_accept = n_accept[step % B:] + n_accept[:step % B]
        keep.append(a.append_tokens(ids, k, v, n_accept, stream=st))
        for t in range(S):                                                  # the same positions one at a time
            members = [i for i in range(B) if n_accept[i] > t]
            if members:
                idx = torch.tensor(members)
                keep.append(b.append([ids[i] for i in members], k[idx, t], v[idx, t], stream=st))
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
    with pytest.raises(ValueError):
        a.append_tokens(ids, k, v, [S + 1, 0, 0, 0, 0], stream=st)
    with pytest.raises(ValueError):
        a.append_tokens(ids, k, v, [1, 1], stream=st)
