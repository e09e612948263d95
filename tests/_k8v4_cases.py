"""The batches and the KV contents of the split pool's decode kernel (k_attend_k8v4, speckv_ext_attend_kv_batch) in the launch
geometries attend_geometry.hpp decides for BatchShape{fp8 = true}; shared by tests/test_k8v4_decode_geometry_cpu.py (the decisions and
the contents, no GPU) and tests/test_gpu_k8v4_decode_geometry.py (the kernel against float64).

regime(name, n_cus)   member lengths (positions), fixed seeds
assert_branch(...)    the engine's own decision (tests/_rules.py decide) reaches the regime's branch: relations, not numbers
content(seed, T, L)   K, V [L][T][H][D] fp16 whose MXFP4 block codes and FP8 page scales change from neighbour to neighbour
content_is_sharp(...) how sharp a content is in those two respects, and how broad its softmax stays

The decisions at 256 CUs (at 304 the same):
  E1  34 x 832                  9 tiles a piece, 3 pieces (9, 9, 8), order as given, splits-first: every member merged
  E2  (CUs / 2 + 1) x 1280      14 tiles a piece, 3 pieces (14, 14, 12): more workgroup columns (two a member) than CUs
  E3  16 x 128..512, member 7 at 2048, member 3 empty, member 5 two positions: by length, rows-first, 8 tiles a piece, 8 pieces at most
  E4  (CUs / 2 + 44) x 64..256  by length, one piece each, more members than a dispatch round: the serpentine order[], no merge
  E5  1 x 4094 (T = 4096)       one piece of 128 tiles, ragged last tile
Each shape is the smallest found that keeps its branch at both CU counts, smaller than first proposed where that held:
  E1  34 x 832 instead of 24 x 2048: 26 tiles is the first count that the rule prices above its floor of 8 tiles a piece AND cuts
      unevenly (13, 13, 13, 13, 12 of 64 tiles at 24 members is the same branch)
  E2  CUs / 2 + 1 members of 1280 positions instead of CUs + 4 of 4096: two columns a member make CUs + 2 columns, and 40 tiles is the
      first count the rule cuts at that many members
  E3  16 members with one of 2048 positions instead of 64 with four of 4096: one member of 8 pieces beside seven of two, seven of one
      and the empty one
  E4  CUs / 2 + 44 members instead of CUs + 44: a dispatch round is CUs / 2 members, so one full round and 44 of the reversed one
  E5  4094 positions instead of 4126: 128 tiles, the last one a page short"""
import functools

import numpy as np

from cxl_speckv_amd import kv_accuracy
from tests._rules import FP8, decide

H, D = 8, 128
REGIMES = ("E1", "E2", "E3", "E4", "E5")
G_OF = {"E1": (8,), "E2": (4,), "E3": (1, 8, 16), "E4": (8,), "E5": (8,)}          # query rows per kv head the GPU cases run
LAYERS_OF = {"E1": (0, 1), "E2": (1,), "E3": (0, 1), "E4": (1,), "E5": (1,)}
N_CONTENTS = 3


def regime(name, n_cus):
    """member lengths (positions, even) of a regime; the lengths that vary are fixed by a seed of their own"""
    rng = np.random.default_rng(8000 + REGIMES.index(name))
    if name == "E1":                              # equal lengths below the machine: pieces priced by the rule, uneven
        return np.full(34, 832)
    if name == "E2":                              # more workgroup columns than CUs
        return np.full(n_cus // 2 + 1, 1280)
    if name == "E3":                              # heavy tail: most 128..512, one at 2048, an empty member and a two-position one
        lens = rng.integers(64, 257, 16) * 2
        lens[7] = 2048
        lens[3], lens[5] = 0, 2
        return lens
    if name == "E4":                              # more members than a dispatch round, short
        return rng.integers(32, 129, n_cus // 2 + 44) * 2
    if name == "E5":                              # one long member, ragged last tile
        return np.array([4094])
    raise KeyError(name)


def layout_tokens(lens):
    """num_tokens of the layout a regime's allocations get: the longest member, up to a multiple of 32"""
    return max(32, -(-int(np.max(lens)) // 32) * 32)


def assert_branch(rules, name, lens, n_cus):
    """The case reaches its regime: what Engine::attend_batch_kv decides for these members (batch_form / batch_dispatch_order /
    batch_geometry / assign_pieces for BatchShape{fp8 = true}, single runs, default tuning).  Returns the decision."""
    lens = np.asarray(lens, np.int64)
    n, pages = len(lens), lens // 2
    tiles = (pages + 15) // 16
    tmax = int(tiles.max())
    d = decide(rules, FP8, "batch", pages, n_cus)
    assert d["fits"] == 1 and not d["table"] and not d["striped"] and d["round"] == n_cus // 2
    pieces = d["pieces"][:, 1].astype(np.int64)
    assert [int(x) for x in pieces] == [int(-(-t // d["tps"])) for t in tiles] and int(pieces.max()) == d["max_splits"]
    if name == "E1":                              # the rule's own pieces, not all of one length, every member merged
        assert d["by_length"] == 0 and d["rows_first"] == 0 and 1 < d["max_splits"] and tmax % d["max_splits"] != 0
        assert np.all(tiles == tmax) and np.all(pieces == d["max_splits"]) and 2 * n <= n_cus
    elif name == "E2":                            # more columns (two a member) than the 256 CUs the rule prices for, and than the machine has
        assert 2 * n > 256 and 2 * n > n_cus and d["tps"] < tmax and d["max_splits"] == -(-tmax // d["tps"])
        assert d["by_length"] == 0 and d["rows_first"] == 0
    elif name == "E3":                            # by length, rows first; members without a piece, with one, with the most
        assert d["by_length"] == 1 and d["rows_first"] == 1 and d["max_splits"] > 1
        assert (pieces == 0).any() and (pieces == 1).any() and (pieces == d["max_splits"]).any()
    elif name == "E4":                            # the serpentine: a first round longest first, a second one shortest first, no merge
        rnd = d["round"]
        assert d["by_length"] == 1 and n > rnd and d["max_splits"] == 1
        got = pages[d["order"]]
        assert sorted(int(x) for x in d["order"]) == list(range(n))
        assert np.all(np.diff(got[:rnd]) <= 0) and np.all(np.diff(got[rnd:2 * rnd]) >= 0) and got[0] > got[rnd - 1]
    elif name == "E5":                            # one long piece that ends inside a tile
        assert d["max_splits"] == 1 and d["tps"] >= 128 and tmax >= 128 and int(pages.max()) % 16 != 0
    else:
        raise KeyError(name)
    return d


# ----------------------------------------------------------------------------- contents
@functools.lru_cache(maxsize=None)
def content(seed, T, L=2):
    """K, V [L][T][H][D] fp16.  K: standard normal times ONE factor per (layer, page) out of U(0.5, 2) -- neighbouring FP8 page scales
    differ by a third.  V: standard normal times 2^e, e an integer of -4 .. 4 per (layer, page, head, block of 16 channels) -- neighbouring
    MXFP4 blocks, along the channels and along the pages, carry different E8M0 codes nine times in ten.  The layers differ.  Made once per (seed, T, L) and shared: read only."""
    assert T % 2 == 0
    rng = np.random.Generator(np.random.SFC64(seed))                            # (fp32 draws of a fast generator: the contents are most of a case's time)
    k = rng.standard_normal((L, T // 2, 2, H, D), dtype=np.float32)
    k *= rng.uniform(0.5, 2.0, (L, T // 2, 1, 1, 1)).astype(np.float32)
    e = rng.integers(-4, 5, (L, T // 2, 1, H, D // 16, 1))
    v = rng.standard_normal((L, T // 2, 2, H, D // 16, 16), dtype=np.float32)
    v *= np.exp2(e).astype(np.float32)
    k, v = k.reshape(L, T, H, D).astype(np.float16), v.reshape(L, T, H, D).astype(np.float16)
    k.setflags(write=False); v.setflags(write=False)
    return k, v


def content_is_sharp(k, v):
    """k, v [L][T][H][D] fp16 -> ((share of neighbouring (head, block) pairs of a page with the SAME E8M0 code, the same of neighbouring
    pages of a (head, block), the most distinct codes a layer holds), the median relative step |s' - s| / mean(s, s') between the FP8 scales
    max|k| / 448 of neighbouring pages, the median effective positions 1 / sum p^2 of standard-normal queries over the first 64
    positions of every (layer, head)).  Codes by kv_accuracy.mxfp4_codes, the rule quantize_mxfp4 scales with."""
    k, v = np.asarray(k), np.asarray(v)
    L = k.shape[0]
    along_blocks, along_pages, distinct, steps, eff = [], [], 0, [], []
    rng = np.random.default_rng(64)
    for layer in range(L):
        codes = kv_accuracy.mxfp4_codes(v[layer]).reshape(-1, H, D // 16)          # [page][head][block]
        along_blocks.append((codes[:, :, 1:] == codes[:, :, :-1]).mean())
        along_pages.append((codes[1:] == codes[:-1]).mean())
        distinct = max(distinct, len(np.unique(codes)))
        s = np.abs(k[layer].astype(np.float64)).reshape(-1, 2 * H * D).max(axis=1) / 448.0
        steps.append(np.abs(np.diff(s)) / ((s[1:] + s[:-1]) / 2))
        q = rng.standard_normal((H, 16, D))
        sc = np.einsum("hgd,thd->hgt", q, k[layer, :64].astype(np.float64)) / np.sqrt(D)
        p = np.exp(sc - sc.max(axis=2, keepdims=True))
        p /= p.sum(axis=2, keepdims=True)
        eff.append(1.0 / (p * p).sum(axis=2).reshape(-1))
    return ((float(np.mean(along_blocks)), float(np.mean(along_pages)), int(distinct)), float(np.median(np.concatenate(steps))),
            float(np.median(np.concatenate(eff))))


def case_contents(name, T):
    """the N_CONTENTS contents of a regime's GPU case, [(k, v)] of [2][T][H][D] each; E5 has one member and one content"""
    return [content(8100 + 10 * REGIMES.index(name) + c, T) for c in range(1 if name == "E5" else N_CONTENTS)]


def case_queries(name, n, g):
    """the members' own query rows [n][H][g][D] fp16, standard normal"""
    return np.random.default_rng(8200 + 20 * REGIMES.index(name) + g).standard_normal((n, H, g, D)).astype(np.float16)


def mixed_contents(T):
    """the two contents of the mixed-layout case's connector of num_tokens T"""
    return [content(8300 + T // 256 * 10 + c, T) for c in range(2)]


def bound_content():
    """the 64 written positions of the 2048-piece case"""
    return content(8400, 64)
