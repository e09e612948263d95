"""Hand-made run-length streams for the whole-tensor decoder (cxl-speckv_amd/csrc/tensor_decompress.hip), a plain numpy
restatement of what a stream decodes to, and the capacities at which a stream's structure makes a clipped decode interesting.
Pure numpy, no GPU: tests/test_tensor_streams_cpu.py ties the oracle to decode_plain on exactly these inputs and asserts that
every case still has the property it was built for; tests/test_gpu_tensor_decode_streams.py runs them through every launch form.

A stream is [value u8][count u8]...: the pairs expand to an int8 delta chain whose running sum (mod 256) is q; an odd trailing
byte is dropped, a zero count emits nothing, the output is clipped at the buffer (cache_engine.cpp:84-116, 241-281)."""
import functools
from collections import namedtuple

import numpy as np

# ---- the decoder's geometry (tensor_codec_device.hpp, tensor_decompress.hip; test_tensor_streams_cpu.py reads them back from there)
CHUNK_PAIRS = 2048        # kTile: pairs per chunk, one wave
STEP_PAIRS = 512          # pairs per scan step of a chunk
LANE_PAIRS = 8            # pairs per lane and step (one 16-byte load)
WINDOW_ELEMS = 4096       # kTdfWin: elements per window of the one-pass kernels
WG_CHUNKS_SINGLE = 16     # kTdfChunks: chunks per workgroup of k_td_fused (SPECKV_TDF_WAVES - SPECKV_TDF_LB_WAVE)
WG_CHUNKS_BATCH = 8       # kTdmChunks: chunks per workgroup of k_tdb_fused / k_tdm_fused (SPECKV_TDM_WAVES - SPECKV_TDF_LB_WAVE)
TILE_ELEMS = 2048         # output elements per wave of the by-output chain (k_td_expand_scatter)
LOOK_BACK_WORDS = 64      # status words a look-back reads at a time
MAX_TOTAL = 8 * 1024 * 1024
FULL_CROSS_PAIRS = 20000  # streams of at most this many pairs are small enough for the full cross of forms, types and clips

Stream = namedtuple("Stream", "name kind data")     # kind: the count structure ("ones", "long", "set", "mixed", "zeros")
COUNT_SET = (1, 2, 3, 127, 128, 254, 255)


def _seed(name):
    return [ord(c) for c in name]


def _counts(kind, pairs, rng, zero_share=0.3):
    if kind == "ones":
        return np.ones(pairs, np.uint8)
    if kind == "long":
        return rng.integers(200, 256, pairs).astype(np.uint8)
    if kind == "set":
        return rng.choice(np.array(COUNT_SET, np.uint8), pairs)
    if kind == "mixed":
        c = rng.choice(np.array(COUNT_SET, np.uint8), pairs)
        c[rng.random(pairs) < zero_share] = 0
        return c
    if kind == "zeros":
        return np.zeros(pairs, np.uint8)
    raise ValueError(kind)


def _make(name, kind, counts, rng, odd):
    pairs = counts.size
    data = np.empty(2 * pairs + (1 if odd else 0), np.uint8)
    data[0:2 * pairs:2] = rng.integers(0, 256, pairs).astype(np.uint8)
    data[1:2 * pairs:2] = counts
    if odd:
        data[-1] = 0x5B                                             # the odd trailing byte: a value without a count, dropped
    return Stream(name, kind, data)


PAIR_COUNTS_SMALL = (1, 7, 8, 9, CHUNK_PAIRS - 1, CHUNK_PAIRS, CHUNK_PAIRS + 1)
PAIR_COUNTS_WG = (WG_CHUNKS_BATCH * CHUNK_PAIRS, WG_CHUNKS_BATCH * CHUNK_PAIRS + 1,
                  WG_CHUNKS_SINGLE * CHUNK_PAIRS, WG_CHUNKS_SINGLE * CHUNK_PAIRS + 1)
DEEP_PAIRS = (LOOK_BACK_WORDS + 1) * WG_CHUNKS_SINGLE * CHUNK_PAIRS + 5      # look-back more than one window of words deep
PLACEMENT_PAIRS = 3 * CHUNK_PAIRS + 77
# zero-count placements: name -> pair indices (of a stream of PLACEMENT_PAIRS pairs) whose count becomes 0
ZERO_PLACEMENTS = {
    "pair0": [0],
    "last_pair": [PLACEMENT_PAIRS - 1],
    "pair511": [STEP_PAIRS - 1],                                    # both sides of a step edge
    "pair512": [STEP_PAIRS],
    "pair2047": [CHUNK_PAIRS - 1],                                  # both sides of a chunk edge; 2047: the pair k_td_expand_scatter reads in front of chunk 1
    "pair2048": [CHUNK_PAIRS],
    "one_lane": list(range(CHUNK_PAIRS + STEP_PAIRS + 13 * LANE_PAIRS, CHUNK_PAIRS + STEP_PAIRS + 14 * LANE_PAIRS)),
    "chunk1": list(range(CHUNK_PAIRS, 2 * CHUNK_PAIRS)),            # a chunk of total 0: chunks 1 and 2 share a start (the tie of the 64-ary search)
    "last_chunk": list(range(3 * CHUNK_PAIRS, PLACEMENT_PAIRS)),
}


@functools.lru_cache(maxsize=1)
def vocabulary():
    """Every stream of the vocabulary, deterministic: [Stream(name, kind, data u8[])].  Half of them end in an odd byte."""
    out = []

    def add(name, kind, counts):
        rng = np.random.default_rng(_seed(name))
        out.append(_make(name, kind, counts, rng, odd=len(out) % 2 == 1))

    for pairs in PAIR_COUNTS_SMALL:
        for kind in ("ones", "long", "set", "mixed"):
            add(f"{kind}_{pairs}", kind, _counts(kind, pairs, np.random.default_rng(_seed(f"c{kind}{pairs}"))))
    for pairs in PAIR_COUNTS_WG:
        for kind in ("ones", "long", "mixed"):
            if kind == "long" and pairs in (WG_CHUNKS_BATCH * CHUNK_PAIRS, WG_CHUNKS_SINGLE * CHUNK_PAIRS):
                continue                                            # (one long-count stream per workgroup size: they are the expensive ones)
            add(f"{kind}_{pairs}", kind, _counts(kind, pairs, np.random.default_rng(_seed(f"c{kind}{pairs}"))))
    for base in ("ones", "long"):
        for where, idx in ZERO_PLACEMENTS.items():
            c = _counts(base, PLACEMENT_PAIRS, np.random.default_rng(_seed(f"z{base}{where}")))
            c[idx] = 0
            add(f"{base}_zero_{where}", base, c)
    add("zeros_only", "zeros", _counts("zeros", PLACEMENT_PAIRS, None))
    rng = np.random.default_rng(_seed("deep"))
    add("deep_0_and_1", "mixed", (rng.random(DEEP_PAIRS) < 0.5).astype(np.uint8))
    assert len({s.name for s in out}) == len(out)
    return out


def by_name(name):
    return next(s for s in vocabulary() if s.name == name)


def counts_of(data):
    data = np.asarray(data, np.uint8)
    return data[1:2 * (data.size // 2):2]


def chunk_totals(data):
    """elements each chunk of CHUNK_PAIRS pairs emits"""
    c = counts_of(data).astype(np.int64)
    n_chunks = (c.size + CHUNK_PAIRS - 1) // CHUNK_PAIRS
    padded = np.zeros(n_chunks * CHUNK_PAIRS, np.int64)
    padded[:c.size] = c
    return padded.reshape(n_chunks, CHUNK_PAIRS).sum(axis=1)


def total_of(data):
    return int(counts_of(data).astype(np.int64).sum())


@functools.lru_cache(maxsize=4)
def _q_of(stream_bytes):
    data = np.frombuffer(stream_bytes, np.uint8)
    pairs = data.size // 2                                          # an odd trailing byte is dropped
    values = data[0:2 * pairs:2]                                    # int8 deltas, kept as their bytes: the sum is taken modulo 256
    counts = data[1:2 * pairs:2]                                    # uint8; a zero count emits nothing
    deltas = np.repeat(values, counts)
    return np.cumsum(deltas, dtype=np.uint8).view(np.int8)          # the running sum modulo 256, read as int8


def decode_plain(stream, scale, mode, cap):
    """What the stream decodes to, in numpy: q = int8(cumsum(repeat(int8(value), count)) mod 256), then
    mode 0 (REF_EXACT, the reference's: cache_engine.cpp:278-281): (fp32(q) / fp32(127)) * scale, each operation rounded to fp32;
    mode 1 (INTENT): fp32(q) * scale;   cut at `cap` elements."""
    q = _q_of(np.ascontiguousarray(stream, np.uint8).tobytes())[:cap]
    f = q.astype(np.float32)
    s = np.float32(scale)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if mode == 0:
            return (f / np.float32(127)) * s
        return f * s


def clip_points(stream):
    """Capacities read off the stream's structure: [(label, cap)], every cap once (the labels of equal caps joined by "|")."""
    data = stream.data if isinstance(stream, Stream) else np.asarray(stream, np.uint8)
    counts = counts_of(data).astype(np.int64)
    tot = chunk_totals(data)
    starts = np.concatenate([[0], np.cumsum(tot)]).astype(np.int64)          # first element of chunk k; starts[-1] = total
    total = int(starts[-1])
    pts = [("zero", 0), ("one", 1), ("total-1", total - 1), ("total", total), ("total+5", total + 5)]
    for k in (1, 2):                                                # every later chunk has start >= end
        if k < tot.size:
            pts.append((f"chunk{k}_start", int(starts[k])))
    if tot.size >= 2:
        k = max(1, tot.size // 2)
        pts += [("chunk_start-1", int(starts[k]) - 1), ("chunk_start+1", int(starts[k]) + 1)]
    wide = np.flatnonzero(tot > WINDOW_ELEMS + 3)                   # a window edge inside a chunk of long counts
    if wide.size:
        k = int(wide[wide >= 1][0]) if (wide >= 1).any() else int(wide[0])
        e = int(starts[k]) + WINDOW_ELEMS
        pts += [("window_edge-3", e - 3), ("window_edge", e), ("window_edge+3", e + 3)]
    if total > TILE_ELEMS + 1:                                      # an output-tile edge of the by-output chain
        e = TILE_ELEMS * max(1, total // TILE_ELEMS // 2)
        pts += [("tile_edge-1", e - 1), ("tile_edge", e), ("tile_edge+1", e + 1)]
    zc = np.flatnonzero((counts == 0) & (np.repeat(tot, CHUNK_PAIRS)[:counts.size] > 0))      # zero counts in chunks that emit something
    if zc.size:
        i = int(zc[0])
        k = i // CHUNK_PAIRS
        before = int(counts[:i].sum())
        if before + 1 < starts[k + 1]:
            pts.append(("behind_zero_count", before + 1))           # one element behind where the zero count sits
        pts.append(("in_zero_count_chunk", int(starts[k]) + int(tot[k]) // 2 + 1))
    pts.append(("far_above", 4 * total + 64))
    merged = {}
    for label, cap in pts:
        if cap >= 0:
            merged.setdefault(cap, []).append(label)
    return [("|".join(labels), cap) for cap, labels in sorted(merged.items())]


def meant_family(stream, cap):
    """The decoder family a (stream, capacity) case is MEANT to reach by the library's own choice, or None where the case makes no
    claim: streams of ones that fill a chunk, at a capacity near their total -> "one_pass"; streams of long counts at a capacity
    at or above their total -> "by_output".  test_tensor_streams_cpu.py holds the input condition of launch_tensor_decompress
    against this."""
    pairs = stream.data.size // 2
    total = total_of(stream.data)
    if stream.kind == "ones" and pairs >= CHUNK_PAIRS - 1 and 1 <= cap <= total + 5:
        return "one_pass"
    if stream.kind == "long" and pairs >= LANE_PAIRS and cap >= total - 1:
        return "by_output"
    return None
