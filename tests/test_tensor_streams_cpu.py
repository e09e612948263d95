"""The hand-made streams of tests/_tensor_streams.py, without a GPU: the oracle equals a second, plain numpy statement of the
decoder on exactly the (stream, mode, capacity) inputs the GPU tests use, and every case still has the property it was built
for -- so that no case silently stops reaching the path it is meant for."""
import os
import re

import numpy as np
import pytest

from tests import _tensor_streams as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cxl-speckv_amd", "csrc")
VOCAB = ts.vocabulary()


def _define(text, name):
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_geometry_constants_are_the_sources():
    dev = open(os.path.join(CSRC, "tensor_codec_device.hpp")).read()
    dec = open(os.path.join(CSRC, "tensor_decompress.hip")).read()
    assert int(re.search(r"constexpr uint32_t kTile = (\d+);", dev).group(1)) == ts.CHUNK_PAIRS == ts.TILE_ELEMS
    assert int(re.search(r"constexpr uint32_t kTdfWin = (\d+);", dec).group(1)) == ts.WINDOW_ELEMS
    lb = _define(dev, "SPECKV_TDF_LB_WAVE")
    assert _define(dec, "SPECKV_TDF_WAVES") - lb == ts.WG_CHUNKS_SINGLE
    assert _define(dev, "SPECKV_TDM_WAVES") - lb == ts.WG_CHUNKS_BATCH
    assert "const uint64_t i = p0 + 512u * j + 8u * lane;" in dec and (ts.STEP_PAIRS, ts.LANE_PAIRS) == (512, 8)
    assert "end -= 64u;" in dec and ts.LOOK_BACK_WORDS == 64
    # the choice between the two decoder families, quoted below as a condition on the input
    assert "const bool few_pairs = n_pairs * 51u < std::min<uint64_t>(dst_cap, n_pairs * 255u) * 50u;" in dec


@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_equals_the_plain_restatement(oracle, mode):
    """The whole vocabulary x every clip point: oracle.decompress_f32(..., cap=) equals decode_plain bit for bit."""
    seen = 0
    for s in VOCAB:
        total = ts.total_of(s.data)
        for label, cap in ts.clip_points(s):
            got = oracle.decompress_f32(s.data, 0.125, mode, cap=cap)
            want = ts.decode_plain(s.data, 0.125, mode, cap)
            assert got.size == min(total, cap) == want.size, (s.name, label, cap)
            assert got.tobytes() == want.tobytes(), (s.name, label, cap)
            seen += 1
    assert seen > 10 * len(VOCAB)


@pytest.mark.parametrize("scale", [0.0, -0.5, 2.0 ** -140, 1e-7, 1000.0, 3e38, float("inf"), float("nan")])
def test_oracle_equals_the_plain_restatement_over_scales(oracle, scale):
    """... and under the scales the GPU tests use (subnormal, overflowing and non-finite outputs): NaNs where the other has NaNs,
    the same bits everywhere else."""
    for name in ("long_zero_pair2048", "ones_2049"):
        s = ts.by_name(name)
        for mode in (0, 1):
            got = oracle.decompress_f32(s.data, scale, mode)
            want = ts.decode_plain(s.data, scale, mode, ts.total_of(s.data))
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (name, mode)
            assert got.view(np.uint32)[~nan].tobytes() == want.view(np.uint32)[~nan].tobytes(), (name, mode)


def test_decode_plain_known_answers():
    """decode_plain by hand: the odd tail is dropped, a zero count emits nothing, counts are uint8, the sum wraps as int8."""
    y = ts.decode_plain(np.array([5, 3, 7], np.uint8), 1.0, 1, 10)
    assert y.tolist() == [5.0, 10.0, 15.0]
    y = ts.decode_plain(np.array([5, 0, 9, 2], np.uint8), 0.5, 1, 10)
    assert y.tolist() == [4.5, 9.0]
    y = ts.decode_plain(np.array([100, 2, 255, 200], np.uint8), 1.0, 1, 4)         # 100, 200 -> -56, then -1 per element, cut at 4
    assert y.tolist() == [100.0, -56.0, -57.0, -58.0]
    y = ts.decode_plain(np.array([127, 1], np.uint8), 2.0, 0, 1)                   # REF_EXACT: 127 / 127 * 2
    assert y.tolist() == [2.0] and y.dtype == np.float32
    assert ts.decode_plain(np.array([1], np.uint8), 1.0, 0, 5).size == 0


def test_vocabulary_holds_every_case_it_was_built_for():
    names = {s.name for s in VOCAB}
    pairs_of = {s.name: s.data.size // 2 for s in VOCAB}
    # pair counts: around a lane, a chunk, a batched workgroup, a single-stream workgroup
    for kind in ("ones", "long", "set", "mixed"):
        assert {pairs_of[f"{kind}_{p}"] for p in ts.PAIR_COUNTS_SMALL} == {1, 7, 8, 9, 2047, 2048, 2049}
    assert set(ts.PAIR_COUNTS_WG) == {ts.WG_CHUNKS_BATCH * 2048, ts.WG_CHUNKS_BATCH * 2048 + 1, ts.WG_CHUNKS_SINGLE * 2048, ts.WG_CHUNKS_SINGLE * 2048 + 1}
    for p in ts.PAIR_COUNTS_WG:
        assert f"ones_{p}" in names and f"mixed_{p}" in names
    assert f"long_{ts.WG_CHUNKS_BATCH * 2048 + 1}" in names and f"long_{ts.WG_CHUNKS_SINGLE * 2048 + 1}" in names
    # an odd trailing byte in half of the cases, and the totals inside the limit
    odd = sum(s.data.size % 2 for s in VOCAB)
    assert abs(2 * odd - len(VOCAB)) <= 1
    for s in VOCAB:
        assert ts.total_of(s.data) <= ts.MAX_TOTAL, s.name
        c = ts.counts_of(s.data)
        if s.kind == "long" and "zero" not in s.name:
            assert c.min() >= 200
        if s.kind == "ones" and "zero" not in s.name:
            assert (c == 1).all()
        if s.kind == "set":
            assert set(c.tolist()) <= set(ts.COUNT_SET)
        if s.kind == "mixed" and c.size >= 100 and s.name != "deep_0_and_1":
            assert 0.2 < (c == 0).mean() < 0.4 and set(c.tolist()) <= set(ts.COUNT_SET) | {0}
    assert any(s.data.size // 2 > ts.FULL_CROSS_PAIRS for s in VOCAB) and sum(s.data.size // 2 <= ts.FULL_CROSS_PAIRS for s in VOCAB) >= 40
    # zero-count placements, each with its property, on a base of ones (one pass by the library's choice) and of long counts
    for base in ("ones", "long"):
        for where, idx in ts.ZERO_PLACEMENTS.items():
            c = ts.counts_of(ts.by_name(f"{base}_zero_{where}").data)
            assert c.size == ts.PLACEMENT_PAIRS and (c[idx] == 0).all() and (np.delete(c, idx) != 0).all(), (base, where)
        tot = ts.chunk_totals(ts.by_name(f"{base}_zero_chunk1").data)
        assert tot[1] == 0 and tot[0] > 0 and tot[2] > 0                          # two chunks share a start: the tie of the 64-ary search
        assert ts.chunk_totals(ts.by_name(f"{base}_zero_last_chunk").data)[-1] == 0
        assert ts.chunk_totals(ts.by_name(f"{base}_zero_one_lane").data).min() > 0
    lane = ts.ZERO_PLACEMENTS["one_lane"]
    assert len(lane) == 8 and lane[0] % 8 == 0 and lane[0] // 512 == lane[-1] // 512
    assert ts.ZERO_PLACEMENTS["pair511"][0] // 512 != ts.ZERO_PLACEMENTS["pair512"][0] // 512
    assert ts.ZERO_PLACEMENTS["pair2047"][0] // 2048 != ts.ZERO_PLACEMENTS["pair2048"][0] // 2048
    z = ts.by_name("zeros_only")
    assert ts.total_of(z.data) == 0 and z.data.size // 2 > 2048
    # a zero count in a chunk that spans several windows (the one-pass kernel's pair-by-pair path under long counts)
    lz = ts.by_name("long_zero_pair512")
    assert ts.chunk_totals(lz.data)[0] > 4 * ts.WINDOW_ELEMS and ts.counts_of(lz.data)[:2048].min() == 0
    # the deep stream: zero counts present, more workgroups than one look-back window of status words
    d = ts.by_name("deep_0_and_1")
    dc = ts.counts_of(d.data)
    assert set(dc.tolist()) == {0, 1}
    chunks = (dc.size + 2047) // 2048
    assert (chunks + ts.WG_CHUNKS_SINGLE - 1) // ts.WG_CHUNKS_SINGLE > ts.LOOK_BACK_WORDS + 1
    assert (ts.chunk_totals(d.data) > 0).all() and dc.reshape(-1)[:chunks // 2 * 2048].reshape(-1, 2048).min(axis=1).max() == 0     # a zero count in every chunk


def test_clip_points_cut_what_they_say():
    labels = {}
    for s in VOCAB:
        tot = ts.chunk_totals(s.data)
        starts = np.concatenate([[0], np.cumsum(tot)])
        total = int(starts[-1])
        counts = ts.counts_of(s.data).astype(np.int64)
        pts = ts.clip_points(s)
        caps = [cap for _, cap in pts]
        assert caps == sorted(set(caps)) and caps[0] == 0
        by_label = {}
        for label, cap in pts:
            for l in label.split("|"):
                by_label[l] = cap
                labels.setdefault(l, []).append(s.name)
        assert by_label["zero"] == 0 and by_label["one"] == 1 and by_label["total"] == total and by_label["total+5"] == total + 5
        assert by_label["far_above"] == 4 * total + 64
        if total:
            assert by_label["total-1"] == total - 1
        for k in (1, 2):
            if f"chunk{k}_start" in by_label:
                assert by_label[f"chunk{k}_start"] == starts[k]
        if "chunk_start-1" in by_label:
            assert by_label["chunk_start-1"] + 1 in starts[1:-1].tolist() + [starts[max(1, tot.size // 2)]]
            assert by_label["chunk_start+1"] - by_label["chunk_start-1"] == 2
        if "window_edge" in by_label:
            e = by_label["window_edge"]
            k = int(np.searchsorted(starts, e, side="right")) - 1
            assert e - starts[k] == ts.WINDOW_ELEMS and tot[k] > ts.WINDOW_ELEMS + 3       # strictly inside a chunk of more than one window
            assert by_label["window_edge-3"] == e - 3 and by_label["window_edge+3"] == e + 3
        if "tile_edge" in by_label:
            e = by_label["tile_edge"]
            assert e % ts.TILE_ELEMS == 0 and 0 < e < total and by_label["tile_edge-1"] == e - 1 and by_label["tile_edge+1"] == e + 1
        for l in ("behind_zero_count", "in_zero_count_chunk"):
            if l in by_label:
                cap = by_label[l]
                k = int(np.searchsorted(starts, cap - 1, side="right")) - 1              # the chunk of the last element that is kept
                assert starts[k] < cap <= starts[k + 1] and counts[2048 * k:2048 * (k + 1)].min() == 0, (s.name, l)
    # every kind of clip exists somewhere; the ones tied to structure exist on the streams built for them
    for l in ("zero", "one", "total-1", "total", "total+5", "chunk1_start", "chunk2_start", "chunk_start-1", "chunk_start+1", "window_edge-3",
              "window_edge", "window_edge+3", "tile_edge-1", "tile_edge", "tile_edge+1", "behind_zero_count", "in_zero_count_chunk", "far_above"):
        assert labels.get(l), l
    assert "long_zero_pair512" in labels["behind_zero_count"] and "long_zero_pair512" in labels["window_edge"]
    assert "ones_zero_pair2048" in labels["in_zero_count_chunk"] and "deep_0_and_1" in labels["in_zero_count_chunk"]
    assert any(n.startswith("long_") for n in labels["chunk2_start"]) and any(n.startswith("ones_") for n in labels["chunk2_start"])


def test_cases_meet_the_input_condition_of_their_decoder_family():
    """launch_tensor_decompress takes the one-pass kernel when NOT few_pairs, i.e. when pairs * 51 >= min(cap, pairs * 255) * 50:
    the condition is quoted from there and held against the cases that are meant for a family by the library's own choice."""
    n = {"one_pass": 0, "by_output": 0}
    for s in VOCAB:
        pairs = s.data.size // 2
        for label, cap in ts.clip_points(s):
            meant = ts.meant_family(s, cap)
            if meant is None:
                continue
            one_pass = pairs * 51 >= min(cap, pairs * 255) * 50
            assert one_pass == (meant == "one_pass"), (s.name, label, cap, meant)
            n[meant] += 1
    assert n["one_pass"] >= 100 and n["by_output"] >= 50, n
    # the zero-count placements are met by BOTH families without a switch: on ones by the one-pass kernel, on long counts by output
    for where in ts.ZERO_PLACEMENTS:
        o, l = ts.by_name(f"ones_zero_{where}"), ts.by_name(f"long_zero_{where}")
        assert ts.meant_family(o, ts.total_of(o.data)) == "one_pass" and ts.meant_family(l, ts.total_of(l.data)) == "by_output"
