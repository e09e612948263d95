"""-m gpu: the whole-tensor decoder (speckv_ext_codec_decompress_tensor / _decompress_tensors) over streams it did not produce --
the hand-made vocabulary of tests/_tensor_streams.py -- in every launch form, at rooms that clip the stream where its structure
makes that interesting, bit for bit against oracle.decompress_f32 with the same capacity (tests/test_tensor_streams_cpu.py ties
that to a second, plain statement on the same inputs).  Every case also checks the element count the decoder reports,
min(total, room), and that nothing behind the room (nor between the stream's end and the room's) was written.

The single-tensor cross product (stream x clip point x output type x mode x form) is run in full; only the runs with the stream off
its 16-byte alignment leave out the streams of more than FULL_CROSS_PAIRS pairs."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import _tensor_streams as ts
from tests._gpu import assert_same_float_bits, load_raw_lib, set_tuning, stream_ptr, torch_mod

pytestmark = pytest.mark.gpu

SCALE = 0.125
FORMS = {
    "default": {},
    "one_pass": {"td_one_pass": 1},                                              # k_td_fused whatever the stream
    "by_output": {"tc_multipass": 1},                                            # k_td_summary, the two-grid scan, k_td_expand_scatter
    "by_output_per_element": {"tc_multipass": 1, "td_expand_per_element": 1},    # ... k_td_expand
    "by_output_scan_wg": {"tc_multipass": 1, "tc_scan": 1},                      # ... k_td_scan_wg
    "by_output_scan_serial": {"tc_multipass": 1, "tc_scan": 2},                  # ... k_td_scan
}
SWITCHES = ("td_one_pass", "tc_multipass", "td_expand_per_element", "tc_scan", "tc_batch_one_wg")
TYPE_MODE = [(True, 0), (False, 1), (True, 1), (False, 0)]                        # (fp32 out, quantiser mode)
PAD = 64                                                                         # elements behind the room that must stay untouched


@contextlib.contextmanager
def launch_form(switches):
    try:
        for k, v in switches.items():
            set_tuning(k, v)
        yield
    finally:
        for k in SWITCHES:
            set_tuning(k, 0)


@pytest.fixture(scope="module")
def lib():
    return load_raw_lib()


class Expectations:
    """Per (stream, mode): the oracle's full decode on the device as fp32 and fp16 bits, and per clip point the element count of
    oracle.decompress_f32(..., cap=) -- whose output is held against the full decode's prefix once, here.  Shared by every test."""

    def __init__(self, oracle):
        self.oracle, self.by_key, self.streams, self.scratch = oracle, {}, {}, {}

    def of(self, s, mode):
        key = (s.name, mode)
        if key not in self.by_key:
            torch = torch_mod()
            full = self.oracle.decompress_f32(s.data, SCALE, mode)
            assert full.size == ts.total_of(s.data)
            counts = {}
            for label, cap in ts.clip_points(s):
                y = self.oracle.decompress_f32(s.data, SCALE, mode, cap=cap)
                assert y.size == min(full.size, cap) and y.tobytes() == full[:y.size].tobytes(), (s.name, label)
                counts[cap] = y.size
            d32 = torch.from_numpy(full.view(np.int32)).cuda()
            d16 = torch.from_numpy(full.astype(np.float16).view(np.int16)).cuda()
            self.by_key[key] = (d32, d16, counts)
        return self.by_key[key]

    def device_stream(self, s, shift):
        """the stream's bytes on the device, `shift` bytes behind a 16-byte boundary"""
        key = (s.name, shift)
        if key not in self.streams:
            torch = torch_mod()
            buf = torch.from_numpy(np.concatenate([np.full(shift, 0xEE, np.uint8), s.data, np.full(32, 0xEE, np.uint8)])).cuda()
            assert buf.data_ptr() % 16 == 0
            self.streams[key] = buf
        return self.streams[key], self.streams[key].data_ptr() + shift

    def workspace(self, lib, rle_bytes):
        torch = torch_mod()
        ws_bytes = lib.speckv_ext_codec_tensor_decode_workspace_bytes(rle_bytes)
        if self.scratch.get("bytes", -1) < ws_bytes:
            self.scratch = {"bytes": ws_bytes, "buf": torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")}
        return (self.scratch["buf"].data_ptr() + 255) & ~255, ws_bytes


@pytest.fixture(scope="module")
def expect(oracle):
    return Expectations(oracle)


def decode_case(lib, expect, s, cap, mode, out_f32, shift=0):
    """One launch of the single-tensor entry; returns None, or what was wrong."""
    torch = torch_mod()
    d32, d16, counts = expect.of(s, mode)
    n = counts[cap]
    _, rle_ptr = expect.device_stream(s, shift)
    ws_ptr, ws_bytes = expect.workspace(lib, s.data.size)
    d_y = torch.full((cap + PAD,), -1, dtype=torch.int32 if out_f32 else torch.int16, device="cuda")      # 0xFF..: a NaN pattern
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    rc = lib.speckv_ext_codec_decompress_tensor(rle_ptr, s.data.size, SCALE, d_y.data_ptr(), cap, int(out_f32), d_n.data_ptr(),
                                                ws_ptr, ws_bytes, mode, stream_ptr())
    assert rc == 0, rc
    want = (d32 if out_f32 else d16)[:n]
    wrong = (d_y[:n] != want).any() | (d_y[n:] != -1).any() | (d_n[0] != n)
    if not bool(wrong):
        return None
    what = []
    if int(d_n[0]) != n:
        what.append(f"n_out {int(d_n[0])} != {n}")
    bad = torch.nonzero(d_y[:n] != want)
    if bad.numel():
        what.append(f"{bad.numel()} elements differ, first at {int(bad[0])}")
    behind = torch.nonzero(d_y[n:] != -1)
    if behind.numel():
        what.append(f"{behind.numel()} elements written behind the last, first at {n + int(behind[0])} (room {cap})")
    return ", ".join(what)


def single_tensor_cases(small_only=False):
    """(stream, label, cap, out_f32, mode): the full cross; small_only: streams of at most FULL_CROSS_PAIRS pairs"""
    for s in ts.vocabulary():
        if small_only and s.data.size // 2 > ts.FULL_CROSS_PAIRS:
            continue
        for label, cap in ts.clip_points(s):
            for out_f32, mode in TYPE_MODE:
                yield s, label, cap, out_f32, mode


def run_single_tensor_cases(lib, expect, form, shift=0, small_only=False):
    failures, n_cases = [], 0
    with launch_form(FORMS[form]):
        for s, label, cap, out_f32, mode in single_tensor_cases(small_only):
            n_cases += 1
            wrong = decode_case(lib, expect, s, cap, mode, out_f32, shift)
            if wrong:
                failures.append(f"{s.name} clip {label}={cap} {'fp32' if out_f32 else 'fp16'} mode {mode}: {wrong}")
    assert n_cases > 2000
    assert not failures, f"{form}: {len(failures)} of {n_cases} cases failed, " \
                         f"{len([f for f in failures if 'n_out' in f])} on n_out; first: {failures[:6]}"


@pytest.mark.parametrize("form", list(FORMS))
def test_single_tensor_entry_over_the_vocabulary(lib, expect, form):
    """vocabulary x {fp32, fp16 out} x mode x clip points through speckv_ext_codec_decompress_tensor in one launch form."""
    run_single_tensor_cases(lib, expect, form)


@pytest.mark.parametrize("shift", [2, 6])
@pytest.mark.parametrize("form", ["default", "one_pass"])
def test_stream_pointer_off_its_16_byte_alignment(lib, expect, form, shift):
    """The decoder accepts a stream pointer that is 2-byte aligned (include/speckv_ext.h): off a 16-byte boundary every load of
    td_load_pairs, k_td_summary and k_td_expand_scatter takes the narrow branch, which aligned streams reach only for the last
    partial group of 8 pairs."""
    run_single_tensor_cases(lib, expect, form, shift=shift, small_only=True)


def test_single_tensor_entry_refuses_an_odd_stream_pointer(lib, expect):
    s = ts.by_name("ones_2049")
    _, rle_ptr = expect.device_stream(s, 2)
    ws_ptr, ws_bytes = expect.workspace(lib, s.data.size)
    d_y = torch_mod().zeros(64, dtype=torch_mod().float32, device="cuda")
    rc = lib.speckv_ext_codec_decompress_tensor(rle_ptr + 1, s.data.size, SCALE, d_y.data_ptr(), 8, 1, None, ws_ptr, ws_bytes, 0, stream_ptr())
    assert rc != 0


SCALES = [0.0, -0.5, 2.0 ** -140, 1e-7, 1000.0, 3e38, float("inf"), float("nan")]


@pytest.mark.parametrize("form", ["one_pass", "by_output"])
def test_scales_table_conversion_equals_per_element_conversion(lib, oracle, expect, form):
    """The one-pass kernels convert through a 512-entry table per tensor, their zero-count chunks and the by-output chain element by
    element: both equal the oracle where outputs are fp32 / fp16 subnormals, overflow fp16 or fp32, are negative, zero, infinite
    or NaN (NaN payloads excepted).  long_zero_pair2048 has a zero count in chunk 1 only: its other chunks take the table."""
    torch = torch_mod()
    with launch_form(FORMS[form]):
        for name in ("long_zero_pair2048", "ones_2049"):
            s = ts.by_name(name)
            total = ts.total_of(s.data)
            _, rle_ptr = expect.device_stream(s, 0)
            ws_ptr, ws_bytes = expect.workspace(lib, s.data.size)
            for scale in SCALES:
                for mode in (0, 1):
                    for out_f32, cap in ((True, total + 5), (False, total + 5), (True, total // 2 + 3), (False, total // 2 + 3)):
                        want = oracle.decompress_f32(s.data, scale, mode, cap=cap)
                        if not out_f32:
                            with np.errstate(over="ignore"):
                                want = want.astype(np.float16)
                        d_y = torch.full((cap + PAD,), -1, dtype=torch.int32 if out_f32 else torch.int16, device="cuda")
                        d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                        rc = lib.speckv_ext_codec_decompress_tensor(rle_ptr, s.data.size, float(scale), d_y.data_ptr(), cap, int(out_f32),
                                                                    d_n.data_ptr(), ws_ptr, ws_bytes, mode, stream_ptr())
                        assert rc == 0, rc
                        torch.cuda.synchronize()
                        what = f"{form} {name} scale {scale!r} mode {mode} {'fp32' if out_f32 else 'fp16'} cap {cap}"
                        assert int(d_n[0]) == want.size == min(total, cap), what
                        y = d_y.cpu().numpy()
                        assert (y[want.size:] == -1).all(), what
                        assert_same_float_bits(y[:want.size].view(np.float32 if out_f32 else np.float16), want, what)


# ---- many streams per launch (speckv_ext_codec_decompress_tensors) ----
def gpu_decode_tensors(lib, streams, scales, rooms, max_elems, mode, out_f32, with_n_out, rle_offset):
    """Decode only: streams[i] (uint8 arrays) under scales[i] into a room of rooms[i] elements, in ONE launch.  Streams lie `rle_offset`
    bytes behind 16-byte boundaries; outputs are 16-byte aligned, filled with 0xFF and followed by guard bytes, which are checked
    here.  Returns ([room bytes of every output, as uint8], n_out or None)."""
    torch = torch_mod()
    lib.speckv_ext_codec_tensors_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64]; lib.speckv_ext_codec_tensors_workspace_bytes.restype = C.c_size_t
    lib.speckv_ext_codec_decompress_tensors.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nt = len(streams)
    osz = 4 if out_f32 else 2
    assert all(r <= max_elems for r in rooms) and all(s.size <= 2 * max_elems for s in streams)          # the header's contract
    ws_bytes = lib.speckv_ext_codec_tensors_workspace_bytes(nt, max_elems)
    d_ws = torch.full((ws_bytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")                        # (dirty: the call clears what it uses)
    ws_ptr = (d_ws.data_ptr() + 255) & ~255
    rle_off, out_off = [], []
    ro = oo = 0
    for s, room in zip(streams, rooms):
        ro = (ro + 15) // 16 * 16 + rle_offset; rle_off.append(ro); ro += s.size + 16
        oo = (oo + 15) // 16 * 16; out_off.append(oo); oo += room * osz + 32
    h_rle = np.full(ro + 16, 0xEE, np.uint8)
    for s, o in zip(streams, rle_off):
        h_rle[o:o + s.size] = s
    d_rle = torch.from_numpy(h_rle).cuda()
    d_out = torch.full((oo + 16,), 0xFF, dtype=torch.uint8, device="cuda")                              # (0xFFFF / 0xFFFFFFFF: NaN patterns)
    assert d_rle.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    desc = np.zeros((nt, 4), np.uint64)
    for i, (s, room) in enumerate(zip(streams, rooms)):
        desc[i] = (d_out.data_ptr() + out_off[i], room, d_rle.data_ptr() + rle_off[i], s.size)
    d_desc = torch.from_numpy(desc.view(np.int64)).cuda()
    d_bytes = torch.from_numpy(np.array([s.size for s in streams], np.int64)).cuda()
    d_scales = torch.from_numpy(np.asarray(scales, np.float32)).cuda()
    d_nout = torch.full((nt,), -1, dtype=torch.int64, device="cuda") if with_n_out else None
    rc = lib.speckv_ext_codec_decompress_tensors(nt, d_desc.data_ptr(), max_elems, d_bytes.data_ptr(), d_scales.data_ptr(), int(out_f32),
                                                 d_nout.data_ptr() if with_n_out else None, ws_ptr, ws_bytes, mode, stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    outs = []
    for i, room in enumerate(rooms):
        outs.append(out[out_off[i]:out_off[i] + room * osz])
        assert (out[out_off[i] + room * osz:out_off[i] + room * osz + 32] == 0xFF).all(), f"stream {i}: something was written behind its room of {room}"
    return outs, (d_nout.cpu().numpy() if with_n_out else None)


BATCH_ROOM = 600_000            # rooms up to here: every clip point; up to BATCH_ROOM_MAX: the totals and the zero-count clips only
BATCH_ROOM_MAX = 1_500_000


def batch_entries(max_elems=None):
    """(stream, label, room) of one ragged batch: every vocabulary stream beside itself at rooms equal to its clip points (0 beside
    non-empty streams among them), and streams of 0 and 1 bytes.  max_elems: only what fits a launch with that bound."""
    entries = []
    for s in ts.vocabulary():
        for label, cap in ts.clip_points(s):
            labels = label.split("|")
            if cap <= BATCH_ROOM or (cap <= BATCH_ROOM_MAX and any(l in ("total", "behind_zero_count", "in_zero_count_chunk") for l in labels)):
                entries.append((s, label, cap))
    for nbytes in (0, 1):
        s = ts.Stream(f"bytes{nbytes}", "zeros", np.full(nbytes, 0x07, np.uint8))
        entries += [(s, "zero", 0), (s, "room", 5), (s, "room", 4099)]
    if max_elems is not None:
        entries = [(s, label, room) for s, label, room in entries if room <= max_elems and s.data.size <= 2 * max_elems]
    return entries


@pytest.mark.parametrize("form", ["one_wg_by_size", "one_wg_forced", "several_wgs"])
def test_batched_entry_over_ragged_batches(lib, oracle, form):
    """speckv_ext_codec_decompress_tensors over the vocabulary in ONE launch -- k_tdb_fused (one workgroup per stream: because
    max_elems fits a workgroup, or forced) and k_tdm_fused (several workgroups per stream, most streams using fewer than the launch
    gives them, the deep stream more than one look-back window of them) -- with rooms that clip, rooms of 0 beside non-empty
    streams, streams of 0 and 1 bytes, streams off their 16-byte alignment, and once per form without d_n_out."""
    one_wg = ts.WG_CHUNKS_BATCH * ts.CHUNK_PAIRS
    entries = batch_entries(one_wg if form == "one_wg_by_size" else None)
    max_elems = max(max(room for _, _, room in entries), max((s.data.size + 1) // 2 for s, _, _ in entries))
    wpt = (max_elems + one_wg - 1) // one_wg
    assert len(entries) > 300 and ((wpt == 1) if form == "one_wg_by_size" else (wpt >= 3))
    if form == "several_wgs":
        assert wpt > ts.LOOK_BACK_WORDS + 1 and sum((s.data.size // 2 + one_wg - 1) // one_wg < wpt for s, _, _ in entries) > 300
    assert any(room == 0 and s.data.size > 2 for s, _, room in entries) and any(s.data.size == 1 and room for s, _, room in entries)
    streams = [s.data for s, _, _ in entries]
    rooms = [room for _, _, room in entries]
    scales = [SCALE] * len(entries)
    full = {}
    failures = []
    with launch_form({"tc_batch_one_wg": 1} if form == "one_wg_forced" else {}):
        for mode, out_f32, with_n_out, rle_offset in ((0, True, True, 0), (1, False, True, 2), (1, True, False, 6), (0, False, False, 0)):
            outs, n_out = gpu_decode_tensors(lib, streams, scales, rooms, max_elems, mode, out_f32, with_n_out, rle_offset)
            for i, (s, label, room) in enumerate(entries):
                if (s.name, mode) not in full:                                          # (the entries of a stream follow each other)
                    full = {(s.name, mode): oracle.decompress_f32(s.data, SCALE, mode, cap=max(r for t, _, r in entries if t.name == s.name))}
                want = full[(s.name, mode)][:room]
                what = f"{s.name} room {label}={room} mode {mode} {'fp32' if out_f32 else 'fp16'} n_out {with_n_out} offset {rle_offset}"
                assert want.size == min(ts.total_of(s.data), room), what
                if with_n_out and n_out[i] != want.size:
                    failures.append(f"{what}: n_out {n_out[i]} != {want.size}")
                y = outs[i].view(np.float32 if out_f32 else np.float16)
                if not (outs[i][want.size * y.itemsize:] == 0xFF).all():
                    failures.append(f"{what}: written between the stream's end and the room's")
                if y[:want.size].tobytes() != (want if out_f32 else want.astype(np.float16)).tobytes():
                    failures.append(f"{what}: elements differ")
    assert not failures, f"{form}: {len(failures)} failures over {4 * len(entries)} streams, " \
                         f"{len([f for f in failures if 'n_out ' in f.split(': ', 1)[1]])} on n_out; first: {failures[:6]}"
