"""The launch decision of the attention entries, asked of the engine's own functions (csrc/attend_geometry.hpp through the wrappers of
tests/csrc/host_rules_test.cpp): decide() walks them in the order Engine::attend_batch / attend_batch_plan + attend_planned do, decide_seq() asks what
the single-sequence entries (qk_scores_fp8, attend_fp8 / _int4 / _mx4) ask."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8, INT4, MX4 = 4, 3, 5
P, I = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
DEFAULT_TUNING = (0, 0, 0, 0, 0)           # attend_tiles_per_split, attend_order_as_given, attend_fp8_table_regs, attend_fp8_striped_table, attend_int4_striped_wg
ORDER_AS_GIVEN = (0, 1, 0, 0, 0)           # no dispatch order and no pieces on account of the lengths: what is left is the rule for equal lengths


def load_rules():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "csrc")])
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libhostrules_test.so"))
    lib.rules_batch_form.restype = None
    lib.rules_batch_form.argtypes = [P, I, P]
    lib.rules_batch_dispatch_order.restype = C.c_int
    lib.rules_batch_dispatch_order.argtypes = [P, I, P, P]
    lib.rules_plan_tiles_bound.restype = C.c_uint32
    lib.rules_plan_tiles_bound.argtypes = [C.c_uint32, C.c_uint32]
    lib.rules_batch_geometry.restype = C.c_uint64
    lib.rules_batch_geometry.argtypes = [C.c_uint32, P, I, P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, P, P]
    lib.rules_stream_begin.restype = C.c_uint64
    lib.rules_stream_begin.argtypes = [C.c_uint32] * 3
    lib.rules_stream_wg_of.restype = C.c_uint32
    lib.rules_stream_wg_of.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    lib.rules_stream_count.restype = C.c_uint32
    lib.rules_stream_count.argtypes = [C.c_uint32] * 4
    lib.rules_int4_wg8_stream.restype = None
    lib.rules_int4_wg8_stream.argtypes = [C.c_uint32] * 4 + [C.c_int32] * 2 + [P]
    lib.rules_mx4_stream.restype = None
    lib.rules_mx4_stream.argtypes = [C.c_uint32] * 6 + [C.c_int32] * 2 + [P]
    lib.rules_striped_tiles.restype = C.c_uint32
    lib.rules_striped_tiles.argtypes = [C.c_uint32] * 2
    lib.rules_int4_wg8_splits.restype = C.c_uint32
    lib.rules_int4_wg8_splits.argtypes = [C.c_uint32] * 3
    lib.rules_seq_decide.restype = C.c_uint64
    lib.rules_seq_decide.argtypes = [P, I, P]
    return lib


def _p(a):
    return a.ctypes.data_as(P)


def striped_tiles(pages, stripe_n):
    """ring_rule.hpp mx4_striped_tiles (rules_striped_tiles is the engine's own): the tiles of a member counted by residue class of the page index"""
    n = np.maximum(np.asarray(stripe_n, np.int64), 1)
    pages = np.asarray(pages, np.int64)
    return np.where(pages > 0, n * (((pages + n - 1) // n + 15) // 16), 0)


def decide(lib, scheme, entry, pages, n_cus, heads=8, stripe_n=1, any_table=False, tuning=DEFAULT_TUNING, kept=None, max_pos_end=None):
    """What the entry ("batch" or "plan": attend_batch_plan followed by attend_planned) decides for members of `pages` pages each, every one in stripe_n
    runs (1: a single run), the first without a regular placement if any_table.  kept = (max_splits, rows_first) of the shape's first plan."""
    pages = np.ascontiguousarray(pages, np.uint32)
    n = len(pages)
    shape = np.array([scheme == FP8, scheme == MX4, n, heads, n_cus, stripe_n != 1 or any_table, any_table], np.uint32)
    tun = np.array(tuning, np.int32)
    form = np.zeros(7, np.uint32)
    lib.rules_batch_form(_p(shape), tun.ctypes.data_as(I), _p(form))
    d = dict(zip(("table", "striped", "fp8_cls", "int4_cls", "by_class", "wg8", "round"), (int(v) for v in form)))
    tiles = np.ascontiguousarray(striped_tiles(pages, stripe_n) if d["by_class"] else (pages.astype(np.int64) + 15) // 16, np.uint32)
    order = np.zeros(n, np.uint32)
    d["by_length"] = lib.rules_batch_dispatch_order(_p(shape), tun.ctypes.data_as(I), _p(pages), _p(order))
    d["order"] = order if d["by_length"] else None
    plan = entry != "batch"
    bound = 0
    if plan:
        max_pos_end = int(pages.max()) * 2 if max_pos_end is None else max_pos_end
        bound = lib.rules_plan_tiles_bound(max_pos_end, stripe_n if d["by_class"] else 0)
    out = np.zeros(8, np.uint32)
    pieces = np.zeros(3 * n, np.uint32)
    k = (-1, 0) if kept is None else (int(kept[0]), int(kept[1]))
    d["parts"] = lib.rules_batch_geometry(1 if plan else 0, _p(shape), tun.ctypes.data_as(I), _p(tiles), bound, d["by_length"], k[0], k[1], _p(out), _p(pieces))
    d.update(zip(("tps", "piece_tps", "max_splits", "rows_first", "unequal", "rule_tps", "rule_splits", "fits"), (int(v) for v in out)))
    d["pieces"] = pieces.reshape(n, 3)
    if plan:                                   # the launch: attend_planned asks with the plan's room and no lengths
        launch = np.zeros(8, np.uint32)
        lib.rules_batch_geometry(1, _p(shape), tun.ctypes.data_as(I), None, bound, 0, d["max_splits"], d["rows_first"], _p(launch), None)
        assert (launch[0], launch[2], launch[3]) == (d["tps"], d["max_splits"], d["rows_first"]), "attend_planned disagrees with its plan"
    return d


# ---- several layers of ONE sequence: the stream decision of Engine::attend_int4 / attend_mx4 (attend_geometry.hpp int4_wg8_stream / mx4_stream)
def _stream(out):
    return None if out[0] == 0 else dict(zip(("n_wgs", "len", "rem", "max_slots", "tiles"), (int(v) for v in out)))


def int4_stream(lib, n_layers, n_tiles, n_cus, cls=False, attend_splits=0, attend_stream=0):
    """What Engine::attend_int4 decides for n_layers x n_tiles tiles on the whole-record kernel (n_tiles by residue class where cls):
    None = the fixed grid, else the AttendArgs::stream fields."""
    out = np.zeros(5, np.uint32)
    lib.rules_int4_wg8_stream(n_layers, n_tiles, n_cus, int(cls), attend_splits, attend_stream, _p(out))
    return _stream(out)


def mx4_stream(lib, n_layers, n_pages, n_cus, g=8, fixed_splits=None, attend_splits=0, attend_stream=0):
    """The same of Engine::attend_mx4 for records in one run.  fixed_splits = the splits its fixed grid would take: None = what the entry's own decision
    gives (decide_seq; its stream must then be this one), a number = the rule alone under that count."""
    d = None
    if fixed_splits is None:
        d = decide_seq(lib, MX4, n_layers, n_pages, n_cus, g=g, tuning=dict(attend_splits=attend_splits, attend_stream=attend_stream))
        fixed_splits = d["n_splits"]
    out = np.zeros(5, np.uint32)
    lib.rules_mx4_stream(n_layers, (n_pages + 15) // 16, n_pages, n_cus, (g + 7) // 8, fixed_splits, attend_splits, attend_stream, _p(out))
    assert d is None or d["stream"] == _stream(out), "Engine::attend_mx4's decision disagrees with mx4_stream"
    return _stream(out)


# ---- ONE sequence: the launch decision of Engine::qk_scores_fp8 / attend_fp8 / attend_int4 / attend_mx4 (attend_geometry.hpp seq_decide)
SEQ_TUNING_KEYS = ("attend_general", "attend_splits", "attend_stream", "attend_fp8_table_regs", "attend_fp8_striped_table", "attend_int4_striped_wg", "attend_fp8_dma")
SEQ_PLACES = ("none", "linear", "striped", "table")
FP8_KERNELS = ("-", "dma<2>", "linear<CLS>", "dma<1>", "dma<0>", "linear<false>", "linear<true>", "linear<false, true>", "k_attend_fp8")
SEQ_FIELDS = ("place", "cls", "wg8", "n_tiles", "n_splits", "tiles_per_split", "stream_len", "stream_rem", "stream_n_wgs", "stream_max_slots", "stream_tiles",
              "slots", "direct_out", "rows_final", "zero_page", "quantize_q", "fp8_kernel")


def decide_seq(lib, scheme, n_layers, n_pages, n_cus, g=8, heads=8, num_tokens=None, pos_begin=0, skip_pages=0, has_tab=True, one_run=True, stripe_n=None,
               scores=False, tuning=None):
    """What the single-sequence entry of `scheme` (scores: qk_scores_fp8) decides for n_pages pages from pos_begin on -- the range AS ATTENDED: FP8 over a
    scale table starts at the table's tile, skip_pages masked pages in front of the caller's begin.  num_tokens: the layout's positions per layer (None: the
    range's tiles, whole); the allocation has a scale table / its records in one run / stripe_n runs (None: 1 with one_run, else 0 = no regular
    placement).  tuning: a dict of tuning keys, or their 7 values in the order of SEQ_TUNING_KEYS.  Returns the SeqDecision fields (SEQ_FIELDS, place and
    fp8_kernel as numbers: SEQ_PLACES, FP8_KERNELS), "parts", and "stream" as int4_stream / mx4_stream return it."""
    if num_tokens is None:
        num_tokens = pos_begin + (n_pages + 15) // 16 * 32
    if stripe_n is None:
        stripe_n = 1 if one_run else 0
    tun = [int(tuning.get(k, 0)) for k in SEQ_TUNING_KEYS] if isinstance(tuning, dict) else list(tuning or [0] * 7)
    assert len(tun) == 7 and (not isinstance(tuning, dict) or set(tuning) <= set(SEQ_TUNING_KEYS))
    shape = np.array([scheme == FP8, scheme == MX4, scores, n_layers, heads, g, n_cus, num_tokens, pos_begin, n_pages, skip_pages, has_tab, one_run, stripe_n], np.uint32)
    out = np.zeros(17, np.uint32)
    parts = lib.rules_seq_decide(_p(shape), np.array(tun, np.int32).ctypes.data_as(I), _p(out))
    d = dict(zip(SEQ_FIELDS, (int(v) for v in out)))
    d["parts"] = int(parts)
    d["stream"] = _stream([d["stream_n_wgs"], d["stream_len"], d["stream_rem"], d["stream_max_slots"], d["stream_tiles"]])
    return d
