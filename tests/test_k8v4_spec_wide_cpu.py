"""Not -m gpu: the split pool's multi-position step with 32 query rows per pass -- spec_groups(S, R, 32), the declaration of
speckv_ext_attend_kv_spec_wide and its answer on an engine without a device, and what SpeckvSplitKVConnector.attend_spec(rows_per_pass=...)
hands the library (against a recording library)."""
import os

import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import speckv_ctypes
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests.test_k8v4_cpu import _ctypes_of, _declared
from tests.test_k8v4_spec_cpu import ROW, _connector, _step
from tests.test_paged_io_cpu import _cpu_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "speckv_ext_attend_kv_spec_wide"


@pytest.mark.parametrize("S,R,want", [(4, 8, [(0, 4)]), (3, 8, [(0, 3)]), (9, 2, [(0, 9)]), (16, 2, [(0, 16)]), (5, 8, [(0, 4), (4, 1)]), (8, 4, [(0, 8)]),
                                      (16, 1, [(0, 16)]), (7, 5, [(0, 6), (6, 1)])])
def test_spec_groups_at_32_rows_per_pass(S, R, want):
    assert SpeckvKVConnector.spec_groups(S, R, 32) == want
    per = 16 // R
    assert SpeckvKVConnector.spec_groups(S, R) == SpeckvKVConnector.spec_groups(S, R, 16) == [(j0, min(per, S - j0)) for j0 in range(0, S, per)]
    for bad in (0, 8, 17, 64):
        with pytest.raises(ValueError):
            SpeckvKVConnector.spec_groups(S, R, bad)


def test_the_entry_is_declared_bound_and_answers_on_the_null_engine():
    """the argument list of speckv_ext_attend_kv_spec_window; a good set is SPECKV_ERR_DRIVER there (no data path), g <= 16, g > 32 and one
    row per position are SPECKV_ERR_INVAL before anything else, as are the sibling's refusals"""
    header = open(os.path.join(ROOT, "include", "speckv_ext.h")).read()
    mine = _declared(header, ENTRY)
    assert mine == _declared(header, "speckv_ext_attend_kv_spec_window") and _ctypes_of(mine) == speckv_ctypes._EXT_SIGNATURES[ENTRY]
    lib = pkg.SpeckvLib(pkg.build_library(), "/dev/null")
    try:
        h, buf = lib.alloc(64 * 4096), np.zeros(8 * 1024 + 16, dtype=np.float16)
        at = buf.ctypes.data + (-buf.ctypes.data) % 16

        def call(**change):
            args = dict(k_handles=[h], v_handles=[h], layer=0, d_q_f16=at, g=32, rows_per_pos=8, pos_end=[32], length=[33], d_depth=at, window=20, d_k_held=at,
                        d_v_held=at, seq_stride_elems=5 * ROW, pos_stride_elems=ROW, d_mask=at, mask_stride=4, sm_scale=0.1, d_out=at, d_lse=None, stream=1)
            args.update(change)
            with pytest.raises(SpeckvError) as e:
                lib.attend_kv_spec_wide(**args)
            return e.value.status
        for good in (dict(), dict(window=0, length=None, d_depth=0), dict(g=24), dict(g=18, rows_per_pos=2, mask_stride=9), dict(g=32, rows_per_pos=2, mask_stride=16)):
            assert call(**good) == -2, good                                          # SPECKV_ERR_DRIVER
        for bad in (dict(g=16), dict(g=8), dict(g=33, rows_per_pos=1, mask_stride=33), dict(g=24, rows_per_pos=1, mask_stride=24), dict(g=40, mask_stride=5),
                    dict(g=30), dict(mask_stride=3), dict(d_mask=0), dict(d_depth=0), dict(length=[35]), dict(pos_stride_elems=ROW + 4)):
            assert call(**bad) == -4, bad                                            # SPECKV_ERR_INVAL
        assert not buf.any()
    finally:
        lib.finalize()


@pytest.mark.parametrize("S,R,window", [(4, 8, None), (5, 8, None), (9, 2, 40), (16, 1, None)])
def test_attend_spec_sends_wide_groups_to_the_wide_entry(monkeypatch, S, R, window):
    """rows_per_pass=32: a group of more than 16 rows is one attend_kv_spec_wide call, a last or only group of 16 rows or fewer one call of
    the 16-row entry, nothing else; each reads the mask table (and the depth table) from its first position on.  rows_per_pass=16 and no
    argument: today's calls.  Any other value is a ValueError before any library call."""
    torch, st = _cpu_torch(monkeypatch)
    (lib, conn), rids = _connector(torch, (0, 1, 38, 97)), [10, 11, 12, 13]
    q, k_new, v_new = _step(torch, 4, S, R)
    conn.attend_spec(1, rids, q, k_new, v_new, 0.125, stream=st, window=window, rows_per_pass=32)
    groups, narrow = SpeckvKVConnector.spec_groups(S, R, 32), "attend_kv_spec_window" if window else "attend_kv_spec"
    assert [c[0] for c in lib.calls] == ["attend_kv_spec_wide" if n * R > 16 else narrow for _, n in groups]
    for (j0, n), call in zip(groups, lib.calls):
        if call[0] == "attend_kv_spec_wide":      # (recorded positionally: ..., g, rows_per_pos, pos_end, length, d_depth, window, d_k, d_v, strides, d_mask, mask_stride)
            assert call[5:7] == (n * R, R) and [int(x) for x in call[8]] == [0, 1, 38, 97] and call[10] == (window or 0) and call[15:17] == (lib.calls[0][15] + 4 * j0, S)
            assert (call[9] != 0) == bool(window)
    for how in (dict(), dict(rows_per_pass=16)):
        del lib.calls[:]
        conn.attend_spec(1, rids, q, k_new, v_new, 0.125, stream=st, window=window, **how)
        assert [c[0] for c in lib.calls] == [narrow] * len(SpeckvKVConnector.spec_groups(S, R))
    del lib.calls[:]
    for bad in (0, 8, 24, 64, None):
        with pytest.raises(ValueError):
            conn.attend_spec(1, rids, q, k_new, v_new, 0.125, stream=st, rows_per_pass=bad)
    assert lib.calls == []
