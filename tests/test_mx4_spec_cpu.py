"""Not -m gpu: SpeckvKVConnector.attend_spec(row_block=16) on an MXFP4 pool against the recording stand-in library of
tests/test_fp8_spec_window_cpu.py -- one speckv_ext_attend_spec_mx4 call per group and layer and nothing else, today's calls unchanged by
default and at row_block=None, and the ValueErrors of the argument."""
import pytest

from tests._gpu import D, H
from tests.test_fp8_spec_window_cpu import PTR, _calls
from tests.test_k8v4_spec_cpu import _step
from tests.test_paged_io_cpu import _cpu_torch


def test_the_row_block_argument(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    monkeypatch.setattr(torch, "zeros", lambda *a, device=None, _zeros=torch.zeros, **k: _zeros(*a, **k))      # (the plan buffer of the planned route)
    step = _step(torch, 4, 3, 8)                                             # S = 3 at 8 rows per position: groups of 16 and 8 rows
    for scheme, how, names in (("fp8", dict(row_block=16), "MXFP4"), ("int4", dict(row_block=16), "MXFP4"), ("mxfp4", dict(row_block=8), "MXFP4"),
                               ("mxfp4", dict(row_block=32), "MXFP4"), ("mxfp4", dict(row_block=16, window=33), r"attend_chunk\(window=W\)"),
                               ("mxfp4", dict(row_block=16, rows_per_pass=32), "rows_per_pass")):
        with pytest.raises(ValueError, match=names):
            _calls(torch, scheme, st, *step, 1, **how)
    today = _calls(torch, "mxfp4", st, *step, 1)
    assert [c[0] for c in today] == ["attend_plan_bytes", "attend_batch_plan"] + ["attend_planned", "attend_fold_held"] * 2
    assert _calls(torch, "mxfp4", st, *step, 1, row_block=None) == today
    # (handles, layer, q, g, rows_per_pos, pos_end, k_held, v_held, seq stride, pos stride, mask words of the group's first position, mask stride, sm, out, lse, stream)
    assert _calls(torch, "mxfp4", st, *step, 1, row_block=16) == [
        ("attend_spec_mx4", [0, 0, 0, 0], 1, PTR, 16, 8, [0, 0, 36, 36], PTR, PTR, 4 * H * D, H * D, PTR, 3, 0.125, PTR, 0, 7),
        ("attend_spec_mx4", [0, 0, 0, 0], 1, PTR, 8, 8, [0, 0, 36, 36], PTR, PTR, 4 * H * D, H * D, PTR, 3, 0.125, PTR, 0, 7)]
    assert [c[:3] for c in _calls(torch, "mxfp4", st, *step, 2, parents=[-1, 0, 0], n_new=[3, 0, 2, 1], row_block=16)] == [("attend_spec_mx4", [0, 0, 0, 0], 2)] * 2
    # attend_spec_layers over layers 1 and 2: every group layer by layer
    assert _calls(torch, "mxfp4", st, *step, 1, n_layers=2, row_block=16) == [
        ("attend_spec_mx4", [0, 0, 0, 0], layer, PTR, g, 8, [0, 0, 36, 36], PTR, PTR, 4 * H * D, H * D, PTR, 3, 0.125, PTR, 0, 7)
        for g in (16, 8) for layer in (1, 2)]
