"""Not -m gpu: SpeckvKVConnector.attend_spec(rows_per_pass=32) on an FP8 pool against the recording stand-in library of
tests/test_fp8_spec_window_cpu.py -- one speckv_ext_attend_spec_wide call per wide group and layer, today's calls for a trailing group,
today's calls unchanged at 16 and by default, and the ValueErrors of the argument."""
import pytest

from tests._gpu import D, H
from tests.test_fp8_spec_window_cpu import PTR, T, _calls
from tests.test_k8v4_spec_cpu import _step
from tests.test_paged_io_cpu import _cpu_torch

POS_END, LENGTHS = [0, 0, 36, 36], [0, 1, 37, 36]


@pytest.mark.parametrize("window", [0, 33])
def test_the_rows_per_pass_argument(monkeypatch, window):
    torch, st = _cpu_torch(monkeypatch)
    monkeypatch.setattr(torch, "zeros", lambda *a, device=None, _zeros=torch.zeros, **k: _zeros(*a, **k))      # (the plan buffer of the planned route)
    step, how = _step(torch, 4, 5, 8), dict(window=window)                 # S = 5 at 8 rows per position: [32, 8] rows at 32 per pass, [16, 16, 8] at 16
    for scheme, bad in (("int4", 32), ("mxfp4", 32), ("fp8", 8), ("fp8", 64)):
        with pytest.raises(ValueError, match="rows_per_pass"):
            _calls(torch, scheme, st, *step, 1, rows_per_pass=bad)
    today = _calls(torch, "fp8", st, *step, 1, **how)
    assert [c[0] for c in today] == (["attend_spec_window"] * 3 if window else ["attend_plan_bytes", "attend_batch_plan"] + ["attend_planned", "attend_fold_held"] * 3)
    assert _calls(torch, "fp8", st, *step, 1, rows_per_pass=16, **how) == today
    wide, *trailing = _calls(torch, "fp8", st, *step, 1, rows_per_pass=32, **how)
    assert wide == ("attend_spec_wide", [0, 0, 0, 0], 1, PTR, 32, 8, POS_END, LENGTHS, PTR, window, PTR, PTR, 6 * H * D, H * D, PTR, 5, 0.125, PTR, 0, 7)
    if window:                                                               # the trailing position: today's call of a sliding-window layer
        assert trailing == [today[2]]
    else:                                                                    # ... of a global layer: the plan, the planned call, the fold by mask words
        assert [c[0] for c in trailing] == ["attend_plan_bytes", "attend_batch_plan", "attend_planned", "attend_fold_masked"]
        assert trailing[:3] == today[:2] + [today[6]] and trailing[3][:5] + trailing[3][11:13] == ("attend_fold_masked", 4, 0, H, 8, PTR, 5)
    one, = _calls(torch, "fp8", st, *_step(torch, 4, 4, 8), 1, rows_per_pass=32, **how)          # S = 4: one wide group and nothing else
    assert one[:6] == ("attend_spec_wide", [0, 0, 0, 0], 1, PTR, 32, 8) and one[9] == window
    # a tree with a ragged n_new: the calls of the chain (the tree and the live counts travel in the mask words alone)
    step16 = lambda name, layer: (name, [0, 0, 0, 0], layer, PTR, 8, 8, POS_END, LENGTHS, PTR, 33, PTR, PTR, 6 * H * D, H * D, PTR, 5, 0.125, PTR, 0, 7)
    plan = [("attend_plan_bytes", 4), ("attend_batch_plan", [0, 0, 0, 0], POS_END, T, 0, 0, 7)]
    assert _calls(torch, "fp8", st, *step, 1, rows_per_pass=32, parents=[-1, 0, 1, 0, 3], n_new=[5, 0, 2, 4], **how) == [wide] + (
        [step16("attend_spec_window", 1)] if window else
        plan + [("attend_planned", 4, 0, 4, 1, PTR, 8, T, 0.125, PTR, PTR, 7),
                ("attend_fold_masked", 4, 0, H, 8, 8, PTR, PTR, PTR, 6 * H * D, H * D, PTR, 5, 0.125, PTR, PTR, 7)])
    # attend_spec_layers over layers 1 and 2: the wide group layer by layer, then the trailing group -- layer by layer under a window, ONE
    # planned call and ONE fold over both layers on a global layer
    assert _calls(torch, "fp8", st, *step, 1, n_layers=2, rows_per_pass=32, **how) == [wide, wide[:2] + (2,) + wide[3:]] + (
        [step16("attend_spec_window", 1), step16("attend_spec_window", 2)] if window else
        plan + [("attend_planned_layers", 4, 0, 4, 1, 2, PTR, 8, T, 0.125, PTR, PTR, 7),
                ("attend_fold_masked", 8, 0, H, 8, 8, PTR, PTR, PTR, 6 * H * D, H * D, PTR, 5, 0.125, PTR, PTR, 7)])
