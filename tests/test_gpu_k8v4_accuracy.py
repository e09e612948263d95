"""-m gpu: what the split pool ("K8V4": FP8 keys, MXFP4 values) costs in attention accuracy on KV-like data, end to end through
SpeckvSplitKVConnector (kv_accuracy.kv_split_accuracy), against float64 attention over the original rows.

Bars: the decode regime's relative L2 error <= 0.25 -- the review's bar for a pool denser than FP8 (the 4-bit pools stand at 0.57-0.75
there); peaky and flat <= 1.25 x what kv_accuracy.format_accuracy_cpu gives for the same seed and regime -- the project's margin of a
quarter over the numpy restatement of the formats, not over the code under test; and the launch's own share (kernel_rel_l2: against
float64 over the dequantised values) <= 0.01 in every regime -- the query is not quantised on this route, and the fp16-query kernels'
own share stands below 0.0003 in DESIGN's table."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_accuracy
from tests._gpu import torch_mod

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [7001, 7002])
def test_the_split_pool_meets_the_bar(seed):
    torch_mod()
    cpu = kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed)
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        acc = kv_accuracy.kv_split_accuracy(lib, seed=seed)
    finally:
        lib.finalize()
    for r in kv_accuracy.REGIMES:
        m = acc[r]
        print(f"k8v4 seed {seed} {r}: rel_l2 {m['rel_l2']:.4f} (format {m['format_rel_l2']:.4f} + kernel {m['kernel_rel_l2']:.5f}), "
              f"cpu restatement {cpu[r]:.4f}, top-1 {m['top1_agreement']:.3f}")
    assert set(acc) == set(kv_accuracy.REGIMES)
    for r in kv_accuracy.REGIMES:
        assert np.isfinite(acc[r]["rel_l2"]) and acc[r]["kernel_rel_l2"] <= 0.01, (r, acc[r])
    assert acc["decode"]["rel_l2"] <= 0.25, acc["decode"]
    for r in ("peaky", "flat"):
        assert acc[r]["rel_l2"] <= 1.25 * cpu[r], (r, acc[r]["rel_l2"], cpu[r])
