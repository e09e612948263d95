"""-m gpu: what the split pool's DECODE route (speckv_ext_attend_kv_batch through SpeckvSplitKVConnector.attend: FP8 keys, MXFP4 values,
the query quantised to E4M3 x a row scale by the kernel) costs in attention accuracy on KV-like data (kv_accuracy.kv_split_decode_accuracy),
against float64 attention over the original rows with the fp16 query.

Bars: the decode regime's relative L2 error <= 0.25 -- the project's bar for a pool denser than FP8; the numpy restatement of this route
(format_accuracy_cpu(query="e4m3")) stands at 0.2162 / 0.1895 for the two seeds.  Peaky and flat <= 1.25 x that restatement for the same
seed and regime -- the project's margin of a quarter over the numpy restatement, not over the code under test.  The launch's own share
(kernel_rel_l2: against float64 over the dequantised values WITH the E4M3-restated query, so the query's share is not counted twice) <=
0.01 in every regime."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd import kv_accuracy
from tests._gpu import torch_mod

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [7001, 7002])
def test_the_decode_route_meets_the_bar(seed):
    torch_mod()
    cpu = kv_accuracy.format_accuracy_cpu("fp8_e4m3", "mxfp4", seed=seed, query="e4m3")
    lib = pkg.SpeckvLib(pkg.library_path(), "hip:0")
    try:
        acc = kv_accuracy.kv_split_decode_accuracy(lib, seed=seed)
    finally:
        lib.finalize()
    for r in kv_accuracy.REGIMES:
        m = acc[r]
        print(f"k8v4 decode seed {seed} {r}: rel_l2 {m['rel_l2']:.4f} (format {m['format_rel_l2']:.4f}, kernel {m['kernel_rel_l2']:.5f}), "
              f"cpu restatement with the e4m3 query {cpu[r]:.4f}, top-1 {m['top1_agreement']:.3f}")
    assert set(acc) == set(kv_accuracy.REGIMES)
    for r in kv_accuracy.REGIMES:
        assert np.isfinite(acc[r]["rel_l2"]) and acc[r]["kernel_rel_l2"] <= 0.01, (r, acc[r])
    assert acc["decode"]["rel_l2"] <= 0.25, acc["decode"]
    for r in ("peaky", "flat"):
        assert acc[r]["rel_l2"] <= 1.25 * cpu[r], (r, acc[r]["rel_l2"], cpu[r])
