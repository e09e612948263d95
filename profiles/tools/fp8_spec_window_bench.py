#!/usr/bin/env python3
"""What a draft step on a SLIDING-WINDOW layer costs on the decode kernel over an FP8 pool (writes profiles/fp8_spec_window.txt): the
measurement of profiles/tools/k8v4_spec_window_bench.py -- its shapes, steps, routes, method and options, see there -- with
SpeckvKVConnector(scheme="fp8") in the place of the split connector.
  route a  SpeckvKVConnector.attend_spec(window=W): ONE speckv_ext_attend_spec_window (k_attend_fp8_spec; S x rows_per_pos = 16: one group)
  route b  SpeckvKVConnector.attend_chunk(window=W, splits=0) with the same step: the only route on a local layer before
  route c  SpeckvKVConnector.attend_spec without a window (the planned step and its fold launch): the same step on a global layer
  route d  SpeckvKVConnector.attend(window=W), ONE position at the same rows_per_pos
--parent-lib PATH: routes c and d, whose kernels this tree leaves byte for byte, against a build of the parent commit in alternating processes.

    python profiles/tools/fp8_spec_window_bench.py [the options of k8v4_spec_window_bench.py] [--out profiles/fp8_spec_window.txt]
"""
import k8v4_spec_window_bench as bench


def connector(lib, L, H, D, T):
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    return SpeckvKVConnector(lib, L, H, D, T, "fp8")


if __name__ == "__main__":
    bench.POOL, bench.OUT, bench.TOOL, bench.connector = "an FP8 pool", "fp8_spec_window.txt", "fp8_spec_window_bench.py", connector
    bench.main()
