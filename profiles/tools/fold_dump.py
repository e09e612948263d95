#!/usr/bin/env python3
"""The bytes the two held-row folds write, for comparing two builds of the library (profiles/fold_one_body.txt).

Seeded inputs of tests/test_gpu_spec_tree.py (fold_case: 7 sequences, 5 of them in the launch through d_rows, scores +-40 from the stored
lse, a sequence with nothing stored) at every launch shape of its SHAPES: speckv_ext_attend_fold_held with the bases and ragged live
counts of test_chain_masks_equal_fold_held, then speckv_ext_attend_fold_masked with the mask words of every kind of KINDS.  out and lse
of every call are appended to FILE as they come back; the SHA-256 of the file is printed.  Run it once per build, each as a process
of its own, and compare the files:

    SPECKV_LIB_PATH=<parent's libcxlspeckv.so> python profiles/tools/fold_dump.py parent.bin
    python profiles/tools/fold_dump.py branch.bin  &&  cmp parent.bin branch.bin
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_gpu_spec_tree import HELD_MAX, KINDS, SHAPES, fold_case, mask_words, open_lib, pkg, run_fold_held, run_fold_masked, torch_mod


def main():
    torch, lib, sm, calls = torch_mod(), open_lib(), 0.0884, 0
    try:
        with open(sys.argv[1], "wb") as f:
            for rpp, n_q in SHAPES:
                rng = np.random.default_rng(3000 * rpp + n_q)
                c = fold_case(rng, rpp, n_q)
                args = (c["q"], c["out"], c["lse"], c["kbuf"], c["vbuf"], c["seq_stride"], c["pos_stride"])
                results = [run_fold_held(lib, torch, *args, [0, 1, 1, HELD_MAX - n_q, 0], [n_q, n_q, max(n_q - 1, 1), n_q, 0], rpp, sm, c["rows"])]
                for kind in KINDS:
                    results.append(run_fold_masked(lib, torch, *args, mask_words(kind, rng, len(c["rows"]), n_q), rpp, sm, c["rows"]))
                for out, lse in results:
                    f.write(out.tobytes()); f.write(lse.tobytes())
                    calls += 1
    finally:
        lib.finalize()
    data = open(sys.argv[1], "rb").read()
    print(f"{pkg.library_path()}: {calls} calls, {len(data)} bytes, sha256 {hashlib.sha256(data).hexdigest()}")


if __name__ == "__main__":
    main()
