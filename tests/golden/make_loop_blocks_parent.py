"""Records tests/golden/loop_blocks/loop_blocks_parent_<case>.npz: what the build BEFORE the ADMM loop ran in check-free blocks
computes for the cases of tests/test_gpu_mpc_loop_blocks.py (results, iteration counts, status, rho of every call), and prints
that build's own parity with the CPU oracle.

Run on an MI355X with QRW_HIP_LIB pointing at a libqrw_hip.so built from the commit before the change:
    QRW_HIP_LIB=/path/to/parent/libqrw_hip.so python tests/golden/make_loop_blocks_parent.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "quadruped-reactive-walking_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import test_gpu_mpc_loop_blocks as t  # noqa: E402

if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "loop_blocks")
    os.makedirs(out_dir, exist_ok=True)
    for name in t.CASES:
        r = t.run_case(name)
        print(name, "iters", r["iters"].tolist(), "status", r["status"].tolist())
        np.savez_compressed(os.path.join(out_dir, "loop_blocks_parent_%s.npz" % name), **r)
        try:
            t.oracle_parity(r, t.oracle_case(name))
        except AssertionError as e:  # (reported, not fatal: the recording is of what that build computes)
            print(name, "PARITY WITH THE ORACLE FAILS:", e)
