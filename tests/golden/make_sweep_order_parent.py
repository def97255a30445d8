"""Records tests/golden/sweep_order/sweep_order_parent_n{16,32}.npz: what the build BEFORE the 2 + 2 half order of the paired sweeps
computes for the workloads of tests/test_gpu_sweep_order.py (results, iteration counts, status, rho of every call).

Run on an MI355X with QRW_HIP_LIB pointing at a libqrw_hip.so built from the commit before the change:
    QRW_HIP_LIB=/path/to/parent/libqrw_hip.so python tests/golden/make_sweep_order_parent.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "quadruped-reactive-walking_amd")):
    sys.path.insert(0, p)

import test_gpu_sweep_order as t  # noqa: E402

if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sweep_order")
    os.makedirs(out_dir, exist_ok=True)
    for name in t.WORKLOADS:
        r = t.run_workload(name)
        assert (r["iters"] >= 200).any(), "no solve reaches the first rho test: pick another seed"
        np.savez_compressed(os.path.join(out_dir, "sweep_order_parent_%s.npz" % name), **r)
        print(name, "iters", r["iters"].tolist(), "status", r["status"].tolist())
