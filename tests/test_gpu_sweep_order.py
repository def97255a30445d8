"""The paired block-tridiagonal sweeps of the MPC solve visit the wavefront's halves as lower, lower, upper, upper (2 + 2
order, csrc/chain_sweep.h) instead of changing halves after every step.  The order moves no arithmetic: every step is the
same 12 FMAs in the same sequence, so the solver must reproduce the build before the change BIT FOR BIT.  The fixtures
tests/golden/sweep_order/sweep_order_parent_n{16,32}.npz were recorded on an MI355X from that earlier build
(tests/golden/make_sweep_order_parent.py, which runs the workloads below); anything but exact equality is a defect.
(A directory of their own: tests/test_golden.py takes every tests/golden/*.npz for an oracle fixture of its schema.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_order")

# name -> (N, batch, gaits, calls): seeded inputs of consecutive receding-horizon calls, the set-up call (0) included
WORKLOADS = {
    "n16": (16, 8, ("trot",), 3),
    "n32": (32, 4, ("walk", "trot", "bounding"), 2),
}
SEED0 = 20400000


def run_workload(name):
    """Every call's result (calls, B, 24, N) float64, iteration counts, status (int) and rho (float64), each (calls, B).
    Plain launch: the time slicing of N > 16 is switched off for this handle."""
    import qrw_hip
    import synth

    N, B, gaits, calls = WORKLOADS[name]
    N_gait = max(20, N + 4)
    sb = synth.SyntheticBatch(B, N, N_gait=N_gait, gaits=gaits, seed0=SEED0 + N)
    old = os.environ.get("QRW_PREEMPT_CHUNK")
    os.environ["QRW_PREEMPT_CHUNK"] = "0"
    try:
        eng = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, T_gait=0.02 * N)
    finally:
        if old is None:
            del os.environ["QRW_PREEMPT_CHUNK"]
        else:
            os.environ["QRW_PREEMPT_CHUNK"] = old
    res = dict(out=[], iters=[], status=[], rho=[])
    for s in range(calls):
        d = sb.step(s)
        res["out"].append(eng.mpc_solve_host(d["xref"], d["fsteps"], s).copy())
        st = eng.mpc_stats()
        for key in ("iters", "status", "rho"):
            res[key].append(np.array(st[key]).copy())
    eng.close()
    return {k: np.stack(v) for k, v in res.items()}


def test_sweeps_selftest_covers_both_compile_time_horizons():
    """qrw_selftest_sweeps checks chain_forward / chain_backward <16> and <32> against a dense host evaluation."""
    import qrw_hip

    rc, err = qrw_hip.selftest_sweeps()
    print("selftest_sweeps: rc %d, error %.3e" % (rc, err))
    assert rc == 0 and err < 1e-12


@pytest.mark.parametrize("name", ["n16", "n32"])
def test_bitwise_identical_to_the_build_before_the_change(name):
    want = np.load(os.path.join(GOLDEN, "sweep_order_parent_%s.npz" % name))
    got = run_workload(name)
    assert want["out"].dtype == np.float64 and got["out"].dtype == np.float64
    print("%s: iteration counts %s" % (name, got["iters"].tolist()))
    # a rho refactorisation (first tested at iteration 200) must be on the path, here and in the recording
    assert (want["iters"] >= 200).any()
    assert np.array_equal(got["iters"], want["iters"])
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["rho"], want["rho"])
    assert np.array_equal(got["out"], want["out"])


def test_n32_time_sliced_launch_equals_the_plain_one(monkeypatch):
    """mpc_solve_kernel<2, true, false, true> (N = 32, time-sliced) on the smallest batch the slicing accepts (more than
    QRW_PREEMPT_MIN_BATCH = 1 instance), slices of 200 iterations.  Same inputs through the plain launch, exact equality."""
    import qrw_hip
    import synth

    N, B, N_gait = 32, 2, 36
    sb = synth.SyntheticBatch(B, N, N_gait=N_gait, gaits=("walk", "trot", "bounding"), seed0=SEED0 + 100)
    monkeypatch.setenv("QRW_PREEMPT_CHUNK", "0")
    plain = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, T_gait=0.02 * N)
    monkeypatch.setenv("QRW_PREEMPT_MIN_BATCH", "1")
    monkeypatch.setenv("QRW_PREEMPT_CHUNK", "200")
    sliced = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, T_gait=0.02 * N)
    resumed = 0
    for s in range(2):
        d = sb.step(s)
        a = plain.mpc_solve_host(d["xref"], d["fsteps"], s)
        b = sliced.mpc_solve_host(d["xref"], d["fsteps"], s)
        sa, sb_ = plain.mpc_stats(), sliced.mpc_stats()
        for key in ("iters", "status", "rho"):
            assert np.array_equal(sa[key], sb_[key]), (s, key)
        assert np.array_equal(a, b), s
        st = sliced.mpc_slice_stats()
        assert st["chunk"] == 200 and st["finished"] == B, st  # the time-sliced kernel did run
        resumed += int((sb_["iters"] > 200).sum())
    assert resumed > 0, "no solve went past its first slice"


@pytest.mark.parametrize("N,B,K", [(16, 2, 2), (32, 2, 2)])
def test_sequence_launch_equals_plain_calls(N, B, K, monkeypatch):
    """mpc_solve_kernel<NW, true, true> (qrw_mpc_solve_sequence, K = 2 calls of 2 instances) against K plain launches."""
    import torch

    import qrw_hip
    import synth

    N_gait = max(20, N + 4)
    monkeypatch.setenv("QRW_PREEMPT_CHUNK", "0")
    sb = synth.SyntheticBatch(B, N, N_gait=N_gait, gaits=("trot", "walk"), seed0=SEED0 + 200 + N)
    steps = [sb.step(s) for s in range(K)]
    a, b = (qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, T_gait=0.02 * N) for _ in range(2))
    dev = torch.device("cuda", 0)
    xs = torch.from_numpy(np.stack([st["xref"] for st in steps])).to(dev)
    fs = torch.from_numpy(np.stack([st["fsteps"] for st in steps])).to(dev)
    ref_out, ref_it = [], []
    for s in range(K):
        ref_out.append(a.mpc_solve(xs[s], fs[s], s).cpu().numpy())
        ref_it.append(a.mpc_stats()["iters"].copy())
    its = torch.zeros((K, B), dtype=torch.int32, device=dev)
    out = b.mpc_solve_sequence(xs, fs, 0, iters=its)
    torch.cuda.synchronize()
    assert not b.mpc_sequence_timed_out()
    assert np.array_equal(its.cpu().numpy(), np.stack(ref_it))
    assert np.array_equal(out.cpu().numpy(), np.stack(ref_out))
    sa, sb_ = a.mpc_stats(), b.mpc_stats()
    for key in ("iters", "status", "rho"):
        assert np.array_equal(sa[key], sb_[key]), key
