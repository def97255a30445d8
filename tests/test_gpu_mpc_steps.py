"""GPU parity tests of the MPC hot path off the reference's 0.02 s step.  dt_mpc is a run-time parameter of every handle
(qrw_config.dt_mpc): mpc_kernel.hip reads it into dt, dt / mass and 9.81 dt, into the dt * I_inv * skew(lever) blocks, the chain
factorisation, the dynamics rows of A x and A^T y and the equilibration norms, in every instantiation and launch form -- and every
other MPC test of the suite passes 0.02.  Here: ten configurations at eight other steps against the CPU oracle (which
tests/test_oracle_mpc.py holds against an independent dense assembly at such steps), the time-sliced and the sequence launch, the
position in the batch, and the two Python wrappers.

Criteria as in tests/test_gpu_mpc.py: every instance of every call takes the oracle's iteration count and status, rho within
1e-9, states and forces within 1e-4 each.  The oracle's two builds (strict IEEE, and -O3 -march=native) run side by side and must
agree on iteration count and status everywhere, so no termination decision of these inputs hangs on a rounding."""
import os

import numpy as np
import pytest

from test_gpu_mpc import RTOL, rel_err, run_sequence

pytestmark = pytest.mark.gpu

G5 = ("walk", "trot", "bounding", "pacing", "static")
G3 = ("walk", "trot", "bounding")

# row: (dt, horizons, N_gait, gaits, B, calls, closed loop); what it reaches in mpc_kernel.hip is in the docstring below
ROWS = {
    1: (0.010, (16,), 20, G5, 12, 6, True),
    2: (0.040, (8,), 20, G5, 12, 6, True),
    3: (0.025, (12,), 20, G5, 12, 6, True),
    4: (0.016, (20,), 24, G3, 8, 5, True),
    5: (0.005, (32,), 36, G3, 8, 4, True),
    6: (0.010, (32,), 36, G3, 8, 4, False),
    7: (0.030, (1, 2, 5), 20, ("trot",), 3, 4, True),
    8: (0.012, (17,), 24, G3, 5, 5, True),
    9: (0.008, (24,), 28, G3, 5, 4, False),
    10: (0.050, (16,), 20, G5, 12, 6, False),
}


def seed_of(dt, N):
    return 47000 + N + int(round(1e4 * dt))


@pytest.mark.parametrize("row", sorted(ROWS))
def test_other_steps_match_the_oracle(oracle_mod, synth_mod, row):
    """The smallest shapes that reach every instantiation, at steps from 0.005 s to 0.05 s (closed loop: the next call starts
    from the oracle's first predicted state; open: noisy states):
         1  dt 0.010  N 16        one wavefront, compile-time N             oracle iterations 150..2000
         2  dt 0.040  N 8         runtime N < 16                            100..550
         3  dt 0.025  N 12        runtime N < 16                            75..600
         4  dt 0.016  N 20        two wavefronts, runtime N                 200..1700
         5  dt 0.005  N 32        two wavefronts, compile-time N            275..2150
         6  dt 0.010  N 32 open   the same, with max-iter exits (status 2)  575..4000
         7  dt 0.030  N 1, 2, 5   the chain's ends                          50..325
         8  dt 0.012  N 17        the first N of the second wavefront       250..1675
         9  dt 0.008  N 24 open   two wavefronts, runtime N                 650..3825
        10  dt 0.050  N 16 open   one wavefront, compile-time N             175..1125
    Rows 1 and 5 also compare the persisted warm-start state and the decoded gait of two instances.
    Worst relative deviation from the oracle, as printed on the device (the suite measures about 1e-10 at 0.02 s):
        row 1  2.1e-13   row 2  3.2e-12   row 3  5.4e-13   row 4  4.6e-13   row 5  1.8e-13   row 6  6.1e-13 (statuses 1 and 2)
        row 7  6.4e-12 (N 1), 3.2e-11 (N 2), 1.2e-12 (N 5)      row 8  3.5e-13   row 9  1.4e-13   row 10  2.7e-11
    -- nothing above the 0.02 s figure; the larger ones belong to the short chains and the long steps, whose solves end after the
    fewest iterations (the two builds of the oracle differ from each other by 1.8e-10 and 1.3e-09 on rows 7 and 10)."""
    dt, horizons, N_gait, gaits, B, calls, closed = ROWS[row]
    seen = set()
    for N in horizons:
        eng, refs, worst = run_sequence(oracle_mod, synth_mod, B, N, gaits, calls, seed_of(dt, N), closed_loop=closed, N_gait=N_gait,
                                        dt=dt, guard=True, seen=seen)
        print("row %d: dt %g N %d: worst relative deviation %.2e, statuses %s" % (row, dt, N, worst, sorted(seen)))
        if row in (1, 5):
            for b in (0, B - 1):
                stt = eng.mpc_state(b)
                x, z, y = refs[b].iterates()
                assert np.allclose(stt["x"], x, rtol=1e-6, atol=1e-9)
                assert np.allclose(stt["z"], z, rtol=1e-6, atol=1e-9)
                assert np.allclose(stt["y"], y, rtol=1e-6, atol=1e-9)
                gait, S = eng.mpc_gait(b)
                assert np.array_equal(gait, refs[b].get_gait()) and np.array_equal(S, refs[b].get_Sgait())
    assert 1 in seen
    if row == 6:
        assert seen & {2, -2}, seen  # a solve that ran into max_iter: the exit that does not pass the residual test


def test_time_sliced_launch_matches_the_oracle_at_another_step(oracle_mod, synth_mod, monkeypatch):
    """Row 6's inputs (dt 0.01, N 32, open loop) at B = 24 through the time-sliced launch (slices of 200 iterations forced on a
    small batch): every instance takes the oracle's iteration count and status, results within 1e-4, as
    test_time_sliced_launch_matches_the_oracle asks at 0.02 s.  The oracle's two builds agree on all 24 instances at this seed.
    Worst relative deviation as printed on the device: 3.8e-13 (statuses 1 and 2, the longest solve 4000 iterations)."""
    import qrw_hip

    dt, N, B, N_gait = 0.010, 32, 24, 36
    monkeypatch.setenv("QRW_PREEMPT_CHUNK", "200")
    monkeypatch.setenv("QRW_PREEMPT_MIN_BATCH", "1")
    sb = synth_mod.SyntheticBatch(B, N, N_gait=N_gait, dt=dt, gaits=G3, seed0=seed_of(dt, N))
    eng = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, dt_mpc=dt, T_gait=dt * N)
    oracle_mod.build(fast=True)
    ref, ref2 = (oracle_mod.MPCBatch(B, dt, N, dt * N, N_gait, fast=f) for f in (False, True))
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    seen, worst, longest = set(), 0.0, 0
    for s in range(4):
        d = sb.step(s)
        out = eng.mpc_solve_host(d["xref"], d["fsteps"], s)
        r = ref.run(s, d["xref"], d["fsteps"], threads)
        ref2.run(s, d["xref"], d["fsteps"], threads)
        (it, st), (it2, st2) = ref.iters(), ref2.iters()
        assert np.array_equal(it, it2) and np.array_equal(st, st2), ("the oracle's two builds", s)
        g = eng.mpc_stats()
        assert np.array_equal(g["iters"], it) and np.array_equal(g["status"], st), (s, g["iters"], it)
        e = max(rel_err(out[:, :12], r[:, :12]), rel_err(out[:, 12:], r[:, 12:]))
        worst, longest = max(worst, e), max(longest, int(it.max()))
        assert rel_err(out[:, :12], r[:, :12]) < RTOL and rel_err(out[:, 12:], r[:, 12:]) < RTOL, s
        seen |= set(st.tolist())
    print("time-sliced, dt %g N %d B %d: worst relative deviation %.2e, statuses %s, longest solve %d" % (dt, N, B, worst, sorted(seen), longest))
    assert longest > 2 * 200 and seen & {2, -2}  # solves of several slices, and one that ends at max_iter


@pytest.mark.parametrize("dt,N,B,K,gaits", [(0.010, 16, 8, 4, ("trot",)), (0.008, 24, 5, 3, G3)])
def test_sequence_launch_equals_consecutive_calls_at_other_steps(synth_mod, dt, N, B, K, gaits):
    """qrw_mpc_solve_sequence against K calls of qrw_mpc_solve, bit for bit: results, iteration counts, the last call's status
    and rho, and the warm-start state (one more ordinary call on both handles)."""
    import torch

    import qrw_hip

    N_gait = max(20, N + 4)
    sb = synth_mod.SyntheticBatch(B, N, N_gait=N_gait, dt=dt, gaits=gaits, seed0=seed_of(dt, N) + 500)
    steps = [sb.step(s) for s in range(K + 1)]
    a, b = (qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, dt_mpc=dt, T_gait=dt * N) for _ in range(2))
    dev = torch.device("cuda", 0)
    xs = torch.from_numpy(np.stack([st["xref"] for st in steps[:K]])).to(dev)
    fs = torch.from_numpy(np.stack([st["fsteps"] for st in steps[:K]])).to(dev)
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
    assert (sa["status"] == 1).all() and np.isfinite(ref_out[-1]).all()
    x1 = torch.from_numpy(steps[K]["xref"]).to(dev)
    f1 = torch.from_numpy(steps[K]["fsteps"]).to(dev)
    assert np.array_equal(a.mpc_solve(x1, f1, K).cpu().numpy(), b.mpc_solve(x1, f1, K).cpu().numpy())


def test_batch_position_at_another_step(synth_mod):
    """Row 1's instances 5, 11 and 0 in a handle of three equal the handle of twelve, bit for bit, over its six calls."""
    import qrw_hip

    dt, (N,), N_gait, gaits, B, calls, _ = ROWS[1]
    big = synth_mod.SyntheticBatch(B, N, N_gait=N_gait, dt=dt, gaits=gaits, seed0=seed_of(dt, N))
    sub = [5, 11, 0]
    eng_big = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, dt_mpc=dt, T_gait=dt * N)
    eng_sub = qrw_hip.Batch(len(sub), n_steps=N, N_gait=N_gait, dt_mpc=dt, T_gait=dt * N)
    for s in range(calls):
        d = big.step(s)
        a = eng_big.mpc_solve_host(d["xref"], d["fsteps"], s)
        b = eng_sub.mpc_solve_host(d["xref"][sub], d["fsteps"][sub], s)
        assert np.array_equal(a[sub], b), s
        assert np.array_equal(eng_big.mpc_stats()["iters"][sub], eng_sub.mpc_stats()["iters"])


def test_wrappers_pass_the_step_on(synth_mod):
    """One call sequence at dt 0.01 through MPC_Wrapper_batch and through the drop-in MPC class gives what a plain Batch gives, bit
    for bit.  The drop-in object is created after a drop-in MPC(0.02, 16, 0.32, 20) exists in the same process: the two differ in
    nothing but the step (and the period that follows from it), and must not be handed the same handle (qrw_hip.shared_batch1's
    key) -- both are stepped in turn, each against a plain handle of its own step."""
    import torch

    import libquadruped_reactive_walking as lqrw
    import MPC_Wrapper
    import qrw_hip

    dt, N, N_gait, B, calls = 0.010, 16, 20, 4, 4
    sb = synth_mod.SyntheticBatch(B, N, N_gait=N_gait, dt=dt, gaits=("trot", "walk"), seed0=seed_of(dt, N) + 900)
    sb02 = synth_mod.SyntheticBatch(1, N, N_gait=N_gait, gaits=("trot",), seed0=seed_of(0.02, N) + 900)
    plain = qrw_hip.Batch(B, n_steps=N, N_gait=N_gait, dt_mpc=dt, T_gait=dt * N)
    plain02 = qrw_hip.Batch(1, n_steps=N, N_gait=N_gait, dt_mpc=0.02, T_gait=0.32)
    wrap = MPC_Wrapper.MPC_Wrapper_batch(dt, N, dt * N, N_gait, B)
    first = lqrw.MPC(0.02, N, 0.32, N_gait)
    drop = lqrw.MPC(dt, N, dt * N, N_gait)
    assert drop._b is not first._b and drop._b.dt_mpc == dt and first._b.dt_mpc == 0.02
    dev = torch.device("cuda", 0)
    for s in range(calls):
        d, d02 = sb.step(s), sb02.step(s)
        want = plain.mpc_solve_host(d["xref"], d["fsteps"], s)
        wrap.get_latest_result_batch()  # (the first call returns the default forces, as the reference's wrapper does)
        assert wrap.solve_batch(s, torch.from_numpy(d["xref"]).to(dev), torch.from_numpy(d["fsteps"]).to(dev)) == 0
        got = wrap.get_latest_result_batch().cpu().numpy()
        assert np.array_equal(got, want), s
        assert np.array_equal(wrap.stats()["iters"], plain.mpc_stats()["iters"])
        # the two drop-in objects in turn: the 0.02 s one first, on its own inputs, then the 0.01 s one on instance 2's
        assert first.run(s, d02["xref"][0], d02["fsteps"][0]) == 0
        assert np.array_equal(first.get_latest_result(), plain02.mpc_solve_host(d02["xref"], d02["fsteps"], s)[0]), s
        assert drop.run(s, d["xref"][2], d["fsteps"][2]) == 0
        assert np.array_equal(drop.get_latest_result(), want[2]), s
        assert drop.solver_stats()["iters"] == plain.mpc_stats()["iters"][2]
