"""GPU tests of the batched planners off their default geometry (qrw_planner_config: shoulders, h_ref, max_height, lock_time,
init_target, init_foot_pos) against the oracle: everything changed at once (TUNED), each parameter alone, and a lock time
longer than any swing.  Cases, sequences, the oracle's runs and the bounds come from tests/planner_cases.py; that each parameter
alone moves the oracle's outputs by far more than a bound is asserted on the oracle in tests/test_planner_cases_cpu.py."""
import numpy as np
import pytest

import planner_cases as pc
from test_gpu_planner_limits import Q_INIT, _t, run_against_the_oracle

pytestmark = pytest.mark.gpu


def test_tuned_geometry_matches_oracle(oracle_mod):
    """TUNED: four different shoulder x and y (and z), h_ref 0.24, max_height 0.08, lock_time 0.04, targets and initial foot
    positions each shifted from the shoulders by its own offset, k_mpc 4; B = 9, 400 iterations, measured velocities that are
    the reference plus noise (the targets move inside the swing), two gait changes per robot.  Measured on the device (err /
    bound, worst over the run):
        xref 3.1e-16 / 3.1e-14  fsteps 1.4e-15 / 1.2e-13  target 1.4e-15 / 1.2e-13  pos 2.1e-09 / 2.9e-07  vel 1.7e-08 / 3.5e-06  acc 1.2e-07 / 1.6e-05
    Before swing_t0 (planner_kernel.hip) rounded its product and differences one by one the device missed this bound by five
    orders of magnitude: pos 1.1e-02 at iteration 96, a tie of `t0 < t_swing - lock_time` decided the other way."""
    c = pc.CASES["TUNED"]["geometry"]
    assert len(set(c["shoulders"][0])) == 4 and len(set(np.abs(c["shoulders"][1]))) == 4
    run_against_the_oracle(oracle_mod, "TUNED")


@pytest.mark.parametrize("case", pc.ALONE)
def test_each_geometry_parameter_alone_matches_oracle(oracle_mod, case):
    """One parameter of qrw_planner_config off its default, the others at theirs: B = 9, 300 iterations, one or two gait changes
    per robot.  Measured on the device (err, worst over the run; the bounds are 100 x planner_cases.SPREAD):
        shoulders     xref 1.4e-16  fsteps 8.9e-16  target 8.9e-16  pos 6.1e-11  vel 2.4e-10  acc 9.3e-10
        h_ref         xref 1.4e-16  fsteps 8.9e-16  target 8.3e-16  pos 6.3e-11  vel 3.7e-10  acc 2.0e-09
        max_height    xref 1.4e-16  fsteps 8.9e-16  target 8.3e-16  pos 7.5e-11  vel 5.7e-10  acc 4.6e-09
        lock_time     xref 1.4e-16  fsteps 8.9e-16  target 8.3e-16  pos 2.8e-09  vel 2.1e-08  acc 1.2e-07
        init_target   xref 1.4e-16  fsteps 8.9e-16  target 8.3e-16  pos 7.5e-11  vel 5.7e-10  acc 4.6e-09
        init_foot_pos xref 1.4e-16  fsteps 8.9e-16  target 8.3e-16  pos 8.5e-11  vel 6.5e-10  acc 3.0e-09"""
    assert list(pc.CASES[case]["geometry"]) == [case]
    run_against_the_oracle(oracle_mod, case)


def test_lock_time_longer_than_the_swing_matches_oracle(oracle_mod):
    """lock_time = 0.5 s, longer than any swing: `t0 < t_swing - lock_time` never holds, the x / y coefficients are never updated
    and stay zero as the reference leaves them (FootTrajectoryGenerator.cpp:28-29,53), so a swinging foot's x / y position,
    velocity and acceleration are EXACTLY zero on both sides and a stance foot keeps its initial position; z does not depend on
    any input (the oracle's spread is 0) and is bounded from the number format, planner_cases.z_bound.  The other outputs as
    everywhere.  Measured on the device, z rows, largest |device - oracle| / bound over the run: pos 0.029, vel 0.017, acc 0.024."""
    case = "lock_long"
    ref, zb = pc.oracle_run(oracle_mod, case), pc.z_bound(oracle_mod, case)
    swing = ref["gait"][:, :, 0, :] == 0
    assert swing.any() and (ref["pos"][:, :, :2][np.broadcast_to(swing[:, :, None, :], ref["pos"][:, :, :2].shape)] == 0.0).all()
    ratio = [0.0, 0.0, 0.0]

    def trajectories(k, got, ref):
        for d, name in enumerate(("pos", "vel", "acc")):
            assert np.array_equal(got[name][:, :2], ref[name][k][:, :2]), (k, name)
            dz = np.abs(got[name][:, 2] - ref[name][k][:, 2]).max(-1)
            assert (dz <= zb[k, :, d]).all(), (k, name, dz, zb[k, :, d])
            ratio[d] = max(ratio[d], float((dz / np.maximum(zb[k, :, d], 1e-300)).max()))

    run_against_the_oracle(oracle_mod, case, floats=("xref", "fsteps", "target"), extra=trajectories)
    print("lock_long: z rows, largest |device - oracle| / bound: pos %.2g vel %.2g acc %.2g" % tuple(ratio))


def test_tuned_geometry_quad_form_equals_the_thread_form(monkeypatch):
    """qrw_control_pre with the TUNED planner configuration: the quad kernel (which selects its foot's shoulder from the kernel
    arguments and keeps the trajectory of one foot per lane) against the one-thread-per-robot form, the kernel
    test_tuned_geometry_matches_oracle holds against the oracle.  The joystick velocity, the measured velocity and the base
    attitude are those of the TUNED sequence (the planners' inputs stay in the range the spread was measured on), so the bounds
    are TUNED's: gait and contacts exactly, xref / fsteps / target / foot position, velocity, acceleration within 100 x the
    oracle's spread, every iteration; the planner's state items at intervals."""
    import torch

    import qrw_hip

    case = "TUNED"
    c, seq = pc.CASES[case], pc.sequence(case)
    K, B = seq["code"].shape
    N, Ng, k_mpc = c["N"], c["N_gait"], c["k_mpc"]
    engs = [qrw_hip.Batch(B, **pc.handle_kwargs(case)) for _ in range(2)]
    for e in engs:
        e.planner_init(**pc.planner_init_kwargs(case))
        e.controller_init(_t(np.tile(Q_INIT, (B, 1))), c["geometry"]["h_ref"])
    rng = np.random.default_rng(5)
    qf = np.zeros((B, 19))
    qf[:, 2], qf[:, 6], qf[:, 7:] = 0.24, 1.0, Q_INIT
    x_f = np.zeros((B, 24, N))
    x_f[:, 2, :], x_f[:, 14::3, :] = 0.24, 6.0
    outs, worst = [None, None], dict.fromkeys(pc.FLOAT_OUTPUTS, 0.0)
    for k in range(K):
        vf = np.zeros((B, 18))
        vf[:, :6] = seq["hv"][k]
        rpy = rng.uniform(-0.02, 0.02, (B, 3))
        qf[:, 0:2] += c["dt_wbc"] * seq["vref"][k][:, 0:2]
        solve = k % k_mpc == 0
        for i, eng in enumerate(engs):
            monkeypatch.setenv("QRW_PRE_QUAD", "1" if i == 0 else "0")
            outs[i] = eng.control_pre(k, _t(seq["vref"][k]), _t(qf), _t(vf), _t(rpy), _t(seq["code"][k], np.int32),
                                      x_f_mpc=(None if solve else _t(x_f)), out=outs[i], mpc_inputs=solve)
        a, b = ({n: v.cpu().numpy() for n, v in o.items()} for o in outs)
        assert np.array_equal(a["contacts"], b["contacts"]) and (not solve or np.array_equal(a["gait"], b["gait"])), k
        pairs = dict(xref=(a["xref"], b["xref"]) if solve else (a["xref"][:, :, :2], b["xref"][:, :, :2]), target=(a["target"], b["target"]),
                     pos=(a["feet_pva"][:, 0], b["feet_pva"][:, 0]), vel=(a["feet_pva"][:, 1], b["feet_pva"][:, 1]),
                     acc=(a["feet_pva"][:, 2], b["feet_pva"][:, 2]))
        if solve:
            pairs["fsteps"] = (a["fsteps"], b["fsteps"])
        for name, (x, y) in pairs.items():
            e = pc.err(x, y)
            worst[name] = max(worst[name], e)
            assert e <= pc.bound(case, name), (k, name, e, pc.bound(case, name))
        if k % pc.STATE_EVERY == 3 or solve:
            for r in (0, 4, B - 1):
                for item, n in ((0, 4 * Ng), (1, 4 * Ng), (2, 4 * Ng), (3, 1), (4, 1), (5, 1), (6, 1)):
                    assert np.array_equal(engs[0].planner_get(item, n, r), engs[1].planner_get(item, n, r)), (k, r, item)
                for item, n, name in ((7, 12, "target"), (8, 12, "target"), (9, 12, "pos"), (10, 12, "vel"), (11, 12, "acc"), (17, 12, "target")):
                    e = pc.err(engs[0].planner_get(item, n, r).reshape(3, 4), engs[1].planner_get(item, n, r).reshape(3, 4))
                    assert e <= pc.bound(case, name), (k, r, item, e)
    assert (seq["code"] != 0).any()
    print("TUNED, quad form against thread form: %s" % "  ".join("%s %.2e / %.2e" % (n, w, pc.bound(case, n)) for n, w in worst.items()))
    for e in engs:
        e.close()
