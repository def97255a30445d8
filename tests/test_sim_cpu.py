"""CPU tests of the rigid-body simulator's checker (tests/sim_numpy.py: its own physics, momentum in flight; no GPU) and of the Python surface that
can be checked without a device (the drop-in's names, Simulator_batch refusing stream groups)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sn(oracle_mod):
    import sim_numpy

    return sim_numpy


def _random_state(sn, rng, height=0.3):
    quat = rng.normal(size=4) * [0.2, 0.2, 1.0, 1.0]
    quat /= np.linalg.norm(quat)
    q = np.concatenate([[rng.normal(), rng.normal(), height], quat, sn.Q_STANCE + 0.3 * rng.normal(size=12)])
    v = np.concatenate([rng.normal(size=6), 3.0 * rng.normal(size=12)])
    return q, v


def test_free_fall_is_gravity_in_the_base_frame(sn):
    """No contact, zero torque, base at rest with the joints moving freely set to rest: the base accelerates with (0, 0, -9.81)
    rotated into the base frame and the joints do not accelerate.  (Measured: 4e-13.)"""
    rng = np.random.default_rng(0)
    for _ in range(5):
        q, _ = _random_state(sn, rng, height=1.0)
        a, f, d = sn.forward_dynamics(q, np.zeros(18), np.zeros(12))
        assert np.all(d < 0) and not f.any()
        g_b = sn.quat_to_rot(q[3:7]).T @ np.array([0.0, 0.0, -9.81])
        assert np.abs(a[:3] - g_b).max() < 1e-10 and np.abs(a[3:]).max() < 1e-9, (a[:3] - g_b, np.abs(a[3:]).max())


def test_inverse_dynamics_of_the_forward_dynamics(sn, oracle_mod):
    """oracle.rnea(q, v, a) - J'f == [0; tau] (+ the external wrench in the base frame) on random states in and out of contact."""
    rng = np.random.default_rng(1)
    seen = set()
    for t in range(12):
        q, v = _random_state(sn, rng, height=0.2 + 0.04 * rng.normal())
        tau = rng.normal(size=12)
        fe = rng.normal(size=6) if t % 2 else None
        a, f, d = sn.forward_dynamics(q, v, tau, f_ext=fe)
        seen.add(int((d > 0).sum()))
        want = np.concatenate([np.zeros(6), tau])
        if fe is not None:
            R = sn.quat_to_rot(q[3:7])
            want[:3] += R.T @ fe[:3]
            want[3:6] += R.T @ fe[3:]
        got = oracle_mod.rnea(q, v, a) - oracle_mod.feet_jacobians(q).T @ f.ravel()
        scale = np.abs(oracle_mod.crba(q)) @ np.abs(a) + np.abs(oracle_mod.rnea(q, v, np.zeros(18)))
        assert np.all(np.abs(got - want) <= 1e-12 * scale + 1e-12), np.abs(got - want).max()
    assert len(seen) >= 3, seen


def momentum_drift(sn, q, v, substeps, ticks=25, step=None):
    """A tumbling robot in flight under zero gains and torques for `ticks` ticks of 2 ms: the drift of the horizontal linear
    momentum, the drift of the vertical angular momentum about the world origin, and -dp_z / (g t), the mass the fall shows.
    step: None = the checker; or a function (q, v, substeps, ticks) -> (q, v) after the ticks (the device)."""
    if step is None:
        s = sn.SimNumpy(q, substeps=substeps)
        s.set_state(q, v, np.zeros(3))
        z = np.zeros(12)
        for _ in range(ticks):
            s.step(z, z, z, z, z)
        assert s.status == 0 and s.tick == ticks and s.min_abs_d > 0.5  # (never near the ground)
        q1, v1 = s.q, s.v
    else:
        q1, v1 = step(q, v, substeps, ticks)
    h0, h1 = sn.world_momentum(q, v), sn.world_momentum(q1, v1)
    return np.linalg.norm((h1 - h0)[:2]), abs((h1 - h0)[5]), -(h1 - h0)[2] / (9.81 * ticks * sn.DEFAULTS["dt"])


def test_momentum_in_flight(sn):
    """Gravity changes neither the horizontal linear momentum nor the vertical angular momentum about the world origin, whatever
    the robot's tumbling: what drift the checker shows is its first-order integrator's and halves (factor in [1.9, 2.1]) with every
    doubling of the sub-steps, and the fall shows the robot's 2.5 kg from below, monotonically.  A Coriolis term missing from h,
    or one that does not belong to M, leaves a drift that does not shrink.  Measured (seed 5, 25 ticks):
      sub-steps   linear (xy)   angular z   mass
          4        2.67e-04     4.69e-05    2.499939
          8        1.34e-04     2.34e-05    2.499971
         16        6.68e-05     1.17e-05    2.499987
         32        3.34e-05     5.86e-06    2.499995      every ratio, linear and angular, 2.000 to four figures"""
    q, v = sn.tumbling_state(np.random.default_rng(5))
    rows = [momentum_drift(sn, q, v, n) for n in (4, 8, 16, 32)]
    for n, (lin, ang, mass) in zip((4, 8, 16, 32), rows):
        print("substeps %2d: linear drift %.3g, angular-z drift %.3g, mass %.6f" % (n, lin, ang, mass))
    for (lin_a, ang_a, mass_a), (lin_b, ang_b, mass_b) in zip(rows, rows[1:]):
        assert 1.9 <= lin_a / lin_b <= 2.1 and 1.9 <= ang_a / ang_b <= 2.1, (lin_a / lin_b, ang_a / ang_b)
        assert mass_a < mass_b < 2.5, (mass_a, mass_b)
    assert 2.5 - rows[-1][2] < 1e-4, rows[-1][2]
    assert rows[0][0] > 1e-5 and rows[0][1] > 1e-7  # (the state does tumble: there is a drift to halve)


def test_longdouble_solve_agrees_with_float64(sn, oracle_mod):
    rng = np.random.default_rng(2)
    q, v = _random_state(sn, rng, 0.2)
    M = oracle_mod.crba(q)
    r = rng.normal(size=18)
    x = sn.solve_longdouble(M, r)
    assert np.abs(np.asarray(x, dtype=float) - np.linalg.solve(M, r)).max() < 1e-10 * np.abs(x).max()


def test_standing_run(sn):
    """The run behind the defaults (dt 0.002, 8 sub-steps, kn 1e4, dn 60, mu 0.9, vs 0.01): PD only, P = 3, D = 0.2 toward the
    stance, from base height 0.235 m, 1500 ticks.  Recorded with this checker: finite throughout, final base height 0.2346 m, the
    four normal forces of the last sub-step equal within 0.002 N (6.71 N each), largest velocity component over the last 500
    ticks 0.104.  The contacts do not come to rest: the explicit friction and damping terms leave a period-two ripple over the
    sub-steps (total normal force 22.2 / 26.9 N alternating about the weight, 24.5 N), bounded, and six times larger with 4
    sub-steps (velocity 0.57, force spread 7 N) -- hence 8 sub-steps as the default."""
    s = sn.SimNumpy(sn.Q_STANCE, base_height=0.235)
    vmax, fz = 0.0, []
    for k in range(1500):
        o = s.step(3.0, 0.2, sn.Q_STANCE, np.zeros(12), np.zeros(12))
        assert s.status == 0, k
        if k >= 1000:
            vmax = max(vmax, np.abs(s.v).max())
            fz.append(o["contact_forces"][:, 2])
    fz = np.array(fz)
    print("standing run: z %.4f, vmax %.3g over the last 500 ticks, fz mean %s spread %.3g, min |d| %.3g"
          % (s.q[2], vmax, fz.mean(0).round(3), fz.max() - fz.min(), s.min_abs_d))
    assert s.tick == 1500 and np.all(np.isfinite(s.q)) and np.all(np.isfinite(s.v))
    assert 0.18 <= s.q[2] <= 0.24, s.q[2]
    assert vmax <= 0.5, vmax
    assert np.all(fz > 0) and np.abs(fz.mean(0) - fz.mean()).max() < 0.01


def test_measurements_on_a_hand_made_state(sn):
    """UpdateMeasurment (:593-631) spelled out by hand: yaw 90 degrees, so R maps base x to world y."""
    c = np.sqrt(0.5)
    q = np.concatenate([[1.0, 2.0, 0.3], [0.0, 0.0, c, c], np.arange(12) * 0.1])
    v = np.concatenate([[0.5, 0.0, 0.0], [0.0, 0.0, 2.0], np.arange(12) * -0.2])
    prev = np.array([0.1, 0.2, 0.3])
    o = sn.measurements(q, v, prev, 0.002)
    assert np.array_equal(o["q_mes"], q[7:]) and np.array_equal(o["v_mes"], v[6:]) and np.array_equal(o["quat"], q[3:7])
    assert np.array_equal(o["ang_vel"], [0.0, 0.0, 2.0]) and np.array_equal(o["true_pos"], [1.0, 2.0, 0.3])
    assert np.array_equal(o["true_b_vel"], [0.5, 0.0, 0.0])
    # cross((0.1163, 0, 0.02), (0, 0, 2)) = (0, -0.2326, 0); base velocity + that = (0.5, -0.2326, 0) -> world (0.2326, 0.5, 0)
    assert np.allclose(o["o_imu_vel"], [0.2326, 0.5, 0.0], rtol=0, atol=1e-15)
    # R'(o_imuVel - prev) / dt: world (0.1326, 0.3, -0.3) -> base (0.3, -0.1326, -0.3), / 0.002
    assert np.allclose(o["lin_acc"], [150.0, -66.3, -150.0], rtol=0, atol=1e-11)


def test_first_measurement_and_the_frozen_robot(sn):
    s = sn.SimNumpy(sn.Q_STANCE)
    assert not s.out["lin_acc"].any() and not s.prev.any() and s.tick == 0
    z = np.zeros(12)
    s.step(3.0, 0.2, sn.Q_STANCE, z, z)
    q, v, out = s.q.copy(), s.v.copy(), {k: x.copy() for k, x in s.out.items()}
    bad = z.copy()
    bad[4] = np.nan
    s.step(3.0, 0.2, sn.Q_STANCE, z, bad)
    assert s.status == 1 and s.tick == 1 and np.array_equal(s.q, q) and np.array_equal(s.v, v)
    s.step(3.0, 0.2, sn.Q_STANCE, z, z)  # frozen for good
    assert s.tick == 1 and all(np.array_equal(s.out[k], out[k]) for k in out)


def test_drop_in_surface():
    """The names the reference's callers use on the device object (scripts/PyBulletSimulator.py), listed by hand."""
    import PyBulletSimulator as P

    methods = ["Init",                      # :557
               "cross3",                    # :577
               "UpdateMeasurment",          # :588
               "SetDesiredJointTorque",     # :635
               "SetDesiredJointPDgains",    # :646
               "SetDesiredJointPosition",   # :656
               "SetDesiredJointVelocity",   # :664
               "SendCommand",               # :672
               "Stop"]                      # :726
    attributes = ["cpt", "nb_motors", "jointTorques", "revoluteJointIndices", "hardware",                      # :532-536
                  "q_mes", "v_mes", "torquesFromCurrentMeasurment", "baseAngularVelocity", "baseOrientation",  # :539-543
                  "baseLinearAcceleration", "baseAccelerometer", "o_baseVel", "o_imuVel", "prev_o_imuVel",     # :544-548
                  "P", "D", "q_des", "v_des", "tau_ff"]                                                        # :551-555
    d = P.PyBulletSimulator()
    for m in methods:
        assert callable(getattr(d, m)), m
    for a in attributes:
        assert hasattr(d, a), a
    assert d.q_mes.shape == (12,) and d.baseOrientation.shape == (4,) and d.o_imuVel.shape == (3, 1) and d.cpt == 0
    for a in ("roll", "pitch", "yaw"):  # :504-506
        assert getattr(d.hardware, a) == 0.0
    assert d.hardware.IsTimeout() is False and d.hardware.Stop() == 0 and d.hardware.imu_data_attitude(2) == 0.0
    q = np.zeros(12)
    for kw in (dict(envID=1), dict(use_flat_plane=False), dict(enable_pyb_GUI=True)):  # refused before any device is touched
        with pytest.raises(NotImplementedError):
            d.Init(q_init=q, **kw)
    assert np.array_equal(d.cross3([1, 0, 0], [0, 1, 0]), [[0], [0], [1]])
    d.SetDesiredJointPDgains(3.0, 0.2)
    d.SetDesiredJointTorque(q + 1.0)
    assert d.P == 3.0 and d.D == 0.2 and np.array_equal(d.tau_ff, q + 1.0)
    assert np.allclose(P.quaternionToRPY([0.0, 0.0, 0.5, np.sqrt(0.75)]).ravel(), [0.0, 0.0, np.pi / 3])


def test_simulator_batch_refuses_stream_groups():
    """Controller_groups is out of scope: refused with a ValueError that says so, before a handle is made."""
    import Controller
    import Simulator

    groups = object.__new__(Controller.Controller_groups)  # (no constructor: that one needs a device)
    with pytest.raises(ValueError, match="Controller_groups"):
        Simulator.Simulator_batch(8, np.zeros(12), controller=groups)
    with pytest.raises(ValueError, match="Controller_groups"):
        Simulator.check_controller(groups)
    with pytest.raises(ValueError, match="unknown simulator parameters"):
        Simulator.Simulator_batch(8, np.zeros(12), stiffness=1.0)


def test_binding_structures_match_the_header():
    """qrw_sim_params / qrw_sim_buffers field for field, and the state's item count."""
    import re

    import qrw_hip

    text = open(os.path.join(ROOT, "include", "qrw_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} qrw_sim_params;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in qrw_hip._SimParams._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} qrw_sim_buffers;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*(d_[a-z_]+)", body) == [n for n, _ in qrw_hip._SimBuffers._fields_]
    assert int(re.search(r"#define QRW_SIM_STATE_ITEMS (\d+)", text).group(1)) == qrw_hip.SIM_STATE_ITEMS
    kern = open(os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc", "qrw_kernels.h")).read()
    assert int(re.search(r"kSimStItems = (\d+)", kern).group(1)) == qrw_hip.SIM_STATE_ITEMS
