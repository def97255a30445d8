"""GPU tests of the batched rigid-body simulator (sim_kernel.hip through the C ABI, Simulator.Simulator_batch and the drop-in
PyBulletSimulator.py) against the numpy checker tests/sim_numpy.py, which solves the dense 18x18 system of the CPU oracle's
crba / rnea / feet_jacobians where the device uses a per-leg Schur complement onto the base's 6x6.

Tolerance.  Not taken over from the estimator: an 18x18 solve sits between the inputs and the results.  The checker was held
against itself on the states of this file (fd_spread / tick_spread below; scripts/sim_tolerance.py prints them):
  forward dynamics, the 17 states of _fd_states() with and without the external wrench: float64 solve against a longdouble solve
      1.15e-15, every input moved by one ulp 1.33e-13 (relative to max(1, |a|_inf) of the state)  -> FD_SPREAD 1.33e-13, FD_BOUND 1.33e-11
  one tick (8 sub-steps), the 60 x 17 ticks of the checker's free run of _tick_case(): the state at the start of the tick moved by
      one ulp, every state item and output relative to max(1, |item|_inf): 3.53e-11             -> TICK_SPREAD 3.53e-11, TICK_BOUND 3.53e-9
      (that free run's smallest |d| is 5.5e-7 and it sees 0, 1, 2, 3 and 4 feet in contact)
The bounds are 100 x the spreads: the margin covers the different summation order of the quad form.  Beside them a residual
check that does not depend on the conditioning: the device's a and f through oracle.rnea and J'f return [0; tau] within
RESIDUAL_EPS machine epsilons of |M| |a| + |h|, row by row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FD_SPREAD, FD_BOUND = 1.33e-13, 1.33e-11
TICK_SPREAD, TICK_BOUND = 3.53e-11, 3.53e-9
RESIDUAL_EPS = 64  # multiples of 2^-52: ~20 operations deep per row in either evaluation order
MIN_ABS_D = 1e-9   # the contact law switches at d = 0: no state of these tests may come nearer, so that no robot is excused
B17 = 17           # two wavefronts, the second holding one quad
STATE_KEYS = ("q", "v", "prev_o_imuVel")
OUT_KEYS = ("q_mes", "v_mes", "quat", "ang_vel", "lin_acc", "o_imu_vel", "true_pos", "true_b_vel", "contact_forces", "joint_torques")


def _t(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


@pytest.fixture(scope="module")
def sn(oracle_mod):
    import sim_numpy

    return sim_numpy


def _rpy_quat(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def _fd_states(sn, n=B17, seed=11):
    """(q19, v18, tau12, f_ext, wanted contacts or None) x n: the named corners first, random states near the ground after."""
    rng = np.random.default_rng(seed)
    level, Q = np.array([0.0, 0.0, 0.0, 1.0]), sn.Q_STANCE
    z18 = np.zeros(18)
    one_leg = Q.copy()
    one_leg[6:9] = [0.0, 0.1, -0.2]  # HL nearly straight: its foot 0.32 below the base, the others 0.245
    fast = np.concatenate([0.3 * rng.normal(size=6), rng.uniform(-20.0, 20.0, 12)])
    fast[6 + 4] = 20.0
    corners = [
        (np.concatenate([[0.3, -0.2, 0.5], _rpy_quat(0.3, -0.2, 1.0), Q + 0.2 * rng.normal(size=12)]), rng.normal(size=18), 0),  # airborne
        (np.concatenate([[0.0, 0.0, 0.235], level, Q]), z18, 4),                                                               # four feet
        (np.concatenate([[0.0, 0.0, 0.245], _rpy_quat(0.02, -0.03, 0.4), Q]), 0.3 * rng.normal(size=18), 4),                   # ... moving
        (np.concatenate([[0.0, 0.0, 0.30], level, one_leg]), 0.2 * rng.normal(size=18), 1),                                     # one foot
        (np.concatenate([[0.0, 0.0, 0.15], level, Q]), 0.5 * rng.normal(size=18), 4),                                           # deep penetration
        (np.concatenate([[0.0, 0.0, 0.25], level, Q]), np.concatenate([[1.0, -0.5, 0.0], np.zeros(15)]), 4),                    # sliding >> vs
        (np.concatenate([[0.0, 0.0, 0.25], level, Q]), np.concatenate([[1e-5, 2e-5, 0.0], np.zeros(15)]), 4),                   # sliding << vs
        (np.concatenate([[1.0, 2.0, 0.24], _rpy_quat(0.2, -0.15, np.pi - 0.01), Q]), 0.5 * rng.normal(size=18), None),         # tilted, yaw ~ +pi
        (np.concatenate([[1.0, 2.0, 0.24], _rpy_quat(-0.25, 0.1, -np.pi + 0.01), Q]), 0.5 * rng.normal(size=18), None),        # tilted, yaw ~ -pi
        (np.concatenate([[0.0, 0.0, 0.25], level, Q + 0.1 * rng.normal(size=12)]), fast, None),                                 # joint speeds to 20 rad/s
    ]
    states = []
    for i in range(n):
        if i < len(corners):
            q, v, want = corners[i]
        else:
            quat = rng.normal(size=4) * [0.15, 0.15, 1.0, 1.0]
            q = np.concatenate([rng.normal(size=2), [0.22 + 0.03 * rng.normal()], quat / np.linalg.norm(quat), Q + 0.3 * rng.normal(size=12)])
            v, want = np.concatenate([0.5 * rng.normal(size=6), 3.0 * rng.normal(size=12)]), None
        states.append((q, np.array(v, dtype=float), rng.normal(size=12), rng.normal(size=6) * [3.0, 3.0, 3.0, 0.3, 0.3, 0.3], want))
    return states


def fd_spread(sn, states, prm=None):
    """The checker against itself: float64 against longdouble solve, and every input moved up by one ulp; relative to max(1, |a|_inf).
    prm: the contact parameters (None: the defaults)."""
    solve, ulp = 0.0, 0.0
    prm = sn.DEFAULTS if prm is None else dict(sn.DEFAULTS, **prm)
    for q, v, tau, fe, _ in states:
        for f_ext in (None, fe):
            a, _, _ = sn.forward_dynamics(q, v, tau, prm, f_ext=f_ext)
            al, _, _ = sn.forward_dynamics(q, v, tau, prm, f_ext=f_ext, solve=sn.solve_longdouble)
            qp = np.nextafter(q, np.inf)
            qp[3:7] = q[3:7]  # (the quaternion stays a unit one)
            ap, _, _ = sn.forward_dynamics(qp, np.nextafter(v, np.inf), np.nextafter(tau, np.inf), prm, f_ext=f_ext)
            scale = max(1.0, np.abs(a).max())
            solve = max(solve, float(np.abs(a - np.asarray(al, dtype=float)).max()) / scale)
            ulp = max(ulp, np.abs(a - ap).max() / scale)
    return solve, ulp


def _rel(got, ref):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() / max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ forward dynamics
@pytest.mark.parametrize("n", [B17, 1])
@pytest.mark.parametrize("with_f_ext", [False, True])
def test_forward_dynamics_matches_the_checker(oracle_mod, sn, n, with_f_ext):
    """qrw_test_sim_forward_dynamics on the corner states (n = 1: the moving four-feet state alone), with and without an external
    wrench: accelerations within FD_BOUND of the checker's dense solve, contact forces within FD_BOUND, and the residual
    rnea(q, v, a) - J'f - [0; tau] - wrench within RESIDUAL_EPS epsilons of |M| |a| + |h| row by row."""
    import qrw_hip

    states = _fd_states(sn) if n == B17 else _fd_states(sn)[2:3]
    eng = qrw_hip.Batch(2)
    fe = np.stack([s[3] for s in states]) if with_f_ext else None
    a_dev, f_dev = eng.test_sim_forward_dynamics(np.stack([s[0] for s in states]), np.stack([s[1] for s in states]),
                                                 np.stack([s[2] for s in states]), f_ext=fe)
    worst = 0.0
    for i, (q, v, tau, fx, want) in enumerate(states):
        f_ext = fx if with_f_ext else None
        a, f, d = sn.forward_dynamics(q, v, tau, f_ext=f_ext)
        assert np.abs(d).min() > MIN_ABS_D, (i, d)
        if want is not None:
            assert int((d > 0).sum()) == want, (i, d)
        worst = max(worst, _rel(a_dev[i], a))
        assert _rel(a_dev[i], a) <= FD_BOUND, (i, _rel(a_dev[i], a))
        assert _rel(f_dev[i], f) <= FD_BOUND, (i, _rel(f_dev[i], f))
        J, M, h = oracle_mod.feet_jacobians(q), oracle_mod.crba(q), oracle_mod.rnea(q, v, np.zeros(18))
        rhs = sn.rhs_of(q, v, tau, f_dev[i], J, f_ext) + h  # [0; tau] + J'f + wrench
        res = oracle_mod.rnea(q, v, a_dev[i]) - rhs
        scale = np.abs(M) @ np.abs(a_dev[i]) + np.abs(h) + np.abs(J.T) @ np.abs(f_dev[i].ravel())
        assert np.all(np.abs(res) <= RESIDUAL_EPS * 2.0 ** -52 * scale), (i, np.abs(res / scale).max() / 2.0 ** -52)
    print("forward dynamics n=%d f_ext=%s: worst relative error %.3g (bound %.3g)" % (n, with_f_ext, worst, FD_BOUND))
    if n == B17:
        contacts = [int((sn.forward_dynamics(q, v, tau)[2] > 0).sum()) for q, v, tau, _, _ in states]
        assert {0, 1, 4} <= set(contacts), contacts


# ------------------------------------------------------------------------------------------------ teacher-forced ticks
def _tick_case(sn, B=B17, seed=3):
    rng = np.random.default_rng(seed)
    q0 = np.zeros((B, 19))
    q0[:, 2] = rng.uniform(0.235, 0.275, B)  # from feet pressed into the ground to feet just above it
    q0[:, 3:7] = [_rpy_quat(*(0.05 * rng.normal(size=2)), rng.uniform(-np.pi, np.pi)) for _ in range(B)]
    q0[:, 7:] = sn.Q_STANCE + 0.1 * rng.normal(size=(B, 12))
    phase, amp = rng.uniform(0, 2 * np.pi, (B, 12)), rng.uniform(0.0, 0.25, (B, 1))

    def command(k):
        P = np.full((B, 12), 3.0) + 0.5 * np.sin(0.3 * k + phase[:, :1])
        D = np.full((B, 12), 0.2)
        q_des = sn.Q_STANCE + amp * np.sin(0.21 * k + phase)
        v_des = amp * np.cos(0.21 * k + phase)
        tau_ff = 0.3 * np.sin(0.17 * k + 2.0 * phase)
        f_ext = None if k % 2 == 0 else np.tile([2.0 * np.sin(0.1 * k), 1.0, -1.0, 0.1, -0.1, 0.05], (B, 1)) * amp * 4.0
        return P, D, q_des, v_des, tau_ff, f_ext

    return q0, command


def tick_spread(sn, B=B17, ticks=60, **params):
    """The checker against itself over its own free run of the teacher-forced case: every tick once more from the state moved up by
    one ulp (the quaternion kept); largest difference of a state item or output relative to max(1, |item|_inf).  Also the
    smallest |d| of the run and the numbers of feet in contact it saw.  params: simulator parameters other than the defaults."""
    q0, command = _tick_case(sn, B)
    spread, smallest, seen = 0.0, np.inf, set()
    for b in range(B):
        r, p = sn.SimNumpy(q0[b], **params), sn.SimNumpy(q0[b], **params)
        for k in range(ticks):
            c = [x if x is None else x[b] for x in command(k)]
            qp = np.nextafter(r.q, np.inf)
            qp[3:7] = r.q[3:7]
            p.set_state(qp, np.nextafter(r.v, np.inf), np.nextafter(r.prev, np.inf), r.tick)
            r.step(*c)
            p.step(*c)
            seen.add(int((r.out["contact_forces"][:, 2] > 0).sum()))
            for x, y in [(r.q, p.q), (r.v, p.v), (r.prev, p.prev)] + [(r.out[n], p.out[n]) for n in OUT_KEYS]:
                spread = max(spread, _rel(y, x))
        smallest = min(smallest, r.min_abs_d, p.min_abs_d)
    return spread, smallest, seen


def _compare_tick(got_state, got_out, refs, k, bound=TICK_BOUND):
    worst = 0.0
    for b, r in enumerate(refs):
        assert r.status == 0 and got_state["status"][b] == 0 and got_state["tick"][b] == r.tick, (k, b)
        for name, ref in (("q", r.q), ("v", r.v), ("prev_o_imuVel", r.prev)):
            e = _rel(got_state[name][b], ref)
            worst = max(worst, e)
            assert e <= bound, (name, k, b, e)
        for name in OUT_KEYS:
            e = _rel(got_out[name][b], r.out[name])
            worst = max(worst, e)
            assert e <= bound, (name, k, b, e)
    return worst


def test_teacher_forced_ticks_match_the_checker(oracle_mod, sn):
    """60 ticks at B = 17 under PD commands that change every tick (an external wrench on the odd ones): each tick the checker
    starts from the device's previous state; every state item and every output compared after each tick, zero robots left out.
    The checker's smallest |d| stays above MIN_ABS_D, so no comparison sits on the contact law's switch."""
    import torch

    import qrw_hip

    q0, command = _tick_case(sn)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    eng.sim_init(_t(q0), out)
    refs = [sn.SimNumpy(q0[b]) for b in range(B17)]
    st = eng.sim_state()
    host = {n: out[n].cpu().numpy() for n in OUT_KEYS}
    worst = _compare_tick(st, host, refs, -1)
    in_contact = set()
    for k in range(60):
        P, D, q_des, v_des, tau_ff, f_ext = command(k)
        for b, r in enumerate(refs):
            r.set_state(st["q"][b], st["v"][b], st["prev_o_imuVel"][b], st["tick"][b])
            r.step(P[b], D[b], q_des[b], v_des[b], tau_ff[b], None if f_ext is None else f_ext[b])
            in_contact.add(int((r.out["contact_forces"][:, 2] > 0).sum()))
        eng.sim_step(_t(P), _t(D), _t(q_des), _t(v_des), _t(tau_ff), out, f_ext=None if f_ext is None else _t(f_ext))
        torch.cuda.synchronize()
        st = eng.sim_state()
        host = {n: out[n].cpu().numpy() for n in OUT_KEYS}
        worst = max(worst, _compare_tick(st, host, refs, k))
    smallest = min(r.min_abs_d for r in refs)
    print("teacher-forced ticks: worst relative error %.3g (bound %.3g), smallest |d| %.3g, feet in contact seen %s"
          % (worst, TICK_BOUND, smallest, sorted(in_contact)))
    assert smallest > MIN_ABS_D, smallest
    assert {0, 4} <= in_contact, in_contact


# ------------------------------------------------------------------------------------------------ init / get / set
def _run(eng, out, command, ticks, k0=0):
    import torch

    rec = []
    for k in range(k0, k0 + ticks):
        P, D, q_des, v_des, tau_ff, f_ext = command(k)
        eng.sim_step(_t(P), _t(D), _t(q_des), _t(v_des), _t(tau_ff), out, f_ext=None if f_ext is None else _t(f_ext))
        torch.cuda.synchronize()
        st = eng.sim_state()
        rec.append([st[n].copy() for n in STATE_KEYS + ("tick", "status")] + [out[n].cpu().numpy() for n in OUT_KEYS])
    return rec


def _same(rec_a, rec_b, rows=slice(None)):
    assert len(rec_a) == len(rec_b)
    for k, (a, b) in enumerate(zip(rec_a, rec_b)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x[rows], y[rows]), (k, i)


@pytest.mark.parametrize("substeps", [1, 8])
def test_init_get_set_round_trip(oracle_mod, sn, substeps):
    """Re-initialisation restores the first ticks bit for bit; a state read with get and written back with set (into a second
    handle, whose own state was something else) continues bit for bit; 1 and 8 sub-steps both work and differ."""
    import qrw_hip

    q0, command = _tick_case(sn, seed=4)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    eng.sim_init(_t(q0), out, substeps=substeps)
    first = [out[n].cpu().numpy() for n in OUT_KEYS]
    st0 = eng.sim_state()
    assert np.array_equal(st0["q"], q0) and not st0["v"].any() and not st0["prev_o_imuVel"].any() and not st0["tick"].any()
    assert np.array_equal(first[0], q0[:, 7:]) and not first[4].any() and not first[8].any()  # q_mes; lin_acc, contact forces zero
    a = _run(eng, out, command, 6)
    assert all(np.all(np.isfinite(x)) for x in a[-1]) and np.array_equal(a[-1][3], np.full(B17, 6)) and not a[-1][4].any()
    eng.sim_init(_t(q0), out, substeps=substeps)
    assert all(np.array_equal(x, out[n].cpu().numpy()) for x, n in zip(first, OUT_KEYS))
    _same(a, _run(eng, out, command, 6))
    # 12-joint initialisation: the base level at base_height
    eng.sim_init(_t(q0[:, 7:]), out, substeps=substeps, base_height=0.3)
    st = eng.sim_state()
    assert np.array_equal(st["q"][:, :7], np.tile([0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 1.0], (B17, 1))) and np.array_equal(st["q"][:, 7:], q0[:, 7:])
    # get -> set into another handle after 3 ticks
    other = qrw_hip.Batch(B17)
    out2 = other.sim_outputs()
    other.sim_init(_t(q0[::-1].copy()), out2, substeps=substeps)
    other.sim_set_state(a[2][0], a[2][1], a[2][2], tick=a[2][3])
    _same(a[3:], _run(other, out2, command, 3, k0=3))
    if substeps == 8:
        eng.sim_init(_t(q0), out, substeps=1)
        assert not np.array_equal(_run(eng, out, command, 1)[0][0], a[0][0])


def test_nan_command_freezes_one_robot_only(oracle_mod, sn):
    """A NaN tau_ff for robot 5 on tick 2 of 5: its status is set, its state, tick counter and outputs keep the values of tick 1
    through the later (clean) ticks; the other 16 are bit-identical to the run without the NaN."""
    import qrw_hip

    q0, command = _tick_case(sn, seed=5)

    def poisoned(k):
        c = list(command(k))
        if k == 2:
            c[4] = c[4].copy()
            c[4][5, 7] = np.nan
        return tuple(c)

    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    eng.sim_init(_t(q0), out)
    clean = _run(eng, out, command, 5)
    eng.sim_init(_t(q0), out)
    bad = _run(eng, out, poisoned, 5)
    others = np.arange(B17) != 5
    _same(clean, bad, rows=others)
    assert not clean[-1][4].any()
    for k in range(5):
        status = bad[k][4]
        assert status[5] == (1 if k >= 2 else 0) and not status[others].any(), (k, status)
        if k >= 2:  # frozen at what tick 1 left
            for i, (x, y) in enumerate(zip(bad[k], bad[1])):
                if i != 4:
                    assert np.array_equal(x[5], y[5]) and np.all(np.isfinite(x[5])), (k, i)


# ------------------------------------------------------------------------------------------------ fleet
Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])  # scripts/main_solo12_control.py:120
H_INIT = 0.22294615


def _closed_loop(ctl, vref, ticks, sim=None, on_loop_stream=False):
    """sim.step(ctl.result); ctl.compute_sensors(joy, **sim.sensors) -- or (sim None) the raw entry points on ctl's handle in the same
    order.  Returns per tick the result tensor, the error flags, the estimator's q_filt and the simulator's outputs."""
    import contextlib

    import torch

    vr, rec = _t(vref), []
    if sim is None:
        b = ctl._b
        out = b.sim_outputs()
        b.sim_init(_t(np.tile(Q_INIT, (ctl.B, 1))), out)
        sensors = {n: out[n] for n in ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")}
    else:
        out, sensors = sim.out, sim.sensors
    ctx = (lambda: torch.cuda.stream(ctl.loop_stream)) if on_loop_stream else contextlib.nullcontext
    with ctx():
        r = ctl.compute_sensors(vr, **sensors)
        for _ in range(ticks):
            if sim is None:
                ctl._b.sim_step(r.P, r.D, r.q_des, r.v_des, r.tau_ff, out)
            else:
                sim.step(r)
            r = ctl.compute_sensors(vr, **sensors)
            torch.cuda.current_stream().synchronize()
            rec.append([x.cpu().numpy().copy() for x in [ctl._res["result"], ctl.error_flag, ctl.q_filt] + [out[n] for n in OUT_KEYS]])
    return rec


def test_fleet_step_is_the_raw_entry_points(oracle_mod):
    """Simulator_batch.step + compute_sensors over 25 ticks (three solves) at B = 8: bit for bit qrw_sim_init / qrw_sim_step called
    on the controller's handle in the same order; the simulated robots respond (contact forces, moving joints) and stay finite."""
    from Controller import Controller_batch
    from Simulator import Simulator_batch

    B, T = 8, 25
    vref = np.zeros((B, 6))
    vref[:, 0] = np.linspace(0.0, 0.2, B)
    ctl = Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT))
    sim = Simulator_batch(B, Q_INIT, controller=ctl)
    a = _closed_loop(ctl, vref, T, sim)
    assert not sim.status.any() and np.array_equal(sim.state()["tick"], np.full(B, T))
    b = _closed_loop(Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT)), vref, T)
    _same(a, b)
    assert all(np.all(np.isfinite(x)) for rec in a for x in rec)
    pressed = np.max([rec[3 + 8][:, :, 2].max(axis=1) for rec in a], axis=0)  # every robot's largest normal force over the run
    assert pressed.min() > 1.0 and np.abs(a[-1][3 + 1]).max() > 0, pressed
    # a simulator with a handle of its own gives the same robots
    ctl2 = Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT))
    _same(a, _closed_loop(ctl2, vref, T, Simulator_batch(B, Q_INIT)))


def test_fleet_asynchronous_mode_on_the_loop_stream():
    """multiprocessing=True, mpc_lag=3: the loop stepped under `with torch.cuda.stream(ctl.loop_stream)` against the same controller
    stepped from the caller's stream (compute_sensors hands over between the two), bit for bit."""
    import torch
    from Controller import Controller_batch
    from Simulator import Simulator_batch

    B, T = 8, 25
    vref = np.zeros((B, 6))
    vref[:, 0] = np.linspace(0.0, 0.2, B)
    with torch.cuda.stream(torch.cuda.Stream()):
        ca = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=dict(h_init=H_INIT))
        assert ca.loop_stream is not None
        sa = Simulator_batch(B, Q_INIT, controller=ca)
        torch.cuda.current_stream().synchronize()
        a = _closed_loop(ca, vref, T, sa, on_loop_stream=True)
        ca.stop_parallel_loop()
        cb = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=dict(h_init=H_INIT))
        b = _closed_loop(cb, vref, T, Simulator_batch(B, Q_INIT, controller=cb))
        cb.stop_parallel_loop()
    _same(a, b)


# ------------------------------------------------------------------------------------------------ drop-in
def test_dropin_matches_the_checker(oracle_mod, sn):
    """PyBulletSimulator (batch-1 handle, host buffers) against the checker for 50 ticks in the reference's order of calls:
    UpdateMeasurment, SetDesired*, SendCommand."""
    import PyBulletSimulator as P

    dev = P.PyBulletSimulator()
    dev.Init(q_init=Q_INIT, dt=0.002)
    ref = sn.SimNumpy(Q_INIT)
    rng = np.random.default_rng(8)
    worst = 0.0
    for k in range(50):
        dev.UpdateMeasurment()
        o = ref.out
        for got, want in ((dev.q_mes, o["q_mes"]), (dev.v_mes, o["v_mes"]), (dev.baseOrientation, o["quat"]),
                          (dev.baseAngularVelocity, o["ang_vel"]), (dev.baseLinearAcceleration, o["lin_acc"]),
                          (dev.o_imuVel.ravel(), o["o_imu_vel"]), (dev.dummyPos, o["true_pos"]), (dev.b_baseVel, o["true_b_vel"]),
                          (dev.torquesFromCurrentMeasurment, o["joint_torques"]), (dev.contact_forces, o["contact_forces"])):
            worst = max(worst, _rel(got, want))
        assert worst <= TICK_BOUND, (k, worst)
        assert np.allclose(dev.baseAccelerometer, dev.baseLinearAcceleration + dev.rot_oMb.T @ [0.0, 0.0, -9.81])
        q_des, tau = Q_INIT + 0.1 * np.sin(0.2 * k + np.arange(12)), 0.2 * rng.normal(size=12)
        dev.SetDesiredJointPDgains(3.0 * np.ones(12), 0.2 * np.ones(12))
        dev.SetDesiredJointPosition(q_des)
        dev.SetDesiredJointVelocity(np.zeros(12))
        dev.SetDesiredJointTorque(tau)
        st = dev._b.sim_state()  # teacher-forced, as the ticks above: the checker steps from the device's state
        ref.set_state(st["q"][0], st["v"][0], st["prev_o_imuVel"][0], st["tick"][0])
        dev.SendCommand(WaitEndOfCycle=False)
        ref.step(3.0, 0.2, q_des, np.zeros(12), tau)
    print("drop-in: worst relative error over 50 ticks %.3g (bound %.3g)" % (worst, TICK_BOUND))
    assert dev.status == 0 and dev._b.sim_state()["tick"][0] == 50 and ref.min_abs_d > MIN_ABS_D and abs(dev.hardware.yaw) < 0.1
    dev.Stop()


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_handle_usable(sn):
    """Step / get / set before init, a q_init of the wrong width, bad parameters, NULL outputs, a wrong batch: refused with -1 (or by
    the binding) and a text that names the entry point; the next valid call works."""
    import ctypes as C

    import qrw_hip

    B = 3
    eng = qrw_hip.Batch(B)
    out = eng.sim_outputs()
    cmd = [_t(np.full((B, 12), x)) for x in (3.0, 0.2, 0.0, 0.0, 0.0)]
    cmd[2] = _t(np.tile(Q_INIT, (B, 1)))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_sim_step: simulator not initialised"):
        eng.sim_step(*cmd, out)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_sim_get_host: simulator not initialised"):
        eng.sim_state()
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_sim_step_host: simulator not initialised"):
        eng.sim_step_host(3.0, 0.2, Q_INIT, 0.0, 0.0)
    q = _t(np.tile(Q_INIT, (B, 1)))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_sim_init: dt must be > 0 and substeps"):
        eng.sim_init(q, out, substeps=0)
    with pytest.raises(qrw_hip.QrwError, match="bad shape"):
        eng.sim_init(_t(np.tile(Q_INIT, (B + 1, 1))), out)
    prm, bufs = qrw_hip.sim_params(), eng._sim_buffers(out)
    rc = eng._lib.qrw_sim_init(eng._handle, q.data_ptr(), 13, C.byref(prm), C.byref(bufs), None)
    assert rc == -1 and eng._lib.qrw_last_error().decode().startswith("qrw_sim_init: q_ld")
    bufs.d_quat = None
    rc = eng._lib.qrw_sim_init(eng._handle, q.data_ptr(), 12, C.byref(prm), C.byref(bufs), None)
    assert rc == -1 and eng._lib.qrw_last_error().decode() == "qrw_sim_init: null output buffer"
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_sim_step: simulator not initialised"):
        eng.sim_step(*cmd, out)  # (none of the refused initialisations counted)
    eng.sim_init(q, out)
    rc = eng._lib.qrw_sim_step(eng._handle, *[c.data_ptr() for c in cmd], 12, None, C.byref(bufs), eng._stream())
    assert rc == -1 and eng._lib.qrw_last_error().decode() == "qrw_sim_step: null output buffer"
    rc = eng._lib.qrw_sim_step(eng._handle, None, *[c.data_ptr() for c in cmd[1:]], 12, None, C.byref(eng._sim_buffers(out)), eng._stream())
    assert rc == -1 and eng._lib.qrw_last_error().decode() == "qrw_sim_step: null input"
    with pytest.raises(qrw_hip.QrwError, match="bad shape"):
        eng.sim_step(*cmd, out, f_ext=_t(np.zeros((B, 3))))
    eng.sim_step(*cmd, out)
    st = eng.sim_state()
    assert np.array_equal(st["tick"], np.ones(B)) and not st["status"].any() and np.all(np.isfinite(st["q"]))
    ref = sn.SimNumpy(Q_INIT)
    ref.step(3.0, 0.2, Q_INIT, np.zeros(12), np.zeros(12))
    assert _rel(st["q"][1], ref.q) <= TICK_BOUND and _rel(st["v"][1], ref.v) <= TICK_BOUND
