"""GPU tests of the simulator's heightfield terrain (the terrain instantiation of sim_kernel.hip through qrw_sim_set_terrain and
Simulator.Simulator_batch(terrain=...)) against the numpy checker tests/sim_terrain_numpy.py, which puts its own restatement of
the contact law under the dense 18x18 solve of tests/sim_numpy.py.

Tolerance, as measured (scripts/sim_terrain_tolerance.py prints these; the method and the margin are those of
tests/test_gpu_sim.py): the checker against itself with every input moved by one ulp,
  forward dynamics, the 2 x 17 states of _fd_states() (rough field and ramp) with and without the external wrench, relative to
      max(1, |a|_inf): float64 against longdouble solve 6.29e-16, one ulp 5.14e-14           -> FD_SPREAD 5.14e-14, FD_BOUND 5.14e-12
  one tick (8 sub-steps), the 60 x 17 ticks of the checker's free run of _tick_case(), every state item and output relative to
      max(1, |item|_inf): 1.24e-11                                                          -> TICK_SPREAD 1.24e-11, TICK_BOUND 1.24e-9
      (that free run's smallest |d| is 1.0e-7, its smallest |fu - fv| 1.6e-6, its smallest distance of fu, fv to 0 or 1 3.4e-7; it
      sees 0, 1, 2, 3 and 4 feet in contact and both triangle kinds)
The bounds are 100 x the spreads.  The law switches at d = 0, on the cell edges and on the diagonal: every test asserts, for
every foot of every state it compares, |d| > 1e-9, |fu - fv| > 1e-9 and fu, fv in (1e-9, 1 - 1e-9), so that no comparison sits on
a switch and no robot is excused; only the states put outside the field on purpose are exempt from the last condition (their
fu or fv is pinned to exactly 0 or 1)."""
import numpy as np
import pytest

from test_gpu_sim import B17, H_INIT, OUT_KEYS, Q_INIT, RESIDUAL_EPS, _rel, _rpy_quat, _run, _same, _t

pytestmark = pytest.mark.gpu

FD_SPREAD, FD_BOUND = 5.14e-14, 5.14e-12
TICK_SPREAD, TICK_BOUND = 1.24e-11, 1.24e-9
MIN_SWITCH = 1e-9  # no |d|, |fu - fv| or distance of fu, fv to a cell edge of these tests may come nearer to a switch of the law
LEVEL = np.array([0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def stn(oracle_mod):
    import sim_terrain_numpy

    return sim_terrain_numpy


# ------------------------------------------------------------------------------------------------ fields and states
def rough_field(stn, seed=21):
    """9 x 9 cells of 0.05 m with heights to 0.05 m, centred on the origin."""
    return stn.Terrain(np.random.default_rng(seed).uniform(0.0, 0.05, (10, 10)), 0.05, 0.05, -0.225, -0.225)


def ramp_field(stn, slope=0.5):
    """h = slope x on 7 x 5 cells of 0.1 m x 0.15 m (rows != cols, dx != dy: a transposed lookup cannot pass)."""
    x = -0.35 + 0.1 * np.arange(8)
    return stn.Terrain(np.tile(slope * x, (6, 1)), 0.1, 0.15, -0.35, -0.375)


def big_field(stn, seed=22):
    return stn.Terrain(np.random.default_rng(seed).uniform(-0.02, 0.03, (24, 20)), 0.04, 0.035, -0.4, -0.42)


FIELDS = {"rough": rough_field, "ramp": ramp_field}


def set_terrain(eng, T, origin=None):
    eng.sim_set_terrain(T.H, T.dx, T.dy, x0=T.x0, y0=T.y0, origin=origin)


def _settle(stn, q, T, origin, delta, deepest=True, prm=None):
    """q with the base height set so that the deepest foot (or, deepest=False, the shallowest one) has d = delta under the
    parameters prm (None: the defaults; only foot_radius enters)."""
    q = q.copy()
    q[2] = 0.0
    _, d0, _ = stn.contact_forces(q, np.zeros(18), stn.DEFAULTS if prm is None else prm, T, origin)
    nz = []
    for j in range(4):  # d is linear in the base height: d = d0 - n_z z
        pf = q[:3] + stn.sn.quat_to_rot(q[3:7]) @ stn.oracle.fixed_feet(q[7:], np.zeros(12))[0][j]
        _, gx, gy, _ = T.surface(pf[0] + origin[0], pf[1] + origin[1])
        nz.append(1.0 / np.sqrt(gx * gx + gy * gy + 1.0))
    z = (d0 - delta) / np.array(nz)
    q[2] = z.max() if deepest else z.min()
    return q


def _fd_states(stn, which, n=B17, seed=13, prm=None):
    """(q19, v18, tau12, f_ext, origin (2,), wanted contacts or None, outside the field) x n on field `which`, settled under the
    parameters prm (None: the defaults)."""
    rng = np.random.default_rng(seed + (0 if which == "rough" else 100))
    T, Q = FIELDS[which](stn), stn.Q_STANCE
    xmax, ymax = T.x0 + T.dx * (T.H.shape[1] - 1), T.y0 + T.dy * (T.H.shape[0] - 1)
    z18 = np.zeros(18)
    one_leg = Q.copy()
    one_leg[6:9] = [0.0, 0.1, -0.2]  # HL nearly straight: its foot 0.32 below the base, the others 0.245
    fast = np.concatenate([0.3 * rng.normal(size=6), rng.uniform(-20.0, 20.0, 12)])
    jig = lambda: rng.uniform(-0.007, 0.007, 2)  # (no foot on a cell edge or a diagonal by construction of the numbers)
    # "level" on the ramp is parallel to it (nose up), so that four feet, one foot and deep penetration mean there what they say
    LEVEL = _rpy_quat(0.0, 0.0, 0.0) if which == "rough" else _rpy_quat(0.0, -np.arctan(0.5), 0.0)

    def q_of(xy, quat, joints):
        return np.concatenate([xy, [0.0], quat, joints])

    def past(side):
        """The base position that puts the feet of the level stance 3 cm past one side of the field (and a bit off the axis)."""
        rel = stn.oracle.fixed_feet(Q, np.zeros(12))[0] @ stn.sn.quat_to_rot(LEVEL).T
        return {"+x": [xmax + 0.03 - rel[:, 0].max(), 0.003], "-x": [T.x0 - 0.03 - rel[:, 0].min(), -0.004],
                "+y": [0.003, ymax + 0.03 - rel[:, 1].max()], "-y": [-0.004, T.y0 - 0.03 - rel[:, 1].min()]}[side]

    far, same = np.array([1.0, 2.0]), q_of(0.3 * jig(), _rpy_quat(0.03, -0.02, 0.05), Q)
    v_same = 0.3 * rng.normal(size=18)
    # (q, v, origin, penetration of the deepest [or shallowest: negative sign convention below] foot, wanted contacts, outside)
    corners = [
        (q_of(jig(), _rpy_quat(0.08, 0.03, 0.1), Q + 0.02 * rng.normal(size=12)), rng.normal(size=18), jig(), -0.2, True, 0, False),  # airborne
        (q_of(jig(), LEVEL, Q), z18, jig(), 0.01, False, 4, False),                                                # four feet on four cells
        (q_of(jig(), _rpy_quat(0.02, -0.03, 0.1), Q), 0.3 * rng.normal(size=18), jig(), 0.004, False, 4, False),   # ... moving
        (q_of(jig(), LEVEL, one_leg), 0.2 * rng.normal(size=18), jig(), 0.01, True, 1, False),                     # one foot
        (q_of(jig(), LEVEL, Q), 0.5 * rng.normal(size=18), jig(), 0.1, True, 4, False),                            # deep penetration
        (q_of(jig(), LEVEL, Q), np.concatenate([[1.0, -0.5, 0.0], np.zeros(15)]), jig(), 0.005, False, 4, False),  # sliding >> vs
        (q_of(jig(), LEVEL, Q), np.concatenate([[1e-5, 2e-5, 0.0], np.zeros(15)]), jig(), 0.005, False, 4, False),  # sliding << vs
        (q_of(far + jig(), _rpy_quat(0.1, -0.08, np.pi - 0.01), Q), 0.5 * rng.normal(size=18), -far, 0.02, True, None, False),   # yaw ~ +pi
        (q_of(far + jig(), _rpy_quat(-0.1, 0.06, -np.pi + 0.01), Q), 0.5 * rng.normal(size=18), -far, 0.02, True, None, False),  # yaw ~ -pi
        (q_of(jig(), LEVEL, Q + 0.1 * rng.normal(size=12)), fast, jig(), 0.01, True, None, False),                 # joint speeds to 20 rad/s
        (q_of(past("+x"), LEVEL, Q), 0.3 * rng.normal(size=18), np.zeros(2), 0.01, True, None, True),     # front feet past +x
        (q_of(past("-x"), LEVEL, Q), 0.3 * rng.normal(size=18), np.zeros(2), 0.01, True, None, True),    # hind feet past -x
        (q_of(past("+y"), LEVEL, Q), 0.3 * rng.normal(size=18), np.zeros(2), 0.01, True, None, True),     # left feet past +y
        (q_of(past("-y"), LEVEL, Q), 0.3 * rng.normal(size=18), np.zeros(2), 0.01, True, None, True),    # right feet past -y
        (same, v_same, np.array([0.0, 0.0]), 0.012, True, None, False),                                            # identical robots ...
        (same, v_same, np.array([0.004, T.dy]), 0.012, True, None, False),                                       # ... one row of cells on
        (same, v_same, np.array([-0.003, -T.dy]), 0.012, True, None, False),                                       # ... and one row back  
    ]
    states = []
    for q, v, origin, delta, deepest, want, outside in corners[:n]:
        origin = np.array(origin, dtype=float)
        q = _settle(stn, q, T, origin, delta, deepest, prm)
        states.append((q, np.array(v, dtype=float), rng.normal(size=12), rng.normal(size=6) * [3.0, 3.0, 3.0, 0.3, 0.3, 0.3], origin, want, outside))
    assert len(states) == n
    return T, states


def check_switches(d, cells, outside=False):
    """No foot near a switch of the law; returns the triangle kinds of the feet in contact."""
    assert np.abs(d).min() > MIN_SWITCH, d
    kinds = set()
    for (r, c, fu, fv), dj in zip(cells, d):
        assert abs(fu - fv) > MIN_SWITCH, (fu, fv)
        inside = all(MIN_SWITCH < f < 1.0 - MIN_SWITCH for f in (fu, fv))
        assert inside or outside, (fu, fv)
        if dj > 0:
            kinds.add("lower" if fu >= fv else "upper")
    return kinds


def check_identical_robots(stn, T, states):
    """The last three states are one robot (the same joints, velocities and pose relative to its own origin; the base heights differ
    with the ground) under three origins that put its feet on three different sets of cells."""
    cells = []
    for q, v, tau, _, origin, _, _ in states[-3:]:
        cells.append([])
        stn.forward_dynamics(q, v, tau, T, origin, cells=cells[-1])
    assert all(np.array_equal(np.delete(states[-3][0], 2), np.delete(s[0], 2)) and np.array_equal(states[-3][1], s[1]) for s in states[-2:])
    assert len({tuple(c[:2] for c in cs) for cs in cells}) == 3, cells


def fd_spread(stn, fields=tuple(FIELDS), prm=None):
    """The checker against itself on the forward-dynamics states of the fields (both by default): float64 against longdouble solve,
    and every input moved up by one ulp (the quaternion kept); relative to max(1, |a|_inf).  prm: parameters other than the
    defaults, under which the states are settled too."""
    solve, ulp = 0.0, 0.0
    prm = stn.DEFAULTS if prm is None else dict(stn.DEFAULTS, **prm)
    for which in fields:
        T, states = _fd_states(stn, which, prm=prm)
        for q, v, tau, fe, origin, _, _ in states:
            for f_ext in (None, fe):
                a, _, _ = stn.forward_dynamics(q, v, tau, T, origin, prm, f_ext=f_ext)
                al, _, _ = stn.forward_dynamics(q, v, tau, T, origin, prm, f_ext=f_ext, solve=stn.sn.solve_longdouble)
                qp = np.nextafter(q, np.inf)
                qp[3:7] = q[3:7]
                ap, _, _ = stn.forward_dynamics(qp, np.nextafter(v, np.inf), np.nextafter(tau, np.inf), T, origin, prm, f_ext=f_ext)
                scale = max(1.0, np.abs(a).max())
                solve = max(solve, float(np.abs(a - np.asarray(al, dtype=float)).max()) / scale)
                ulp = max(ulp, np.abs(a - ap).max() / scale)
    return solve, ulp


def _tick_case(stn, B=B17, seed=7, prm=None):
    """Robots dropped onto / pressed into the rough field under PD commands that change every tick (test_gpu_sim's law); the
    initial heights settled under the parameters prm (None: the defaults)."""
    rng = np.random.default_rng(seed)
    T = rough_field(stn)
    origin = rng.uniform(-0.004, 0.004, (B, 2))
    q0 = np.zeros((B, 19))
    q0[:, :2] = rng.uniform(-0.002, 0.002, (B, 2))
    q0[:, 3:7] = [_rpy_quat(*(0.03 * rng.normal(size=2)), 0.03 * rng.normal()) for _ in range(B)]
    q0[:, 7:] = stn.Q_STANCE + 0.02 * rng.normal(size=(B, 12))
    for b, delta in enumerate(rng.uniform(-0.02, 0.015, B)):  # from the lowest foot 2 cm above the ground to 1.5 cm into it
        q0[b] = _settle(stn, q0[b], T, origin[b], delta, prm=prm)
    phase, amp = rng.uniform(0, 2 * np.pi, (B, 12)), rng.uniform(0.0, 0.25, (B, 1))

    def command(k):
        P = np.full((B, 12), 3.0) + 0.5 * np.sin(0.3 * k + phase[:, :1])
        D = np.full((B, 12), 0.2)
        q_des = stn.Q_STANCE + amp * np.sin(0.21 * k + phase)
        v_des = amp * np.cos(0.21 * k + phase)
        tau_ff = 0.3 * np.sin(0.17 * k + 2.0 * phase)
        f_ext = None if k % 2 == 0 else np.tile([2.0 * np.sin(0.1 * k), 1.0, -1.0, 0.1, -0.1, 0.05], (B, 1)) * amp * 4.0
        return P, D, q_des, v_des, tau_ff, f_ext

    return T, origin, q0, command


def tick_spread(stn, B=B17, ticks=60, seed=7, **params):
    """The checker against itself over its own free run of the teacher-forced case: every tick once more from the state moved up by
    one ulp (the quaternion kept).  Returns the spread, the smallest |d|, |fu - fv| and edge distance of the run (both copies),
    the numbers of feet in contact and the triangle kinds it saw.  params: simulator parameters other than the defaults (the
    initial heights are settled under them)."""
    T, origin, q0, command = _tick_case(stn, B, seed, prm=dict(stn.DEFAULTS, **params) if params else None)
    spread, d_min, diag_min, edge_min, seen, kinds = 0.0, np.inf, np.inf, np.inf, set(), set()
    for b in range(B):
        r, p = stn.SimTerrainNumpy(q0[b], T, origin[b], **params), stn.SimTerrainNumpy(q0[b], T, origin[b], **params)
        for k in range(ticks):
            c = [x if x is None else x[b] for x in command(k)]
            qp = np.nextafter(r.q, np.inf)
            qp[3:7] = r.q[3:7]
            p.set_state(qp, np.nextafter(r.v, np.inf), np.nextafter(r.prev, np.inf), r.tick)
            r.step(*c)
            p.step(*c)
            seen.add(int((np.abs(r.out["contact_forces"]).sum(axis=1) > 0).sum()))
            for x, y in [(r.q, p.q), (r.v, p.v), (r.prev, p.prev)] + [(r.out[n], p.out[n]) for n in OUT_KEYS]:
                spread = max(spread, _rel(y, x))
        assert r.status == 0 and p.status == 0
        d_min, diag_min, edge_min = min(d_min, r.min_abs_d, p.min_abs_d), min(diag_min, r.min_diag, p.min_diag), min(edge_min, r.min_edge, p.min_edge)
        kinds |= r.kinds
    return spread, d_min, diag_min, edge_min, seen, kinds


# ------------------------------------------------------------------------------------------------ forward dynamics
def _compare_fd(oracle_mod, stn, eng, T, states, with_f_ext, bound=FD_BOUND, **params):
    """params: simulator parameters other than the defaults, given to the device and to the checker alike."""
    fe = np.stack([s[3] for s in states]) if with_f_ext else None
    prm = dict(stn.DEFAULTS, **params)
    a_dev, f_dev = eng.test_sim_forward_dynamics(np.stack([s[0] for s in states]), np.stack([s[1] for s in states]),
                                                 np.stack([s[2] for s in states]), f_ext=fe, **params)
    worst, contacts, kinds = 0.0, [], set()
    for i, (q, v, tau, fx, origin, want, outside) in enumerate(states):
        f_ext, cells = (fx if with_f_ext else None), []
        a, f, d = stn.forward_dynamics(q, v, tau, T, origin, prm, f_ext=f_ext, cells=cells)
        kinds |= check_switches(d, cells, outside)
        if outside:
            assert any(fu in (0.0, 1.0) or fv in (0.0, 1.0) for _, _, fu, fv in cells), (i, cells)
        contacts.append(int((d > 0).sum()))
        if want is not None:
            assert contacts[-1] == want, (i, d)
        ea, ef = _rel(a_dev[i], a), _rel(f_dev[i], f)
        print("  state %2d: %d feet in contact, a %.3g f %.3g" % (i, contacts[-1], ea, ef))
        worst = max(worst, ea, ef)
        assert ea <= bound and ef <= bound, (i, ea, ef)
        J, M, h = oracle_mod.feet_jacobians(q), oracle_mod.crba(q), oracle_mod.rnea(q, v, np.zeros(18))
        rhs = stn.sn.rhs_of(q, v, tau, f_dev[i], J, f_ext) + h  # [0; tau] + J'f + wrench, J'f from the device's forces
        res = oracle_mod.rnea(q, v, a_dev[i]) - rhs
        scale = np.abs(M) @ np.abs(a_dev[i]) + np.abs(h) + np.abs(J.T) @ np.abs(f_dev[i].ravel())
        assert np.all(np.abs(res) <= RESIDUAL_EPS * 2.0 ** -52 * scale), (i, np.abs(res / scale).max() / 2.0 ** -52)
    return worst, contacts, kinds


@pytest.mark.parametrize("n", [B17, 1])
@pytest.mark.parametrize("with_f_ext", [False, True])
@pytest.mark.parametrize("which", ["rough", "ramp"])
def test_forward_dynamics_on_terrain_matches_the_checker(oracle_mod, stn, which, n, with_f_ext):
    """qrw_test_sim_forward_dynamics with the handle's terrain and per-robot origins on the corner states of _fd_states (n = 1: the
    moving four-feet state alone): accelerations and forces within FD_BOUND of the checker, the row-by-row residual of
    tests/test_gpu_sim.py with J'f from the device's forces; no foot of any state near a switch of the law."""
    import qrw_hip

    T, states = _fd_states(stn, which)
    if n == 1:
        states = states[2:3]
    eng = qrw_hip.Batch(n)
    set_terrain(eng, T, origin=np.stack([s[4] for s in states]))
    worst, contacts, kinds = _compare_fd(oracle_mod, stn, eng, T, states, with_f_ext)
    print("forward dynamics on %s n=%d f_ext=%s: worst relative error %.3g (bound %.3g)" % (which, n, with_f_ext, worst, FD_BOUND))
    if n == B17:
        assert {0, 1, 4} <= set(contacts), contacts
        assert kinds == {"lower", "upper"} or which == "ramp", kinds  # (both triangles of a ramp's cell are one plane)
        check_identical_robots(stn, T, states)


# ------------------------------------------------------------------------------------------------ teacher-forced ticks
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


@pytest.mark.parametrize("B", [B17, 1])
def test_teacher_forced_ticks_on_the_rough_field(oracle_mod, stn, B):
    """60 ticks on the rough field with per-robot origins: each tick the checker starts from the device's previous state; every
    state item and every output compared after each tick, zero robots left out; the run stays clear of every switch of the law
    and (B = 17) sees 0, 1, 2, 3 and 4 feet in contact and both triangle kinds."""
    import torch

    import qrw_hip

    T, origin, q0, command = _tick_case(stn)
    origin, q0 = origin[:B], q0[:B]
    eng = qrw_hip.Batch(B)
    out = eng.sim_outputs()
    set_terrain(eng, T, origin=origin)
    eng.sim_init(_t(q0), out)
    refs = [stn.SimTerrainNumpy(q0[b], T, origin[b]) for b in range(B)]
    st = eng.sim_state()
    host = {n: out[n].cpu().numpy() for n in OUT_KEYS}
    worst = _compare_tick(st, host, refs, -1)
    in_contact = set()
    for k in range(60):
        P, D, q_des, v_des, tau_ff, f_ext = [x if x is None else x[:B] for x in command(k)]
        for b, r in enumerate(refs):
            r.set_state(st["q"][b], st["v"][b], st["prev_o_imuVel"][b], st["tick"][b])
            r.step(P[b], D[b], q_des[b], v_des[b], tau_ff[b], None if f_ext is None else f_ext[b])
            in_contact.add(int((np.abs(r.out["contact_forces"]).sum(axis=1) > 0).sum()))
        eng.sim_step(_t(P), _t(D), _t(q_des), _t(v_des), _t(tau_ff), out, f_ext=None if f_ext is None else _t(f_ext))
        torch.cuda.synchronize()
        st = eng.sim_state()
        host = {n: out[n].cpu().numpy() for n in OUT_KEYS}
        worst = max(worst, _compare_tick(st, host, refs, k))
    d_min, diag_min, edge_min = (min(getattr(r, n) for r in refs) for n in ("min_abs_d", "min_diag", "min_edge"))
    kinds = set().union(*[r.kinds for r in refs])
    print("teacher-forced ticks on the rough field, B=%d: worst relative error %.3g (bound %.3g); smallest |d| %.3g, |fu - fv| %.3g, "
          "edge distance %.3g; feet in contact seen %s, triangles %s" % (B, worst, TICK_BOUND, d_min, diag_min, edge_min,
                                                                         sorted(in_contact), sorted(kinds)))
    assert min(d_min, diag_min, edge_min) > MIN_SWITCH, (d_min, diag_min, edge_min)
    if B == B17:
        assert in_contact == {0, 1, 2, 3, 4}, in_contact
        assert kinds == {"lower", "upper"}, kinds


# ------------------------------------------------------------------------------------------------ field and offset identities
def _teacher_forced_pair(lead, lead_out, follow, follow_out, command, ticks, shift=0.0, check=None):
    """`lead` runs freely; before every tick `follow` is given lead's state with the base `shift` higher; returns the worst
    relative difference of a state item or output after the tick (heights compared after taking the shift out)."""
    import torch

    worst = 0.0
    for k in range(ticks):
        st = lead.sim_state()
        q = st["q"].copy()
        q[:, 2] += shift
        follow.sim_set_state(q, st["v"], st["prev_o_imuVel"], tick=st["tick"])
        for b in range(len(q) if check else 0):  # (the state every tick starts from is clear of the law's switches)
            check(q[b], st["v"][b])
        cmd = command(k)
        for eng, out in ((lead, lead_out), (follow, follow_out)):
            eng.sim_step(*[_t(x) for x in cmd[:5]], out, f_ext=None if cmd[5] is None else _t(cmd[5]))
        torch.cuda.synchronize()
        a, b = lead.sim_state(), follow.sim_state()
        assert not a["status"].any() and not b["status"].any() and np.array_equal(a["tick"], b["tick"])
        b["q"][:, 2] -= shift
        for x, y in [(a[n], b[n]) for n in ("q", "v", "prev_o_imuVel")] + [(lead_out[n].cpu().numpy(), follow_out[n].cpu().numpy() - (
                np.array([0.0, 0.0, shift]) if n == "true_pos" else 0.0)) for n in OUT_KEYS]:
            for i in range(len(x)):
                worst = max(worst, _rel(y[i], x[i]))
    return worst


def test_constant_fields_are_the_plane(oracle_mod, stn):
    """H = 0 through the terrain instantiation against the flat instantiation (another handle), and H = c against the flat one with
    the base lowered by c: forward dynamics of the rough field's states within FD_BOUND, 10 teacher-forced ticks within
    TICK_BOUND.  The field's x0, y0 and the origins moved by the same amount change nothing at all (H = c: bit for bit)."""
    import qrw_hip

    _, states = _fd_states(stn, "rough")
    _, _, q0, command = _tick_case(stn)
    q0 = q0.copy()
    q0[:, 2] -= 0.02  # (the rough field's robots, now on a plane: lower, so that most of them touch it)
    flat = qrw_hip.Batch(B17)
    flat_out = flat.sim_outputs()
    qs, vs, taus = (np.stack([s[i] for s in states]) for i in range(3))
    qs[:, 2] -= 0.02
    geo = dict(dx=1.5, dy=1.5, x0=-1.4, y0=-0.7)  # 3 x 2 cells that hold every state of the two sets

    def clear_of_switches(q, v, c):
        cells = []
        _, d, _ = stn.contact_forces(q, v, stn.DEFAULTS, stn.Terrain(np.full((3, 4), c), **geo), cells=cells)
        check_switches(d, cells)

    for c in (0.0, 0.0371):
        eng = qrw_hip.Batch(B17)
        out = eng.sim_outputs()
        eng.sim_set_terrain(np.full((3, 4), c), **geo)
        a_ref, f_ref = flat.test_sim_forward_dynamics(qs, vs, taus)
        up = qs.copy()
        up[:, 2] += c
        for i in range(B17):
            clear_of_switches(up[i], vs[i], c)
        a, f = eng.test_sim_forward_dynamics(up, vs, taus)
        worst = max(max(_rel(a[i], a_ref[i]), _rel(f[i], f_ref[i])) for i in range(B17))
        assert worst <= FD_BOUND, (c, worst)
        assert np.abs(f_ref).sum() > 0
        flat.sim_init(_t(q0), flat_out)
        eng.sim_init(_t(q0), out)
        tick = _teacher_forced_pair(flat, flat_out, eng, out, command, 10, shift=c, check=lambda q, v: clear_of_switches(q, v, c))
        print("H = %g against the plane: forward dynamics %.3g (bound %.3g), ticks %.3g (bound %.3g)" % (c, worst, FD_BOUND, tick, TICK_BOUND))
        assert tick <= TICK_BOUND, (c, tick)
        assert np.abs(flat_out["contact_forces"].cpu().numpy()).sum() > 0
        # the same field somewhere else, the origins moved with it: nothing changes
        eng.sim_set_terrain(np.full((3, 4), c), 1.5, 1.5, x0=-1.4 + 7.0, y0=-0.7 - 3.0, origin=np.tile([7.0, -3.0], (B17, 1)))
        a2, f2 = eng.test_sim_forward_dynamics(up, vs, taus)
        assert np.array_equal(a2, a) and np.array_equal(f2, f)


def test_clear_terrain_is_a_handle_that_never_had_one(oracle_mod, stn):
    """qrw_sim_clear_terrain: the ticks after it are bit for bit those of a handle that never had a terrain (and differ from the
    ticks on the terrain)."""
    import qrw_hip

    T, origin, q0, command = _tick_case(stn)
    never, eng = qrw_hip.Batch(B17), qrw_hip.Batch(B17)
    out_n, out = never.sim_outputs(), eng.sim_outputs()
    set_terrain(eng, T, origin=origin)
    eng.sim_init(_t(q0), out)
    on_terrain = _run(eng, out, command, 5)
    eng.sim_clear_terrain()
    eng.sim_init(_t(q0), out)
    never.sim_init(_t(q0), out_n)
    cleared, plain = _run(eng, out, command, 5), _run(never, out_n, command, 5)
    _same(cleared, plain)
    assert not np.array_equal(on_terrain[-1][0], plain[-1][0])
    a, f = eng.test_sim_forward_dynamics(q0, np.zeros((B17, 18)), np.zeros((B17, 12)))
    a_n, f_n = never.test_sim_forward_dynamics(q0, np.zeros((B17, 18)), np.zeros((B17, 12)))
    assert np.array_equal(a, a_n) and np.array_equal(f, f_n)


# ------------------------------------------------------------------------------------------------ init and lifetime
def _inside(stn, states, T):
    """Those of `states` whose four feet are over the field T (at least 8 of them)."""
    keep = []
    for s in states:
        cells = []
        stn.contact_forces(s[0], s[1], stn.DEFAULTS, T, s[4], cells)
        if all(0.0 < f < 1.0 for c in cells for f in c[2:]):
            keep.append(s)
    assert len(keep) >= 8, len(keep)
    return keep


def test_init_on_terrain_and_terrain_lifetime(oracle_mod, stn):
    """12-joint initialisation on terrain: the level base at (0, 0), base_height above the highest ground under its four feet, for
    the checker and the device alike (per robot: the origins differ); q19 initialisation takes the pose as given;
    re-initialisation keeps the terrain (the same ticks bit for bit); a larger field set afterwards, from device tensors, works."""
    import qrw_hip

    T, origin, q0, command = _tick_case(stn)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    set_terrain(eng, T, origin=origin)
    eng.sim_init(_t(q0[:, 7:]), out, base_height=0.27)
    st = eng.sim_state()
    want = np.array([stn.init_height(q0[b, 7:], T, origin[b], 0.27) for b in range(B17)])
    ground = want - 0.27
    assert ground.min() > 0.0 and len(set(ground)) == B17, ground  # (no two robots stand on the same ground)
    assert np.abs(st["q"][:, 2] - want).max() <= 4 * 2.0 ** -52, np.abs(st["q"][:, 2] - want).max()
    assert np.array_equal(st["q"][:, :2], np.zeros((B17, 2))) and np.array_equal(st["q"][:, 3:7], np.tile(LEVEL, (B17, 1)))
    assert np.array_equal(st["q"][:, 7:], q0[:, 7:]) and np.array_equal(out["true_pos"].cpu().numpy(), st["q"][:, :3])
    ref = stn.SimTerrainNumpy(q0[3, 7:], T, origin[3], base_height=0.27)
    assert abs(ref.q[2] - st["q"][3, 2]) <= 4 * 2.0 ** -52
    # q19: as given, whatever the ground
    eng.sim_init(_t(q0), out)
    assert np.array_equal(eng.sim_state()["q"], q0)
    a = _run(eng, out, command, 4)
    eng.sim_init(_t(q0), out)  # (re-initialisation keeps the terrain)
    _same(a, _run(eng, out, command, 4))
    # a larger field, from device tensors this time (reallocation), then forward dynamics against the checker on it
    big = big_field(stn)
    _, states = _fd_states(stn, "rough")
    states = _inside(stn, [(q, v, tau, fe, origin[i], None, False) for i, (q, v, tau, fe, _, _, _) in enumerate(states)], big)
    kept = np.zeros((B17, 2))
    kept[:len(states)] = [s[4] for s in states]  # (state i of the call is looked up at row i of the origins)
    eng.sim_set_terrain(_t(big.H), big.dx, big.dy, x0=big.x0, y0=big.y0, origin=_t(kept))
    worst, contacts, _ = _compare_fd(oracle_mod, stn, eng, big, states, True)
    assert max(contacts) > 0, contacts
    # ... and back to a small one without origins
    set_terrain(eng, T)
    states = _inside(stn, [(q, v, tau, fe, np.zeros(2), None, False) for q, v, tau, fe, _, _, _ in states], T)
    _compare_fd(oracle_mod, stn, eng, T, states, False)


# ------------------------------------------------------------------------------------------------ fleet and freeze
def _fleet_field(stn, B):
    """A field large enough to trot on for 25 ticks, and origins that spread the fleet over it."""
    T = stn.Terrain(np.random.default_rng(31).uniform(0.0, 0.02, (30, 30)), 0.05, 0.05, -0.725, -0.725)
    origin = np.random.default_rng(32).uniform(-0.3, 0.3, (B, 2))
    return T, origin


def _closed_loop(ctl, vref, ticks, T, origin, sim=None, on_loop_stream=False):
    """test_gpu_sim._closed_loop on terrain: sim.step + compute_sensors, or (sim None) the raw entry points on ctl's handle."""
    import contextlib

    import torch

    vr, rec = _t(vref), []
    if sim is None:
        b = ctl._b
        out = b.sim_outputs()
        set_terrain(b, T, origin=origin)
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


def test_fleet_on_terrain_is_the_raw_entry_points(oracle_mod, stn):
    """Simulator_batch(terrain=, terrain_origin=).step + compute_sensors over 25 ticks at B = 8: bit for bit qrw_sim_set_terrain /
    qrw_sim_init / qrw_sim_step on the controller's handle; the robots stand on their own ground (12-joint initialisation) and
    differ from the fleet on the plane."""
    from Controller import Controller_batch
    from Simulator import Simulator_batch

    B, ticks = 8, 25
    T, origin = _fleet_field(stn, B)
    terrain = dict(heights=T.H, dx=T.dx, dy=T.dy, x0=T.x0, y0=T.y0)
    vref = np.zeros((B, 6))
    vref[:, 0] = np.linspace(0.0, 0.2, B)
    ctl = Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT))
    sim = Simulator_batch(B, Q_INIT, controller=ctl, terrain=terrain, terrain_origin=origin)
    z0 = sim.state()["q"][:, 2]
    want = np.array([stn.init_height(Q_INIT, T, origin[b]) for b in range(B)])
    assert np.abs(z0 - want).max() <= 4 * 2.0 ** -52 and len(set(z0)) == B
    a = _closed_loop(ctl, vref, ticks, T, origin, sim)
    assert not sim.status.any() and np.array_equal(sim.state()["tick"], np.full(B, ticks))
    b = _closed_loop(Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT)), vref, ticks, T, origin)
    _same(a, b)
    assert all(np.all(np.isfinite(x)) for rec in a for x in rec)
    pressed = np.max([rec[3 + 8][:, :, 2].max(axis=1) for rec in a], axis=0)
    assert pressed.min() > 1.0, pressed
    ctl2 = Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT))
    plane = _closed_loop(ctl2, vref, ticks, T, origin, Simulator_batch(B, Q_INIT, controller=ctl2))
    assert not np.array_equal(plane[-1][3], a[-1][3])
    with pytest.raises(ValueError, match="terrain=: unknown keys"):
        Simulator_batch(B, Q_INIT, terrain=dict(terrain, dz=1.0))
    with pytest.raises(ValueError, match="terrain_origin= without terrain="):
        Simulator_batch(B, Q_INIT, terrain_origin=origin)


def test_fleet_on_terrain_asynchronous_mode_on_the_loop_stream(oracle_mod, stn):
    """multiprocessing=True, mpc_lag=3 on terrain: the loop stepped under `with torch.cuda.stream(ctl.loop_stream)` against the same
    controller stepped from the caller's stream, bit for bit (the terrain, set on the caller's stream, is in place for both)."""
    import torch
    from Controller import Controller_batch
    from Simulator import Simulator_batch

    B, ticks = 8, 25
    T, origin = _fleet_field(stn, B)
    terrain = dict(heights=_t(T.H), dx=T.dx, dy=T.dy, x0=T.x0, y0=T.y0)
    vref = np.zeros((B, 6))
    vref[:, 0] = np.linspace(0.0, 0.2, B)
    with torch.cuda.stream(torch.cuda.Stream()):
        ca = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=dict(h_init=H_INIT))
        assert ca.loop_stream is not None
        sa = Simulator_batch(B, Q_INIT, controller=ca, terrain=terrain, terrain_origin=_t(origin))
        torch.cuda.current_stream().synchronize()
        a = _closed_loop(ca, vref, ticks, T, origin, sa, on_loop_stream=True)
        ca.stop_parallel_loop()
        cb = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=dict(h_init=H_INIT))
        b = _closed_loop(cb, vref, ticks, T, origin, Simulator_batch(B, Q_INIT, controller=cb, terrain=terrain, terrain_origin=_t(origin)))
        cb.stop_parallel_loop()
    _same(a, b)
    assert np.abs(a[-1][3 + 8]).sum() > 0


def test_nan_command_on_terrain_freezes_one_robot_only(oracle_mod, stn):
    """A NaN tau_ff for robot 5 on tick 2 of 5, on the rough field: its status is set and its state and outputs keep the values of
    tick 1; the other 16 are bit-identical to the run without the NaN."""
    import qrw_hip

    T, origin, q0, command = _tick_case(stn)

    def poisoned(k):
        c = list(command(k))
        if k == 2:
            c[4] = c[4].copy()
            c[4][5, 7] = np.nan
        return tuple(c)

    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    set_terrain(eng, T, origin=origin)
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
        if k >= 2:
            for i, (x, y) in enumerate(zip(bad[k], bad[1])):
                if i != 4:
                    assert np.array_equal(x[5], y[5]) and np.all(np.isfinite(x[5])), (k, i)


# ------------------------------------------------------------------------------------------------ errors
def test_terrain_errors_leave_the_handle_usable(oracle_mod, stn):
    """rows or cols < 2, a spacing that is zero, negative, infinite or NaN, NULL heights, origins of the wrong shape, more
    forward-dynamics states than origins: refused with -1 (or by the binding) and a text that names the entry point; the terrain
    set before stays in force and the next valid call works."""
    import ctypes as C

    import qrw_hip

    B = 3
    T, states = _fd_states(stn, "rough")
    states = states[1:1 + B]
    eng = qrw_hip.Batch(B)
    set_terrain(eng, T, origin=np.stack([s[4] for s in states]))
    before = eng.test_sim_forward_dynamics(*[np.stack([s[i] for s in states]) for i in range(3)])
    H = _t(T.H)
    lib, h = eng._lib, eng._handle

    def dev(rows, cols, dx, dy, heights=H.data_ptr()):
        return lib.qrw_sim_set_terrain(h, heights, rows, cols, 0.0, 0.0, dx, dy, None, eng._stream()), lib.qrw_last_error().decode()

    def host(rows, cols, dx, dy, heights=T.H.ctypes.data_as(C.POINTER(C.c_double))):
        return lib.qrw_sim_set_terrain_host(h, heights, rows, cols, 0.0, 0.0, dx, dy, None), lib.qrw_last_error().decode()

    for call, name in ((dev, "qrw_sim_set_terrain: "), (host, "qrw_sim_set_terrain_host: ")):
        for args, text in (((1, 10, 0.05, 0.05), "rows and cols must be >= 2"), ((10, 1, 0.05, 0.05), "rows and cols must be >= 2"),
                           ((10, 10, 0.0, 0.05), "dx and dy must be positive and finite"), ((10, 10, 0.05, -0.05), "dx and dy must be positive and finite"),
                           ((10, 10, np.inf, 0.05), "dx and dy must be positive and finite"), ((10, 10, 0.05, np.nan), "dx and dy must be positive and finite"),
                           ((10, 10, 0.05, 0.05, None), "null heights")):
            rc, err = call(*args)
            assert rc == -1 and err == name + text, (args, rc, err)
    with pytest.raises(qrw_hip.QrwError, match="bad shape"):
        eng.sim_set_terrain(H, T.dx, T.dy, origin=_t(np.zeros((B + 1, 2))))
    with pytest.raises(qrw_hip.QrwError, match="heights must be"):
        eng.sim_set_terrain(np.zeros(10), T.dx, T.dy)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_test_sim_forward_dynamics: more states than the terrain's per-robot origins"):
        eng.test_sim_forward_dynamics(np.zeros((B + 1, 19)), np.zeros((B + 1, 18)), np.zeros((B + 1, 12)))
    after = eng.test_sim_forward_dynamics(*[np.stack([s[i] for s in states]) for i in range(3)])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])  # (none of the refused calls counted)
    out = eng.sim_outputs()
    eng.sim_init(_t(np.tile(Q_INIT, (B, 1))), out)
    cmd = [_t(np.full((B, 12), x)) for x in (3.0, 0.2, 0.0, 0.0, 0.0)]
    cmd[2] = _t(np.tile(Q_INIT, (B, 1)))
    eng.sim_step(*cmd, out)
    st = eng.sim_state()
    assert np.array_equal(st["tick"], np.ones(B)) and not st["status"].any() and np.all(np.isfinite(st["q"]))
    ref = stn.SimTerrainNumpy(Q_INIT, T, states[1][4])
    ref.step(3.0, 0.2, Q_INIT, np.zeros(12), np.zeros(12))
    assert _rel(st["q"][1], ref.q) <= TICK_BOUND and _rel(st["v"][1], ref.v) <= TICK_BOUND
    assert min(ref.min_abs_d, ref.min_diag, ref.min_edge) > MIN_SWITCH
