"""numpy restatement of the rigid-body simulator's tick (csrc/sim_kernel.hip), one object per robot.  TEST CODE: the product never
imports it.  The rigid-body terms come from the CPU oracle (oracle.crba 18x18, oracle.rnea, oracle.feet_jacobians,
oracle.fixed_feet), so the device's per-leg Schur-complement form is checked against a dense 18x18 solve of independent code.

Line numbers are those of the reference's scripts/PyBulletSimulator.py.  The physics step is the project's own (penalty contact on
the plane z = 0, semi-implicit Euler), NOT PyBullet's.
"""
import numpy as np

import oracle

DEFAULTS = dict(dt=0.002, substeps=8, kn=1e4, dn=60.0, mu=0.9, vs=0.01, foot_radius=0.0155)
Q_STANCE = np.array([0.0, 0.7, -1.4, 0.0, 0.7, -1.4, 0.0, -0.7, 1.4, 0.0, -0.7, 1.4])  # scripts/main_solo12_control.py q_init
LEVER = np.array([0.1163, 0.0, 0.02])  # (:626)


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def contact_forces(q19, v18, prm):
    """World forces on the four feet (4,3) and the penetrations d (4,): normal kn d - dn vz clipped at 0 while d > 0,
    friction -mu fn v_t / sqrt(|v_t|^2 + vs^2)."""
    R = quat_to_rot(q19[3:7])
    pf_b = oracle.fixed_feet(q19[7:], v18[6:])[0]  # feet in the base frame
    J = oracle.feet_jacobians(q19)                 # world-aligned: J v = world velocity of the feet
    pw = q19[:3] + pf_b @ R.T                      # p + R pf_b
    vw = (J @ v18).reshape(4, 3)                   # R (v_lin + w x pf_b + J_leg dq_leg)
    f = np.zeros((4, 3))
    d = prm["foot_radius"] - pw[:, 2]
    for j in range(4):
        if d[j] > 0:
            fn = max(0.0, prm["kn"] * d[j] - prm["dn"] * vw[j, 2])
            vt = vw[j, :2]
            ft = -prm["mu"] * fn * vt / np.sqrt(vt @ vt + prm["vs"] ** 2)
            f[j] = [ft[0], ft[1], fn]
    return f, d, J


def rhs_of(q19, v18, tau12, f, J, f_ext=None):
    """[0; tau] + J'f + [R'f_ext; R'm_ext; 0] - h(q, v), h = rnea(q, v, 0) with gravity."""
    rhs = np.concatenate([np.zeros(6), tau12]) + J.T @ f.ravel() - oracle.rnea(q19, v18, np.zeros(18))
    if f_ext is not None:
        R = quat_to_rot(q19[3:7])
        rhs[:3] += R.T @ f_ext[:3]
        rhs[3:6] += R.T @ f_ext[3:]
    return rhs


def forward_dynamics(q19, v18, tau12, prm=DEFAULTS, f_ext=None, solve=np.linalg.solve):
    """a18 with M(q) a = rhs, the contact forces (4,3) and the penetrations (4,)."""
    f, d, J = contact_forces(q19, v18, prm)
    a = solve(oracle.crba(q19), rhs_of(q19, v18, tau12, f, J, f_ext))
    return a, f, d


def solve_longdouble(M, r):
    """Gaussian elimination with partial pivoting in numpy's longdouble (the yardstick of the float64 solve's own error)."""
    A = np.array(M, dtype=np.longdouble)
    b = np.array(r, dtype=np.longdouble)
    n = len(b)
    for p in range(n):
        i = p + int(np.argmax(np.abs(A[p:, p])))
        if i != p:
            A[[p, i]] = A[[i, p]]
            b[[p, i]] = b[[i, p]]
        for k in range(p + 1, n):
            l = A[k, p] / A[p, p]
            A[k, p:] -= l * A[p, p:]
            b[k] -= l * b[p]
    x = np.zeros(n, dtype=np.longdouble)
    for p in range(n - 1, -1, -1):
        x[p] = (b[p] - A[p, p + 1:] @ x[p + 1:]) / A[p, p]
    return x


def substep(q19, v18, tau12, h, prm, f_ext=None):
    """One semi-implicit Euler step: v += h a; p += h R v_lin; quat = normalise(quat (x) exp(h w)); q_j += h dq_j, every update with
    the velocities just updated, R of the start of the step."""
    a, f, d = forward_dynamics(q19, v18, tau12, prm, f_ext)
    R = quat_to_rot(q19[3:7])
    v2 = v18 + h * a
    q2 = q19.copy()
    q2[:3] += h * (R @ v2[:3])
    r = h * v2[3:6]
    th = np.sqrt(r @ r)
    k = 0.5 if th < 1e-8 else np.sin(0.5 * th) / th
    qn = quat_mul(q19[3:7], np.array([k * r[0], k * r[1], k * r[2], np.cos(0.5 * th)]))
    q2[3:7] = qn / np.sqrt(qn @ qn)
    q2[7:] += h * v2[6:]
    return q2, v2, f, d


def measurements(q19, v18, prev_o_imuVel, dt):
    """UpdateMeasurment (:593-631) from the simulator's state (base velocities are already in the base frame)."""
    R = quat_to_rot(q19[3:7])
    w = v18[3:6].copy()                                # (:620) oMb.rotation' (world angular velocity)
    o_imuVel = R @ v18[:3] + R @ np.cross(LEVER, w)    # (:623, :626)
    lin_acc = R.T @ (o_imuVel - prev_o_imuVel) / dt    # (:628)
    return dict(q_mes=q19[7:].copy(), v_mes=v18[6:].copy(), quat=q19[3:7].copy(), ang_vel=w, o_imu_vel=o_imuVel, lin_acc=lin_acc,
                true_pos=q19[:3].copy(), true_b_vel=v18[:3].copy())  # dummyPos (:604), b_baseVel (:624)


def world_momentum(q19, v18):
    """Linear momentum and angular momentum about the world origin, both in the world frame (6,).  The top six rows of M(q) v are
    the robot's momentum in the base frame, the angular part about the base origin: rotated by R and moved by p x."""
    hb = (oracle.crba(q19) @ v18)[:6]
    R = quat_to_rot(q19[3:7])
    lin = R @ hb[:3]
    return np.concatenate([lin, R @ hb[3:] + np.cross(q19[:3], lin)])


def tumbling_state(rng, height=1.0):
    """An airborne state far from the ground: random attitude and joints, base twist and joint speeds of a few rad/s."""
    quat = rng.normal(size=4)
    q = np.concatenate([0.2 * rng.normal(size=2), [height], quat / np.linalg.norm(quat), Q_STANCE + 0.3 * rng.normal(size=12)])
    v = np.concatenate([rng.normal(size=3), 2.0 * rng.normal(size=3), 3.0 * rng.normal(size=12)])
    return q, v


class SimNumpy:
    """One robot.  state(): (q19, v18, prev_o_imuVel, tick, status)."""

    def __init__(self, q_init, **params):
        self.prm = dict(DEFAULTS, **params)
        q_init = np.asarray(q_init, dtype=float).ravel()
        if q_init.size == 12:
            q_init = np.concatenate([[0.0, 0.0, params.get("base_height", 0.2596)], [0.0, 0.0, 0.0, 1.0], q_init])
        self.prm.pop("base_height", None)
        self.q, self.v = q_init.copy(), np.zeros(18)
        self.prev = np.zeros(3)
        self.tick, self.status = 0, 0
        self.min_abs_d = np.inf  # smallest |foot_radius - z_foot| met over all sub-steps: how near a contact switch came
        self.out = measurements(self.q, self.v, self.prev, self.prm["dt"])
        self.prev = self.out["o_imu_vel"].copy()  # (:629)
        self.out.update(contact_forces=np.zeros((4, 3)), joint_torques=np.zeros(12))

    def set_state(self, q19, v18, prev, tick=0, status=0):
        self.q, self.v, self.prev = np.array(q19, dtype=float), np.array(v18, dtype=float), np.array(prev, dtype=float)
        self.tick, self.status = int(tick), int(status)

    def step(self, P, D, q_des, v_des, tau_ff, f_ext=None):
        """SendCommand (:672-710) with the project's physics step, then UpdateMeasurment (:588-633)."""
        if self.status:
            return self.out
        prm = self.prm
        tau = tau_ff + P * (q_des - self.q[7:]) + D * (v_des - self.v[6:])  # (:685-688), once per tick
        q, v, f = self.q, self.v, np.zeros((4, 3))
        h = prm["dt"] / prm["substeps"]
        with np.errstate(all="ignore"):
            for _ in range(prm["substeps"]):
                q, v, f, d = substep(q, v, tau, h, prm, f_ext)
                if np.all(np.isfinite(d)):
                    self.min_abs_d = min(self.min_abs_d, float(np.abs(d).min()))
            out = measurements(q, v, self.prev, prm["dt"])
        out.update(contact_forces=f, joint_torques=tau)
        if not all(np.all(np.isfinite(x)) for x in (q, v, tau, f, *out.values())):
            self.status = 1  # frozen: state and outputs keep their last finite values
            return self.out
        self.q, self.v, self.prev, self.out = q, v, out["o_imu_vel"].copy(), out
        self.tick += 1
        return out
