"""A second implementation of the planners, in plain numpy, written from the reference's C++ (src/Gait.cpp, src/FootstepPlanner.cpp,
src/FootTrajectoryGenerator.cpp, src/StatePlanner.cpp, called in the order of scripts/Controller.py:222-236) and NOT from
oracle/planner_oracle.c or the kernel: it pins the oracle the GPU tests compare with (tests/test_planner_second_impl.py).

It is different where that buys independence:
  * the gait matrices are dense (N_gait + 1) x 4 arrays moved with np.roll, the phase durations are found with argmin on boolean
    columns instead of row-by-row walks;
  * the swing's height is the factored form  z(e) = h 64 (e (d - e))^3 / d^6  and its derivatives (the reference expands it into
    four monomials, FootTrajectoryGenerator.cpp:76-80,103-105);
  * the swing's x / y quintic is found by SOLVING its six boundary conditions -- position, velocity, acceleration now; the target
    with zero velocity and acceleration at the end of the swing -- in np.longdouble, in the time since `now`, where the reference
    evaluates a closed form in powers of absolute time (:57-69).  closed_form() restates that closed form only to show, once,
    that the two agree to rounding (test_solved_quintic_is_the_closed_form).

The size rule and the zero row beyond the table are those of csrc/gait_masks.h: every generator must fit N_gait rows, and a
period that fills the table makes row N_gait count as zero (the reference reads past its matrices there).  Where the reference
would walk off the end of its footstep list looking for a target (a foot that never stands in the table), the search stops at
the last row, as the kernel and the oracle do."""
import math

import numpy as np

LD = np.longdouble


def lround(x):
    f = math.floor(abs(x))
    n = f + (1 if abs(x) - f >= 0.5 else 0)
    return n if x >= 0 else -n


def rows_needed(T_gait, dt):
    return max(2 * lround(0.5 * T_gait / dt), 4 * lround(0.25 * T_gait / dt), lround(T_gait / dt))


def table_fits(N_gait, n_steps, T_gait, dt):
    return 1 <= N_gait <= 63 and n_steps >= 1 and n_steps + 1 <= N_gait and rows_needed(T_gait, dt) <= N_gait


# ------------------------------------------------------------------------------------------------ the swing polynomials
def solve_quintic(D, x0, v0, a0, target):
    """c[0..5] of p(s) = sum c[n] s^n, s the time since now, with p(0) = x0, p'(0) = v0, p''(0) = a0 and p(D) = target,
    p'(D) = p''(D) = 0, in longdouble.  The first three conditions give c[0..2]; the other three are a 3 x 3 system in
    (c3 D^3, c4 D^4, c5 D^5), solved by elimination with the rows as they stand (the matrix is fixed and well conditioned)."""
    D, x0, v0, a0, target = LD(D), LD(x0), LD(v0), LD(a0), LD(target)
    c0, c1, c2 = x0, v0, a0 / 2
    # unknowns u = c3 D^3, v = c4 D^4, w = c5 D^5:
    #   u +   v +   w = target - c0 - c1 D - c2 D^2            (position)
    #  3u +  4v +  5w = -(c1 D + 2 c2 D^2)                      (velocity * D)
    #  6u + 12v + 20w = -(2 c2 D^2)                             (acceleration * D^2)
    M = np.array([[1, 1, 1], [3, 4, 5], [6, 12, 20]], dtype=LD)
    r = np.array([target - c0 - c1 * D - c2 * D * D, -(c1 * D + 2 * c2 * D * D), -(2 * c2 * D * D)], dtype=LD)
    for i in range(3):
        for k in range(i + 1, 3):
            f = M[k, i] / M[i, i]
            M[k] -= f * M[i]
            r[k] -= f * r[i]
    sol = np.zeros(3, dtype=LD)
    for i in (2, 1, 0):
        sol[i] = (r[i] - (M[i, i + 1:] * sol[i + 1:]).sum()) / M[i, i]
    return np.array([c0, c1, c2, sol[0] / D ** 3, sol[1] / D ** 4, sol[2] / D ** 5], dtype=LD)


def monomials(c, t):
    """The coefficients A[0..5] of the same polynomial in powers of ABSOLUTE time e = t + s, highest power first (the reference's
    Ax(0..5)): p = sum c[n] (e - t)^n expanded with the binomial theorem, in longdouble."""
    A = np.zeros(6, dtype=LD)
    t = LD(t)
    for n in range(6):
        for m in range(n + 1):
            A[5 - m] += c[n] * math.comb(n, m) * (-t) ** (n - m)
    return A


def closed_form(t, d, x0, dx0, ddx0, tg):
    """The reference's closed-form coefficients Ax(0..5) (FootTrajectoryGenerator.cpp:57-62) in double, as it evaluates them."""
    P = pow
    den1 = 2 * P(t - d, 2) * (P(t, 3) - 3 * P(t, 2) * d + 3 * t * P(d, 2) - P(d, 3))
    den2 = 2 * (P(t, 2) - 2 * t * d + P(d, 2)) * (P(t, 3) - 3 * P(t, 2) * d + 3 * t * P(d, 2) - P(d, 3))
    A0 = (ddx0 * P(t, 2) - 2 * ddx0 * t * d - 6 * dx0 * t + ddx0 * P(d, 2) + 6 * dx0 * d + 12 * x0 - 12 * tg) / den1
    A1 = (30 * t * tg - 30 * t * x0 - 30 * d * x0 + 30 * d * tg - 2 * P(t, 3) * ddx0 - 3 * P(d, 3) * ddx0 + 14 * P(t, 2) * dx0
          - 16 * P(d, 2) * dx0 + 2 * t * d * dx0 + 4 * t * P(d, 2) * ddx0 + P(t, 2) * d * ddx0) / den1
    A2 = (P(t, 4) * ddx0 + 3 * P(d, 4) * ddx0 - 8 * P(t, 3) * dx0 + 12 * P(d, 3) * dx0 + 20 * P(t, 2) * x0 - 20 * P(t, 2) * tg
          + 20 * P(d, 2) * x0 - 20 * P(d, 2) * tg + 80 * t * d * x0 - 80 * t * d * tg + 4 * P(t, 3) * d * ddx0
          + 28 * t * P(d, 2) * dx0 - 32 * P(t, 2) * d * dx0 - 8 * P(t, 2) * P(d, 2) * ddx0) / den1
    A3 = -(P(d, 5) * ddx0 + 4 * t * P(d, 4) * ddx0 + 3 * P(t, 4) * d * ddx0 + 36 * t * P(d, 3) * dx0 - 24 * P(t, 3) * d * dx0
           + 60 * t * P(d, 2) * x0 + 60 * P(t, 2) * d * x0 - 60 * t * P(d, 2) * tg - 60 * P(t, 2) * d * tg
           - 8 * P(t, 2) * P(d, 3) * ddx0 - 12 * P(t, 2) * P(d, 2) * dx0) / den2
    A4 = -(2 * P(d, 5) * dx0 - 2 * t * P(d, 5) * ddx0 - 10 * t * P(d, 4) * dx0 + P(t, 2) * P(d, 4) * ddx0
           + 4 * P(t, 3) * P(d, 3) * ddx0 - 3 * P(t, 4) * P(d, 2) * ddx0 - 16 * P(t, 2) * P(d, 3) * dx0
           + 24 * P(t, 3) * P(d, 2) * dx0 - 60 * P(t, 2) * P(d, 2) * x0 + 60 * P(t, 2) * P(d, 2) * tg) / den1
    A5 = (2 * tg * P(t, 5) - ddx0 * P(t, 4) * P(d, 3) - 10 * tg * P(t, 4) * d + 2 * ddx0 * P(t, 3) * P(d, 4)
          + 8 * dx0 * P(t, 3) * P(d, 3) + 20 * tg * P(t, 3) * P(d, 2) - ddx0 * P(t, 2) * P(d, 5) - 10 * dx0 * P(t, 2) * P(d, 4)
          - 20 * x0 * P(t, 2) * P(d, 3) + 2 * dx0 * t * P(d, 5) + 10 * x0 * t * P(d, 4) - 2 * x0 * P(d, 5)) / den2
    return np.array([A0, A1, A2, A3, A4, A5])


def quat_to_rpy(q):
    """pinocchio::rpy::matrixToRpy of Eigen's Quaterniond(w, x, y, z).toRotationMatrix(), q = (x, y, z, w)."""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    p = math.atan2(-R[2, 0], math.hypot(R[2, 1], R[2, 2]))
    if abs(abs(p) - math.pi / 2) < 0.001:
        return np.array([0.0, p, -math.atan2(R[0, 1], R[1, 1])])
    return np.array([math.atan2(R[2, 1], R[2, 2]), p, math.atan2(R[1, 0], R[0, 0])])


SEQUENCES = {1: ((1, 0, 1, 0), (0, 1, 0, 1)), 2: ((1, 1, 0, 0), (0, 0, 1, 1)), 3: ((1, 0, 0, 1), (0, 1, 1, 0)), 4: ((1, 1, 1, 1),),
             5: ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0))}


class Planner:
    """Gait + StatePlanner + FootstepPlanner + FootTrajectoryGenerator of one robot; the getters are those of oracle.Planner."""

    def __init__(self, dt_mpc=0.02, dt_wbc=0.002, T_gait=0.32, T_mpc=0.32, N_gait=20, k_mpc=10, h_ref=0.2229, shoulders=None,
                 max_height=0.05, lock_time=0.07, init_target=None, init_foot_pos=None):
        self.dt, self.dt_wbc, self.T_gait, self.T_mpc, self.N_gait, self.k_mpc = dt_mpc, dt_wbc, T_gait, T_mpc, int(N_gait), int(k_mpc)
        self.n_steps = lround(T_mpc / dt_mpc)
        if not table_fits(self.N_gait, self.n_steps, T_gait, dt_mpc):
            raise ValueError("Sizes of matrices are too small for considered durations. Increase N_gait in config file.")
        if shoulders is None:
            shoulders = [[0.1946, 0.1946, -0.1946, -0.1946], [0.14695, -0.14695, 0.14695, -0.14695], [0.0, 0.0, 0.0, 0.0]]
        sh = np.array(shoulders, dtype=np.float64).reshape(3, 4)
        Ng = self.N_gait
        # Gait::initialize (Gait.cpp:19-36)
        self.past, self.cur = np.zeros((Ng + 1, 4)), np.zeros((Ng + 1, 4))
        self.des = self._generate(3)
        self.remaining_time, self.new_phase, self.is_static, self.q_static = 0.0, False, False, np.zeros(19)
        live = self._first_zero_row(self.des)
        for j in range(self.n_steps):  # create_gait_f (:110-139): the period repeated down the horizon ...
            self.cur[j] = self.des[j % live]
        self.des[:live] = np.roll(self.des[:live], -(self.n_steps % live), axis=0)  # ... and the desired gait aged as far
        # StatePlanner::initialize (StatePlanner.cpp:12-19)
        self.h_ref = h_ref
        self.dt_vector = np.array([T_mpc]) if self.n_steps == 1 else np.linspace(dt_mpc, T_mpc, self.n_steps)
        self.X = np.zeros((12, self.n_steps + 1))
        # FootstepPlanner::initialize (FootstepPlanner.cpp:22-49)
        self.k_feedback, self.g, self.L = 0.03, 9.81, 0.155
        self.shoulders, self.current, self.target, self.o_target = sh.copy(), sh.copy(), sh.copy(), sh.copy()
        self.fs = np.zeros((Ng, 3, 4))
        # FootTrajectoryGenerator::initialize (FootTrajectoryGenerator.cpp:23-38)
        self.max_height, self.lock_time = max_height, lock_time
        self.ft_tgt = np.array(sh if init_target is None else init_target, dtype=np.float64).reshape(3, 4).copy()
        self.pos = np.array(sh if init_foot_pos is None else init_foot_pos, dtype=np.float64).reshape(3, 4).copy()
        self.vel, self.acc = np.zeros((3, 4)), np.zeros((3, 4))
        self.feet, self.t0s, self.t_swing = [], np.zeros(4), np.zeros(4)
        self.poly = [[(0.0, np.zeros(6, dtype=LD)) for _ in range(2)] for _ in range(4)]  # per foot, x / y: (fitted at, c[0..5])

    # ---------------------------------------------------------------- Gait
    def _generate(self, code):
        seq = SEQUENCES[code]
        n = lround((1.0 / len(seq)) * self.T_gait / self.dt)  # rows per phase: 0.5, 0.25 or 1.0 times the period (Gait.cpp:41,59,101)
        m = np.zeros((self.N_gait + 1, 4))
        for p, row in enumerate(seq):
            m[p * n:(p + 1) * n] = row
        return m

    @staticmethod
    def _first_zero_row(m):  # of rows 1, 2, ...: the loops of Gait.cpp:126-130,242-247,253-258 start at row 1
        return 1 + int(np.argmin(m[1:].any(axis=1)))

    def phase_duration(self, i, j, value):
        """Gait::getPhaseDuration (Gait.cpp:142-185)."""
        same = self.cur.any(axis=1) & (self.cur[:, j] == value)
        run = int(np.argmin(same[i + 1:]))  # (row N_gait is zero: the search always ends)
        t = 1 + run
        if not self.cur[i + run + 1].any():
            t += int(np.argmin(self.des.any(axis=1) & (self.des[:, j] == value)))
        self.remaining_time = float(t)
        back = (self.cur[:i, j] == value)[::-1]
        runb = i if back.all() else int(np.argmin(back))
        t += runb
        if runb == i:
            t += int(np.argmin(self.past.any(axis=1) & (self.past[:, j] == value)))
        return t * self.dt

    def gait_update(self, k, q7, code):
        """Gait::updateGait = changeGait + rollGait (Gait.cpp:187-260); code 5 selects create_walk (:38-54)."""
        self.is_static = False
        if code in SEQUENCES:
            self.des = self._generate(code)
            if code == 4:
                self.q_static[:7] = q7
                self.is_static = True
        if k % self.k_mpc != 0:
            return
        n = self.n_steps + 1
        self.past[:n] = np.roll(self.past[:n], 1, axis=0)
        self.past[0] = self.cur[0]
        self.new_phase = not np.array_equal(self.cur[0], self.cur[1])
        live = self._first_zero_row(self.cur)
        self.cur[:live] = np.roll(self.cur[:live], -1, axis=0)
        self.cur[live - 1] = self.des[0]
        live = self._first_zero_row(self.des)
        self.des[:live] = np.roll(self.des[:live], -1, axis=0)

    # ---------------------------------------------------------------- StatePlanner
    def state_compute(self, q7, v, vref, z_average=0.0):
        """StatePlanner::computeReferenceStates (StatePlanner.cpp:21-61)."""
        rpy = quat_to_rpy(q7[3:7])
        X, t, w = self.X, self.dt_vector, vref[5]
        X[:, 0] = [0.0, 0.0, q7[2], rpy[0], rpy[1], 0.0, *v]
        yaw = w * t
        if w != 0:
            X[0, 1:] = (vref[0] * np.sin(yaw) + vref[1] * (np.cos(yaw) - 1.0)) / w
            X[1, 1:] = (vref[1] * np.sin(yaw) - vref[0] * (np.cos(yaw) - 1.0)) / w
        else:
            X[0, 1:], X[1, 1:] = vref[0] * t, vref[1] * t
        X[2, 1:], X[5, 1:], X[11, 1:] = self.h_ref + z_average, yaw, w
        X[6, 1:] = vref[0] * np.cos(yaw) - vref[1] * np.sin(yaw)
        X[7, 1:] = vref[0] * np.sin(yaw) + vref[1] * np.cos(yaw)

    # ---------------------------------------------------------------- FootstepPlanner
    def footsteps_update(self, refresh, k, q7, b_v, b_vref):
        """FootstepPlanner::updateFootsteps (FootstepPlanner.cpp:51-75) and what it calls (:77-232)."""
        stance = self.cur[0] == 1.0
        if refresh and self.new_phase:  # updateNewContact (:223-232)
            self.current[:, stance] = self.fs[1][:, stance]
        a = self.dt_wbc * b_vref[5]
        c, s = math.cos(a), math.sin(a)
        moved = np.array([[c, s], [-s, c]]) @ (self.current[:2] - (self.dt_wbc * b_vref[:2])[:, None])
        self.current[:2, stance] = moved[:, stance]
        # computeFootsteps (:77-156)
        Ng, gait, w = self.N_gait, self.cur, b_vref[5]
        fs = np.zeros((Ng, 3, 4))
        fs[0][:, stance] = self.current[:, stance]
        steps = np.zeros(Ng)
        steps[0], steps[1:] = self.dt_wbc * k, np.where(gait[1:Ng].any(axis=1), self.dt, 0.0)
        dt_cum = np.cumsum(steps)
        yaws = w * dt_cum
        if w != 0:
            dx = (b_v[0] * np.sin(yaws) + b_v[1] * (np.cos(yaws) - 1.0)) / w
            dy = (b_v[1] * np.sin(yaws) - b_v[0] * (np.cos(yaws) - 1.0)) / w
        else:
            dx, dy = b_v[0] * dt_cum, b_v[1] * dt_cum
        cross = np.array([b_v[1] * b_vref[5] - b_v[2] * b_vref[4], b_v[2] * b_vref[3] - b_v[0] * b_vref[5], 0.0])
        i = 1
        while gait[i].any():
            keep = gait[i - 1] * gait[i] > 0
            fs[i][:, keep] = fs[i - 1][:, keep]
            for j in np.nonzero((1 - gait[i - 1]) * gait[i] > 0)[0]:
                nxt = self.phase_duration(i, j, 1.0) * 0.5 * b_v[:3]                 # computeNextFootstep (:158-186)
                nxt = nxt + self.k_feedback * (b_v[:3] - b_vref[:3])
                nxt = nxt + 0.5 * math.sqrt(self.h_ref / self.g) * cross
                nxt[:2] = np.clip(nxt[:2], -self.L, self.L)
                nxt = nxt + self.shoulders[:, j]
                nxt[2] = 0.0
                c, s = math.cos(yaws[i - 1]), math.sin(yaws[i - 1])
                fs[i][:, j] = [c * nxt[0] - s * nxt[1] + dx[i - 1], s * nxt[0] + c * nxt[1] + dy[i - 1], nxt[2]]
            i += 1
        self.fs = fs
        for f in range(4):  # updateTargetFootsteps (:188-199)
            hit = np.nonzero(fs[:, 0, f] != 0.0)[0]
            row = int(hit[0]) if len(hit) else Ng - 1
            self.target[:, f] = [fs[row, 0, f], fs[row, 1, f], 0.0]
        yaw = quat_to_rpy(q7[3:7])[2]  # computeTargetFootstep (:201-221)
        c, s = math.cos(yaw), math.sin(yaw)
        self.Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        self.o_target[:2] = np.array([[c, -s], [s, c]]) @ self.target[:2] + np.asarray(q7[:2])[:, None]
        return self.o_target.copy()

    # ---------------------------------------------------------------- FootTrajectoryGenerator
    def _update_foot(self, j, tf):
        """FootTrajectoryGenerator::updateFootPosition (FootTrajectoryGenerator.cpp:41-106)."""
        t, d, dt, h = self.t0s[j], self.t_swing[j], self.dt_wbc, self.max_height
        if t < d - self.lock_time:
            for ax in range(2):
                self.poly[j][ax] = (t, solve_quintic(d - t, self.pos[ax, j], self.vel[ax, j], self.acc[ax, j], tf[ax]))
            self.ft_tgt[:2, j] = tf[:2]
        ev = t + dt
        if t < 0.0 or t > d:
            self.vel[:2, j], self.acc[:2, j] = 0.0, 0.0
        else:
            for ax in range(2):
                at, c = self.poly[j][ax]
                s = LD(ev) - LD(at)
                self.pos[ax, j] = float(sum(c[n] * s ** n for n in range(6)))
                self.vel[ax, j] = float(sum(n * c[n] * s ** (n - 1) for n in range(1, 6)))
                self.acc[ax, j] = float(sum(n * (n - 1) * c[n] * s ** (n - 2) for n in range(2, 6)))
        u, du, scale = ev * (d - ev), d - 2 * ev, 64.0 * h / d ** 6
        self.pos[2, j] = scale * u ** 3
        self.vel[2, j] = scale * 3 * u ** 2 * du
        self.acc[2, j] = scale * (6 * u * du ** 2 - 6 * u ** 2)

    def traj_update(self, k, target):
        """FootTrajectoryGenerator::update (FootTrajectoryGenerator.cpp:108-151)."""
        if k % self.k_mpc == 0:
            self.feet = [i for i in range(4) if self.cur[0, i] == 0]
            for i in self.feet:
                self.t_swing[i] = self.phase_duration(0, i, 0.0)
                self.t0s[i] = max(0.0, self.t_swing[i] - (self.remaining_time * self.k_mpc - ((k + 1) % self.k_mpc)) * self.dt_wbc - self.dt_wbc)
        else:
            for i in self.feet:
                self.t0s[i] = max(0.0, self.t0s[i] + self.dt_wbc)
        for i in self.feet:
            self._update_foot(i, target[:, i])

    # ---------------------------------------------------------------- one control iteration (scripts/Controller.py:222-236)
    def step(self, k, q7, h_v, vref, code=0):
        q7, h_v, vref = (np.asarray(x, dtype=np.float64) for x in (q7, h_v, vref))
        self.gait_update(k, q7, code)
        target = self.footsteps_update(k % self.k_mpc == 0 and k != 0, self.k_mpc - k % self.k_mpc, q7, h_v, vref)
        self.traj_update(k, target)
        self.state_compute(q7, h_v, vref, 0.0)

    def gaits(self):
        Ng = self.N_gait
        assert not (self.past[Ng].any() or self.cur[Ng].any() or self.des[Ng].any())  # the row beyond the table stays zero
        return self.past[:Ng].copy(), self.cur[:Ng].copy(), self.des[:Ng].copy()

    def flags(self):
        return dict(new_phase=bool(self.new_phase), is_static=bool(self.is_static), remaining_time=self.remaining_time, n_swing=len(self.feet))

    def xref(self):
        return self.X.copy()

    def footsteps(self):
        return self.fs.transpose(0, 2, 1).reshape(self.N_gait, 12).copy(), self.target.copy(), self.o_target.copy()

    def feet_state(self):
        return self.pos.copy(), self.vel.copy(), self.acc.copy(), self.t0s.copy(), self.t_swing.copy()

    def ft_target(self):
        return self.ft_tgt.copy()
