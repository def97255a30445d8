"""Independent numpy restatement of the reference's state estimator with its Kalman filter (scripts/Estimator.py, kf_enabled=True:
KFilterBis :88-181 and the Kalman branch of run_filter :555-580), one object per robot, built on estimator_numpy.Estimator for
everything the two filters share.  Test infrastructure: the product never imports it.

The filter is kept in the reference's DENSE form -- 18 states, 16 measurements, the full 18 x 18 P, np.linalg.inv of the 16 x 16
innovation covariance -- not in the per-axis, one-measurement-at-a-time arrangement of csrc/kalman_filter.h (that arrangement,
restated in numpy for the tolerance measurement, is AxisFilter below: the tests never use it as their reference)."""
import numpy as np

import estimator_numpy as en
import oracle

KALMAN_DEFAULTS = dict(sigma_kin=0.1, sigma_h=1.0, sigma_a=0.1, sigma_dp=0.1, gamma=30.0)  # :133-137
N_STATE, N_MEAS = 18, 16  # :92-93


class KFilterBis:
    """scripts/Estimator.py:88-181"""

    def __init__(self, dt, solve=False, **tuning):
        self.dt, self.solve = dt, solve
        self.A = np.eye(N_STATE)
        self.A[0:3, 3:6] = dt * np.eye(3)                                                  # :96-97
        self.B = np.zeros((N_STATE, 3))
        self.H = np.zeros((N_MEAS, N_STATE))
        for j in range(3):
            self.B[j, j], self.B[3 + j, j] = 0.5 * dt**2, dt                                 # :100-103
        for i in range(4):
            for j in range(3):
                self.H[3 * i + j, j], self.H[3 * i + j, 6 + 3 * i + j] = 1.0, -1.0           # :109-110
            self.H[12 + i, 6 + 3 * i + 2] = 1.0                                              # :111
        self.Q, self.R = np.zeros((N_STATE, N_STATE)), np.zeros((N_MEAS, N_MEAS))
        self.P, self.X = np.eye(N_STATE), np.zeros(N_STATE)                                 # :121, :127
        unknown = set(tuning) - set(KALMAN_DEFAULTS)
        assert not unknown, unknown
        self.tuning = dict(KALMAN_DEFAULTS, **tuning)

    def update_coeffs(self, status):
        """:167-181"""
        t = self.tuning
        for i in range(4):
            trust = 0.01 if status[i] == 0 else 1.0
            self.R[3 * i:3 * i + 3, 3 * i:3 * i + 3] = t["sigma_kin"]**2 / trust * np.eye(3)
            self.R[12 + i, 12 + i] = t["sigma_h"]**2 / trust
            self.Q[6 + 3 * i:9 + 3 * i, 6 + 3 * i:9 + 3 * i] = (t["sigma_dp"]**2 * (1 + np.exp(t["gamma"] * (0.5 - trust)))
                                                                * np.eye(3) * self.dt**2)
        self.Q[3:6, 3:6] = t["sigma_a"]**2 * np.eye(3) * self.dt**2

    def predict(self, U):
        """:152-157"""
        self.X = self.A @ self.X + self.B @ U
        self.P = self.A @ self.P @ self.A.T + self.Q

    def correct(self, Z):
        """:159-165 (solve=True: the same gain from a linear solve instead of the inverse, for the tolerance measurement)"""
        S = self.H @ self.P @ self.H.T + self.R
        PHt = self.P @ self.H.T
        K = np.linalg.solve(S.T, PHt.T).T if self.solve else PHt @ np.linalg.inv(S)
        self.X = self.X + K @ (Z - self.H @ self.X)
        self.P = self.P - K @ self.H @ self.P


class AxisFilter:
    """The arrangement of csrc/kalman_filter.h in numpy, with KFilterBis's interface: three 6-state filters (axis j: states
    j, 3+j, 6+j, 9+j, 12+j, 15+j), the rows of Z taken one at a time.  Only scripts/kalman_tolerance.py and the test of the
    structure use it."""

    def __init__(self, dt, **tuning):
        self.dt = dt
        self.dense = KFilterBis(dt, **tuning)  # for update_coeffs and the index structure alone
        self.idx = [np.array([j, 3 + j, 6 + j, 9 + j, 12 + j, 15 + j]) for j in range(3)]
        self.x = [np.zeros(6) for _ in range(3)]
        self.p = [np.eye(6) for _ in range(3)]

    @property
    def X(self):
        X = np.zeros(N_STATE)
        for j in range(3):
            X[self.idx[j]] = self.x[j]
        return X

    @X.setter
    def X(self, X):
        self.x = [np.array(X[self.idx[j]], dtype=np.float64) for j in range(3)]

    @property
    def P(self):
        P = np.zeros((N_STATE, N_STATE))
        for j in range(3):
            P[np.ix_(self.idx[j], self.idx[j])] = self.p[j]
        return P

    def update_coeffs(self, status):
        self.dense.update_coeffs(status)

    def predict(self, U):
        dt, Q = self.dt, self.dense.Q
        for j in range(3):
            x, p = self.x[j], self.p[j]
            x[0] = (x[0] + dt * x[1]) + (0.5 * (dt * dt)) * U[j]
            x[1] = x[1] + dt * U[j]
            p[0, :] += dt * p[1, :]
            p[:, 0] += dt * p[:, 1]
            p[np.arange(6), np.arange(6)] += Q[self.idx[j], self.idx[j]]

    def correct(self, Z):
        R = self.dense.R
        for j in range(3):
            x, p = self.x[j], self.p[j]
            rows = [(3 * i + j, i, False) for i in range(4)] + ([(12 + i, i, True) for i in range(4)] if j == 2 else [])
            for row, foot, height in rows:
                f = 2 + foot
                pht = p[:, f].copy() if height else p[:, 0] - p[:, f]
                hp = p[f, :].copy() if height else p[0, :] - p[f, :]
                s = (pht[f] if height else pht[0] - pht[f]) + R[row, row]
                innov = Z[row] - (x[f] if height else x[0] - x[f])
                gain = pht / s
                x += gain * innov
                p -= np.outer(gain, hp)


class Estimator(en.Estimator):
    """scripts/Estimator.py:234-629 with kf_enabled=True, without the logging.  Everything of run_filter outside :519-580 is the
    base class's; its complementary filters are left as __init__ leaves them in this mode (:282-285: the height goes into X[2],
    not into filter_xyz_pos) and are not stepped."""

    def __init__(self, dt, h_init=0.22294615, perfect=False, kalman=True, filter_class=KFilterBis, **filter_args):
        super().__init__(dt, h_init, perfect)
        tuning = {} if kalman is True else dict(kalman)
        self.filter_xyz_pos.LP_x[2] = 0.0                                                  # :282-283 not taken
        self.kf = filter_class(dt, **filter_args, **tuning)                                 # :269
        X = np.zeros(N_STATE)
        X[2] = h_init                                                                       # :285
        self.kf.X = X
        self.Z = np.zeros(N_MEAS)                                                           # :270

    @property
    def X(self):
        return self.kf.X

    @property
    def P(self):
        return self.kf.P

    def run_filter(self, gait, goals, lin_acc, ang_vel, quat, q_mes, v_mes, true_pos=None, true_b_vel=None):
        lin_acc, ang_vel = np.asarray(lin_acc, dtype=np.float64), np.asarray(ang_vel, dtype=np.float64)
        # the shared part (:476-517, :593-627) through the base class.  Its complementary branch (:519-553) runs too and is
        # undone: the two filters' states and what it put into filt_lin_vel, q_filt[0:3] and v_filt[0:3]
        keep = [f.copy() for f in (self.filter_xyz_vel.HP_x, self.filter_xyz_vel.LP_x, self.filter_xyz_pos.HP_x,
                                   self.filter_xyz_pos.LP_x)]
        v_prev = self.v_filt[0:3].copy()
        super().run_filter(gait, goals, lin_acc, ang_vel, quat, q_mes, v_mes, true_pos=true_pos, true_b_vel=true_b_vel)
        (self.filter_xyz_vel.HP_x, self.filter_xyz_vel.LP_x, self.filter_xyz_pos.HP_x, self.filter_xyz_pos.LP_x) = keep
        # the Kalman branch (:555-580)
        feet_status = np.asarray(gait, dtype=np.float64)[0, :]
        oRb = en.rotation_of(self.q_filt[3:7])                                              # :558 (q_filt[3:7] is IMU_ang_pos)
        self.kf.update_coeffs(feet_status)                                                  # :561
        self.kf.predict(oRb @ lin_acc)                                                      # :564
        posf = oracle.fixed_feet(np.asarray(q_mes, dtype=np.float64), np.asarray(v_mes, dtype=np.float64))[0]
        Z = np.zeros(N_MEAS)
        for i in range(4):
            Z[3 * i:3 * i + 3] = oRb @ (-posf[i] + self.lever)                              # :568-569
            Z[12 + i] = 0.0                                                                 # :570
        self.Z = Z
        self.kf.correct(Z)                                                                  # :575
        cross_product = np.cross(self.lever, ang_vel)                                       # :578
        filt_lin_pos = self.kf.X[0:3] - self.lever                                          # :579 (the offset is not rotated)
        self.filt_lin_vel = oRb.T @ (self.kf.X[3:6] - cross_product)                        # :580
        # outputs (:594-604) again with the Kalman results
        self.q_filt[0:3] = filt_lin_pos
        if self.perfect:
            self.q_filt[2] = true_pos[2] - 0.0155
        new = np.asarray(true_b_vel, dtype=np.float64) if self.perfect else self.filt_lin_vel
        self.v_filt[0:3] = (1 - self.alpha_v) * v_prev + self.alpha_v * new
        return 0
