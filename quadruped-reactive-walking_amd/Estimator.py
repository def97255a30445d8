"""Drop-in for the reference's scripts/Estimator.py: `Estimator` with the complementary filters (kf_enabled=False, the
reference's default, scripts/Controller.py:110-111) for ONE robot, on a batch-1 handle of libqrw_hip.so
(qrw_estimator_step_host -> estimator_kernel.hip).  The fleet path is Controller_batch.compute_sensors, which has both of the
reference's filters (estimator=dict(kalman=True) for KFilterBis).

Provided: the constructor, run_filter(k, gait, device, goals), get_configurations(), EulerToQuaternion, quaternionToRPY, cross3
and the attributes the reference's callers read (q_filt, v_filt, v_secu, RPY, alpha, FK_lin_vel, FK_xyz, xyz_mean_feet,
filt_lin_vel, filt_lin_pos, close_from_contact, k_since_contact, feet_status, feet_goals, k_log, offset_yaw_IMU, the two
filters' HP_x / LP_x / alpha, and the copies of the device's readings).
Not provided HERE yet: the Kalman variant.  The library and the fleet path have it (qrw_estimator_init_kalman,
qrw_hip.Batch.estimator_init(kalman=True)), but this single-robot drop-in still raises NotImplementedError for kf_enabled=True
and has no `kf` / `Z` attributes: tests/test_estimator_cpu.py pins that refusal, and lifting it (a kalman=True on the batch-1
handle, X / P / Z through estimator_kalman_get) belongs to a change that may touch that test.  Never provided: KFilter (which
Estimator does not construct), the log_* arrays and plot_graphs.  One departure: a gait whose rows all equal row 0 gives remaining_steps = N_gait where the reference raises
IndexError (scripts/Estimator.py:476-479)."""
import numpy as np

import qrw_hip


class Estimator:
    """State estimator with a complementary filter (scripts/Estimator.py:234-342)."""

    def __init__(self, dt, N_simulation, h_init=0.22294615, kf_enabled=False, perfectEstimator=False):
        if kf_enabled:
            raise NotImplementedError("Estimator(kf_enabled=True): the Kalman variant (KFilterBis) is not provided; the reference's "
                                      "default is the complementary filter (scripts/Controller.py:110-111)")
        self.dt = float(dt)
        self.perfectEstimator = bool(perfectEstimator)
        self.kf_enabled = False
        self.FK_h = float(h_init)
        # (scripts/Estimator.py:254-262)
        y = 1 - np.cos(2 * np.pi * 50.0 * dt)
        self.alpha_v = -y + np.sqrt(y * y + 2 * y)
        y = 1 - np.cos(2 * np.pi * 6.0 * dt)
        self.alpha_secu = -y + np.sqrt(y * y + 2 * y)
        self.q_filt = np.zeros((19, 1))
        self.v_filt = np.zeros((18, 1))
        self.v_secu = np.zeros((12, ))
        self.RPY = np.zeros((3, 1))
        self.IMU_lin_acc = np.zeros((3, ))
        self.feet_status = np.zeros(4)
        self.feet_goals = np.zeros((3, 4))
        self._b = None
        self._calls = 0

    # ---- the batch-1 handle: made for the gait matrix of the first call (the reference's constructor does not know N_gait)
    def _ensure(self, rows=None):
        b = self._b
        if b is not None and (rows is None or rows == b.N_gait):
            return b
        if b is not None and self._calls > 0:
            raise ValueError("run_filter: gait matrix of %d rows, earlier calls had %d" % (rows, b.N_gait))
        if b is not None:
            b.close()
        rows = 20 if rows is None else int(rows)
        self._b = b = qrw_hip.Batch(1, n_steps=min(16, rows), N_gait=rows, dt_wbc=self.dt)
        b.estimator_init(self.FK_h, self.perfectEstimator)
        return b

    def get_configurations(self):
        return self.q_filt.reshape((19,)), self.v_filt.reshape((18,))

    def run_filter(self, k, gait, device, goals):
        """scripts/Estimator.py:466-629.  device: any object with baseLinearAcceleration, baseAngularVelocity, baseOrientation
        (xyzw), q_mes, v_mes -- and dummyPos, b_baseVel for a perfect estimator."""
        gait = np.asarray(gait, dtype=np.float64)
        goals = np.asarray(goals, dtype=np.float64)
        b = self._ensure(gait.shape[0])
        tp = tv = None
        if self.perfectEstimator:
            tp, tv = np.asarray(device.dummyPos, dtype=np.float64), np.asarray(device.b_baseVel, dtype=np.float64)
        o = b.estimator_step_host(device.baseLinearAcceleration, device.baseAngularVelocity, device.baseOrientation,
                                  device.q_mes, device.v_mes, gait=gait, goals=goals, true_pos=tp, true_b_vel=tv)
        self._calls += 1
        self.q_filt[:, 0] = o["q_filt"][0]
        self.v_filt[:, 0] = o["v_filt"][0]
        self.v_secu[:] = o["v_secu"][0]
        self.RPY = o["rpy"][0].reshape((3, 1)).copy()
        self.IMU_lin_acc[:] = device.baseLinearAcceleration
        self.feet_status[:] = gait[0, :]
        self.feet_goals[:, :] = goals
        return 0

    # ---- state the reference keeps as attributes: read from the handle when asked for
    def _item(self, name):
        return self._ensure().estimator_get(name)

    FK_lin_vel = property(lambda self: self._item("FK_lin_vel"))
    FK_xyz = property(lambda self: self._item("FK_xyz"))
    xyz_mean_feet = property(lambda self: self._item("xyz_mean_feet"))
    filt_lin_vel = property(lambda self: self._item("filt_lin_vel"))
    k_since_contact = property(lambda self: self._item("k_since_contact"))
    HP_lin_vel = property(lambda self: self._item("HP_lin_vel"))
    LP_lin_vel = property(lambda self: self._item("LP_lin_vel"))
    alpha = property(lambda self: float(self._item("alpha")[0]))
    close_from_contact = property(lambda self: bool(self._item("close_from_contact")[0]))
    offset_yaw_IMU = property(lambda self: float(self._item("offset_yaw_IMU")[0]))
    k_log = property(lambda self: int(self._item("k_log")[0]))

    @property
    def filt_lin_pos(self):
        return self._item("HP_lin_pos") + self._item("LP_lin_pos")

    class _Filter:
        """The state of one ComplementaryFilter (scripts/Estimator.py:184-231) as the handle holds it."""

        def __init__(self, dt, HP_x, LP_x, alpha):
            self.dt, self.HP_x, self.LP_x, self.alpha, self.filt_x = dt, HP_x, LP_x, alpha, HP_x + LP_x

    @property
    def filter_xyz_vel(self):
        return Estimator._Filter(self.dt, self._item("HP_lin_vel"), self._item("LP_lin_vel"), self.alpha)

    @property
    def filter_xyz_pos(self):
        return Estimator._Filter(self.dt, self._item("HP_lin_pos"), self._item("LP_lin_pos"), np.array([0.995, 0.995, 0.9]))

    # what the reference copies from the device before filtering: the same numbers leave in q_filt / v_filt (:597-606)
    IMU_ang_pos = filt_ang_pos = property(lambda self: self.q_filt[3:7, 0].copy())
    IMU_ang_vel = filt_ang_vel = property(lambda self: self.v_filt[3:6, 0].copy())
    actuators_pos = property(lambda self: self.q_filt[7:, 0].copy())
    actuators_vel = property(lambda self: self.v_filt[6:, 0].copy())

    # ---- conversions the reference's callers use (scripts/Controller.py:401)
    def cross3(self, left, right):
        return np.array([[left[1] * right[2] - left[2] * right[1]],
                         [left[2] * right[0] - left[0] * right[2]],
                         [left[0] * right[1] - left[1] * right[0]]])

    def EulerToQuaternion(self, roll_pitch_yaw):
        """scripts/Estimator.py:672-684"""
        roll, pitch, yaw = roll_pitch_yaw
        sr, cr = np.sin(roll / 2.), np.cos(roll / 2.)
        sp, cp = np.sin(pitch / 2.), np.cos(pitch / 2.)
        sy, cy = np.sin(yaw / 2.), np.cos(yaw / 2.)
        return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                cr * cp * cy + sr * sp * sy]

    def quaternionToRPY(self, quat):
        """scripts/Estimator.py:686-714"""
        qx, qy, qz, qw = quat[0], quat[1], quat[2], quat[3]
        a0, a1 = 2.0 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz
        rx = np.arctan2(a0, a1) if (a0 != 0.0) and (a1 != 0.0) else 0.0
        a0 = -2.0 * (qx * qz - qw * qy)
        ry = np.pi / 2.0 if a0 >= 1.0 else -np.pi / 2.0 if a0 <= -1.0 else np.arcsin(a0)
        a0, a1 = 2.0 * (qx * qy + qw * qz), qw * qw + qx * qx - qy * qy - qz * qz
        rz = np.arctan2(a0, a1) if (a0 != 0.0) and (a1 != 0.0) else 0.0
        return np.array([[rx], [ry], [rz]])
