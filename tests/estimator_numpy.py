"""Independent numpy restatement of the reference's state estimator with the complementary filters (scripts/Estimator.py,
kf_enabled=False) and its perfectEstimator branch: one object per robot.  Test infrastructure: the product never imports it.

The kinematics come from the oracle's rigid-body code (oracle.fixed_feet = rbd_oracle_fixed_feet: fixed-base foot positions and
LOCAL_WORLD_ALIGNED foot velocities, what get_data_FK / BaseVelocityFromKinAndIMU obtain from Pinocchio), a different code path
from the kernel's closed-form leg_kinematics.  The one departure from the reference is the kernel's: the scan for
remaining_steps stops at the number of gait rows (:476-479 raises IndexError there)."""
import numpy as np

import oracle


def filter_alpha(fc, dt):
    """scripts/Estimator.py:254-256 (also :196-197)"""
    y = 1 - np.cos(2 * np.pi * fc * dt)
    return -y + np.sqrt(y * y + 2 * y)


def quaternion_to_rpy(quat):
    """scripts/Estimator.py:686-714"""
    qx, qy, qz, qw = (float(x) for x in quat)
    rotateXa0 = 2.0 * (qy * qz + qw * qx)
    rotateXa1 = qw * qw - qx * qx - qy * qy + qz * qz
    rotateX = 0.0
    if (rotateXa0 != 0.0) and (rotateXa1 != 0.0):
        rotateX = np.arctan2(rotateXa0, rotateXa1)
    rotateYa0 = -2.0 * (qx * qz - qw * qy)
    if rotateYa0 >= 1.0:
        rotateY = np.pi / 2.0
    elif rotateYa0 <= -1.0:
        rotateY = -np.pi / 2.0
    else:
        rotateY = np.arcsin(rotateYa0)
    rotateZa0 = 2.0 * (qx * qy + qw * qz)
    rotateZa1 = qw * qw + qx * qx - qy * qy - qz * qz
    rotateZ = 0.0
    if (rotateZa0 != 0.0) and (rotateZa1 != 0.0):
        rotateZ = np.arctan2(rotateZa0, rotateZa1)
    return np.array([rotateX, rotateY, rotateZ])


def euler_to_quaternion(rpy):
    """scripts/Estimator.py:672-684 (xyzw)"""
    roll, pitch, yaw = rpy
    sr, cr = np.sin(roll / 2.), np.cos(roll / 2.)
    sp, cp = np.sin(pitch / 2.), np.cos(pitch / 2.)
    sy, cy = np.sin(yaw / 2.), np.cos(yaw / 2.)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def rotation_of(quat):
    """pin.Quaternion(xyzw).toRotationMatrix() (scripts/Estimator.py:522) in the homogeneous form
    (w^2 - v.v) I + 2 v v' + 2 w [v]x -- not the expansion the kernel uses."""
    v, w = np.asarray(quat[:3], dtype=np.float64), float(quat[3])
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return (w * w - v @ v) * np.eye(3) + 2.0 * np.outer(v, v) + 2.0 * w * vx


def base_velocity_from_kin_and_imu(p_foot, v_foot, gyro):
    """BaseVelocityFromKinAndIMU (scripts/Estimator.py:642-670): cross(_1F, _1w01) - _1RF _Fv1F; with the base at the origin and
    identity orientation _1RF _Fv1F is the LOCAL_WORLD_ALIGNED foot velocity."""
    return np.cross(p_foot, gyro) - v_foot


def remaining_steps_of(gait):
    """scripts/Estimator.py:476-479, stopping at the last row"""
    n = 1
    while n < gait.shape[0] and np.array_equal(gait[0, :], gait[n, :]):
        n += 1
    return n


def alpha_schedule(k_since_contact, remaining_steps):
    """scripts/Estimator.py:503-517 -> (alpha, close_from_contact)"""
    a = np.ceil(np.max(k_since_contact) / 10) - 1
    b = remaining_steps
    n = 1
    v_max, v_min = 1.00, 0.97
    c = ((a + b) - 2 * n) * 0.5
    if (a <= (n - 1)) or (b <= n):
        return v_max, True
    return v_min + (v_max - v_min) * np.abs(c - (a - n)) / c, False


class ComplementaryFilter:
    """scripts/Estimator.py:184-231"""

    def __init__(self, dt, fc):
        self.dt = dt
        self.alpha = filter_alpha(fc, dt)
        self.HP_x, self.LP_x = np.zeros(3), np.zeros(3)

    def compute(self, x, dx, alpha):
        self.alpha = alpha
        self.HP_x = self.alpha * (self.HP_x + dx * self.dt)
        self.LP_x = self.alpha * self.LP_x + (1.0 - self.alpha) * x
        return self.HP_x + self.LP_x


class Estimator:
    """scripts/Estimator.py:234-629 without the Kalman branch and the logging."""

    def __init__(self, dt, h_init=0.22294615, perfect=False):
        self.dt, self.perfect = dt, bool(perfect)
        self.alpha_v, self.alpha_secu = filter_alpha(50.0, dt), filter_alpha(6.0, dt)   # :254-262
        self.filter_xyz_vel = ComplementaryFilter(dt, 3.0)
        self.filter_xyz_pos = ComplementaryFilter(dt, 500.0)
        self.FK_lin_vel = np.zeros(3)
        self.FK_xyz = np.array([0.0, 0.0, h_init])
        self.xyz_mean_feet = np.zeros(3)
        self.filter_xyz_pos.LP_x[2] = h_init                                              # :283
        self.close_from_contact = False
        self.alpha = 0.0
        self.k_since_contact = np.zeros(4)
        self.filt_lin_vel = np.zeros(3)
        self.q_filt, self.v_filt, self.v_secu = np.zeros(19), np.zeros(18), np.zeros(12)
        self.RPY = np.zeros(3)
        self.offset_yaw_IMU = 0.0
        self.remaining_steps = 0
        self.lever = np.array([0.1163, 0.0, 0.02])                                         # :323-324
        self.k_log = 0

    def run_filter(self, gait, goals, lin_acc, ang_vel, quat, q_mes, v_mes, true_pos=None, true_b_vel=None):
        gait, goals = np.asarray(gait, dtype=np.float64), np.asarray(goals, dtype=np.float64).reshape(3, 4)
        lin_acc, ang_vel = np.asarray(lin_acc, dtype=np.float64), np.asarray(ang_vel, dtype=np.float64)
        q_mes, v_mes = np.asarray(q_mes, dtype=np.float64), np.asarray(v_mes, dtype=np.float64)
        feet_status = gait[0, :].copy()
        self.remaining_steps = remaining_steps_of(gait)
        # get_data_IMU (:347-373)
        self.RPY = quaternion_to_rpy(quat)
        if self.k_log <= 1:
            self.offset_yaw_IMU = self.RPY[2]
        self.RPY[2] -= self.offset_yaw_IMU
        ang_pos = euler_to_quaternion(self.RPY)
        # contact counters (:494-495), before the forward kinematics
        self.k_since_contact += feet_status
        self.k_since_contact *= feet_status
        # get_data_FK (:387-445)
        posf, vf = oracle.fixed_feet(q_mes, v_mes)[:2]
        oRb = rotation_of(ang_pos)
        cpt, vel_est, xyz_est = 0, np.zeros(3), np.zeros(3)
        for i in np.where(feet_status == 1)[0]:
            if self.k_since_contact[i] >= 16:
                cpt += 1
                vel_est += base_velocity_from_kin_and_imu(posf[i], vf[i], ang_vel)
                xyz_est += -(oRb @ posf[i])
                r_foot = 0.025
                if i <= 1:
                    vel_est[0] += r_foot * (v_mes[1 + 3 * i] - v_mes[2 + 3 * i])
                else:
                    vel_est[0] += r_foot * (v_mes[1 + 3 * i] + v_mes[2 + 3 * i])
        if cpt > 0:
            self.FK_lin_vel = vel_est / cpt
            self.FK_xyz = xyz_est / cpt
        # get_xyz_feet (:447-464)
        cpt, xyz_feet = 0, np.zeros(3)
        for i in np.where(feet_status == 1)[0]:
            cpt += 1
            xyz_feet += goals[:, i]
        if cpt > 0:
            self.xyz_mean_feet = xyz_feet / cpt
        # :503-517
        self.alpha, self.close_from_contact = alpha_schedule(self.k_since_contact, self.remaining_steps)
        # cascade of complementary filters (:521-553)
        cross_product = np.cross(self.lever, ang_vel)
        i_FK_lin_vel = self.FK_lin_vel + cross_product
        oi_FK_lin_vel = oRb @ i_FK_lin_vel
        oi_filt_lin_vel = self.filter_xyz_vel.compute(oi_FK_lin_vel, oRb @ lin_acc, alpha=self.alpha)
        i_filt_lin_vel = oRb.T @ oi_filt_lin_vel
        b_filt_lin_vel = i_filt_lin_vel - cross_product
        ob_filt_lin_vel = oRb @ b_filt_lin_vel
        filt_lin_pos = self.filter_xyz_pos.compute(self.FK_xyz + self.xyz_mean_feet, ob_filt_lin_vel,
                                                   alpha=np.array([0.995, 0.995, 0.9]))
        self.filt_lin_vel = b_filt_lin_vel
        # outputs (:594-624)
        self.q_filt[0:3] = filt_lin_pos
        if self.perfect:
            self.q_filt[2] = true_pos[2] - 0.0155
        self.q_filt[3:7] = ang_pos
        self.q_filt[7:] = q_mes
        new = np.asarray(true_b_vel, dtype=np.float64) if self.perfect else self.filt_lin_vel
        self.v_filt[0:3] = (1 - self.alpha_v) * self.v_filt[0:3] + self.alpha_v * new
        self.v_filt[3:6] = ang_vel
        self.v_filt[6:] = v_mes
        self.v_secu = (1 - self.alpha_secu) * v_mes + self.alpha_secu * self.v_secu
        self.k_log += 1
        return 0

    def items(self):
        """The state items qrw_estimator_get_host returns, by the binding's names (qrw_hip.ESTIMATOR_ITEMS)."""
        return dict(k_since_contact=self.k_since_contact, FK_lin_vel=self.FK_lin_vel, FK_xyz=self.FK_xyz,
                    xyz_mean_feet=self.xyz_mean_feet, HP_lin_vel=self.filter_xyz_vel.HP_x, LP_lin_vel=self.filter_xyz_vel.LP_x,
                    HP_lin_pos=self.filter_xyz_pos.HP_x, LP_lin_pos=self.filter_xyz_pos.LP_x, alpha=np.array([self.alpha]),
                    close_from_contact=np.array([float(self.close_from_contact)]),
                    offset_yaw_IMU=np.array([self.offset_yaw_IMU]), k_log=np.array([float(self.k_log)]),
                    filt_lin_vel=self.filt_lin_vel)
