"""Drop-in for the device class of the reference's scripts/PyBulletSimulator.py (`PyBulletSimulator`, :525-733) for ONE robot,
on a batch-1 handle of libqrw_hip.so (qrw_sim_init_host / qrw_sim_step_host -> sim_kernel.hip).  The fleet path is
Simulator.Simulator_batch.

Provided: Init, UpdateMeasurment, SetDesiredJointTorque / SetDesiredJointPDgains / SetDesiredJointPosition /
SetDesiredJointVelocity, SendCommand, Stop, cross3, the measurement attributes of :538-555, dummyPos, dummyHeight, b_baseVel,
rot_oMb, hardware.roll / pitch / yaw and cpt.
NOT PyBullet: the physics step is the project's own (penalty contact on a flat plane, no joint limits, no joint friction), so
nothing about PyBullet's numerics is reproduced.  envID != 0, use_flat_plane=False and enable_pyb_GUI=True raise
NotImplementedError; the pybullet_simulator helper class (:18-497: environments, debug shapes, camera, apply_external_force by
time window) is not provided -- SendCommand takes an optional external wrench instead.
One tick of the handle is SendCommand FOLLOWED BY the next UpdateMeasurment, so SendCommand computes both and UpdateMeasurment
publishes the readings that are waiting, in the reference's order of calls (:588, :635-670, :672)."""
import time

import numpy as np

import qrw_hip


def quaternionToRPY(quat):
    """scripts/Estimator.py:686-714 (imported by the reference from utils_mpc)."""
    qx, qy, qz, qw = quat
    rx = ry = rz = 0.0
    xa0, xa1 = 2.0 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz
    if xa0 != 0.0 and xa1 != 0.0:
        rx = np.arctan2(xa0, xa1)
    ya0 = -2.0 * (qx * qz - qw * qy)
    ry = np.pi / 2.0 if ya0 >= 1.0 else (-np.pi / 2.0 if ya0 <= -1.0 else np.arcsin(ya0))
    za0, za1 = 2.0 * (qx * qy + qw * qz), qw * qw + qx * qx - qy * qy - qz * qz
    if za0 != 0.0 and za1 != 0.0:
        rz = np.arctan2(za0, za1)
    return np.array([[rx], [ry], [rz]])


class Hardware:
    """scripts/PyBulletSimulator.py:494-522."""

    def __init__(self):
        self.is_timeout = False
        self.roll = 0.0
        self.pitch = 0.0
        self.yaw = 0.0

    def IsTimeout(self):
        return self.is_timeout

    def Stop(self):
        return 0

    def imu_data_attitude(self, i):
        return (self.roll, self.pitch, self.yaw)[i] if i in (0, 1, 2) else None


class PyBulletSimulator:
    def __init__(self):
        # (:532-555)
        self.cpt = 0
        self.nb_motors = 12
        self.jointTorques = np.zeros(self.nb_motors)
        self.revoluteJointIndices = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]
        self.hardware = Hardware()
        self.q_mes = np.zeros(12)
        self.v_mes = np.zeros(12)
        self.torquesFromCurrentMeasurment = np.zeros(12)
        self.baseAngularVelocity = np.zeros(3)
        self.baseOrientation = np.zeros(4)
        self.baseLinearAcceleration = np.zeros(3)
        self.baseAccelerometer = np.zeros(3)
        self.o_baseVel = np.zeros((3, 1))
        self.o_imuVel = np.zeros((3, 1))
        self.prev_o_imuVel = np.zeros((3, 1))
        self.P = 0.0
        self.D = 0.0
        self.q_des = np.zeros(12)
        self.v_des = np.zeros(12)
        self.tau_ff = np.zeros(12)
        self.contact_forces = np.zeros((4, 3))
        self._b = None
        self._pending = None

    def Init(self, calibrateEncoders=False, q_init=None, envID=0, use_flat_plane=True, enable_pyb_GUI=False, dt=0.002, **params):
        """(:557-575)  params: the simulator's own (substeps, kn, dn, mu, vs, foot_radius, base_height)."""
        if envID != 0:
            raise NotImplementedError("PyBulletSimulator.Init(envID=%r): only the flat plane (envID 0) is provided" % (envID,))
        if not use_flat_plane:
            raise NotImplementedError("PyBulletSimulator.Init(use_flat_plane=False): the rough ground is not provided")
        if enable_pyb_GUI:
            raise NotImplementedError("PyBulletSimulator.Init(enable_pyb_GUI=True): there is no PyBullet, hence no GUI")
        if q_init is None:
            raise ValueError("PyBulletSimulator.Init: q_init (12 joint angles) is needed")
        self.q_init = np.asarray(q_init, dtype=np.float64).ravel()
        self.dt = float(dt)
        if self._b is not None:
            self._b.close()
        self._b = qrw_hip.Batch(1, dt_wbc=self.dt)
        self._pending = self._b.sim_init_host(self.q_init.reshape(1, -1), dt=self.dt, **params)
        self.cpt = 0
        self.time_loop = time.time()

    def cross3(self, left, right):
        """(:577-586)"""
        return np.array([[left[1] * right[2] - left[2] * right[1]],
                         [left[2] * right[0] - left[0] * right[2]],
                         [left[0] * right[1] - left[1] * right[0]]])

    def UpdateMeasurment(self):
        """(:588-633): publish the readings of the state the last SendCommand (or Init) left."""
        o = self._pending
        self.q_mes[:] = o["q_mes"][0]
        self.v_mes[:] = o["v_mes"][0]
        self.torquesFromCurrentMeasurment[:] = self.jointTorques[:].ravel()   # (:598)
        self.dummyPos = o["true_pos"][0].copy()                                # (:604)
        self.dummyHeight = self.dummyPos.copy()
        self.dummyHeight[2] = 0.20                                             # (:603)
        self.baseOrientation[:] = o["quat"][0]                                 # (:611)
        RPY = quaternionToRPY(self.baseOrientation)
        self.hardware.roll, self.hardware.pitch, self.hardware.yaw = RPY[0], RPY[1], RPY[2]
        x, y, z, w = self.baseOrientation
        self.rot_oMb = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        self.baseAngularVelocity[:] = o["ang_vel"][0]                          # (:620)
        self.b_baseVel = o["true_b_vel"][0].copy()                             # (:624)
        self.o_baseVel = (self.rot_oMb @ self.b_baseVel).reshape(3, 1)         # (:623)
        self.prev_o_imuVel[:, 0] = self.o_imuVel[:, 0]
        self.o_imuVel = o["o_imu_vel"][0].reshape(3, 1).copy()                 # (:626)
        self.baseLinearAcceleration[:] = o["lin_acc"][0]                       # (:628)
        self.baseAccelerometer[:] = self.baseLinearAcceleration + self.rot_oMb.T @ np.array([0.0, 0.0, -9.81])  # (:630-631)
        self.contact_forces = o["contact_forces"][0].copy()

    def SetDesiredJointTorque(self, torques):
        self.tau_ff = np.asarray(torques, dtype=np.float64).copy()

    def SetDesiredJointPDgains(self, P, D):
        self.P = P
        self.D = D

    def SetDesiredJointPosition(self, q_des):
        self.q_des = q_des

    def SetDesiredJointVelocity(self, v_des):
        self.v_des = v_des

    def SendCommand(self, WaitEndOfCycle=True, f_ext=None):
        """(:672-710)  f_ext: optional world force and moment (6,) at the base origin during this tick (the reference's
        apply_external_force, :402-431, without its time window)."""
        fe = None if f_ext is None else np.asarray(f_ext, dtype=np.float64).reshape(1, 6)
        o = self._b.sim_step_host(self.P, self.D, np.ravel(self.q_des), np.ravel(self.v_des), np.ravel(self.tau_ff), f_ext=fe)
        self.jointTorques = o["joint_torques"][0].copy()                       # (:688)
        self._pending = o
        if WaitEndOfCycle:
            while (time.time() - self.time_loop) < self.dt:
                pass
            self.cpt += 1
        self.time_loop = time.time()

    @property
    def status(self):
        """0, or 1 once the state stopped being finite (the robot is frozen from then on)."""
        return int(self._b.sim_state()["status"][0])

    def Stop(self):
        """(:726-733)"""
        if self._b is not None:
            self._b.close()
            self._b = None
