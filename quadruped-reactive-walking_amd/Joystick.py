"""Per-robot joystick scenarios on the device: the first stage of a fleet's control iteration.

    ctl = Controller_batch(B, q_init, estimator=dict(h_init=...))
    sim = Simulator_batch(B, q_init, controller=ctl)
    joy, n = Joystick_batch.for_analysis(ctl, des_vel, dt_wbc=0.002)      # or Joystick_batch(ctl, profiles=[...], pushes=[...])
    for k in range(n):
        joy.step(k)                                                        # qrw_joystick_step: v_ref, code, f_ext of tick k
        r = ctl.compute_sensors(joy.v_ref, **sim.sensors, joystick_code=joy.code)
        sim.step(r, f_ext=joy.f_ext)
    joy.k_stop()                                                           # per robot: the tick its error flag rose, -1 = finished

One step is qrw_joystick_step (csrc/joystick_kernel.hip) for scripts/Joystick.py's update_v_ref (scripts/Controller.py:210): the
velocity profiles of handle_v_switch (:160-190), the ramps of update_v_ref_multi_simu (:289-315) or the gamepad's low-pass filter
(:135-137), the one-shot gait codes of computeCode (:144-158) and the pushes of apply_external_force
(scripts/PyBulletSimulator.py:402-431), every robot with tables of its own.  The three output tensors never move, so the
controller's bound iteration stays bound.  A robot whose error flag rises gets zero outputs from that tick on (k_stop()).

Not here: the gamepad client (gamepad_command() below is its stick mapping, the values come from the caller), the `reduced` flag,
joystick.stop reaching the controller's security branch, a single-robot reference-named Joystick class, the velID tables."""
import numpy as np

import qrw_hip


def gamepad_command(left_x, left_y, right_x, l1=False):
    """The stick mapping of update_v_ref_gamepad (scripts/Joystick.py:94-103): stick values in [-1, 1] (scalars or (B,) arrays)
    -> the unfiltered command v_gp (6,) or (B,6).  l1: the orientation of the base is commanded instead of its velocity."""
    vX, vY, vYaw = np.asarray(left_x) * 0.6, np.asarray(left_y) * 1.2, np.asarray(right_x) * 1.6
    zero = np.zeros_like(vX + vY + vYaw)
    cols = [zero, zero, -vYaw * 0.25, -vX * 5, -vY * 2, zero] if l1 else [-vY, -vX, zero, zero, zero, -vYaw]
    return np.stack(np.broadcast_arrays(*cols), axis=-1).astype(np.float64)


def pad_profiles(profiles, B):
    """B pairs (k_switch (n,), v_switch (6,n)) -> (B,n_max) int32 and (B,6,n_max) float64, shorter tables padded by repeating
    their last column (never selected as a segment: bit-neutral)."""
    if len(profiles) != B:
        raise ValueError("profiles=: one (k_switch, v_switch) pair per robot (%d given, batch %d)" % (len(profiles), B))
    pairs = []
    for b, (ks, vs) in enumerate(profiles):
        ks, vs = np.asarray(ks, dtype=np.int64).reshape(-1), np.asarray(vs, dtype=np.float64)
        if ks.size < 1 or vs.shape != (6, ks.size):
            raise ValueError("profiles=: robot %d: k_switch (n,) with n >= 1 and v_switch (6,n)" % b)
        pairs.append((ks, vs))
    n = max(ks.size for ks, _ in pairs)
    if n > qrw_hip.JOY_MAX_SWITCH:
        raise ValueError("profiles=: at most %d columns" % qrw_hip.JOY_MAX_SWITCH)
    K, V = np.empty((B, n), np.int32), np.empty((B, 6, n))
    for b, (ks, vs) in enumerate(pairs):
        K[b, :ks.size], K[b, ks.size:] = ks, ks[-1]
        V[b, :, :ks.size], V[b, :, ks.size:] = vs, vs[:, -1:]
    return K, V


def pad_codes(codes, B):
    """B lists of (tick, code) -> two (B,n_max) int32; unused entries carry tick -1, which never fires."""
    if len(codes) != B:
        raise ValueError("codes=: one list of (tick, code) pairs per robot")
    n = max([len(c) for c in codes] + [0])
    if n > qrw_hip.JOY_MAX_CODES:
        raise ValueError("codes=: at most %d pairs per robot" % qrw_hip.JOY_MAX_CODES)
    K, V = np.full((B, n), -1, np.int32), np.zeros((B, n), np.int32)
    for b, pairs in enumerate(codes):
        for e, (k, code) in enumerate(pairs):
            if int(k) < 0:
                raise ValueError("codes=: robot %d: ticks are >= 0" % b)
            K[b, e], V[b, e] = int(k), int(code)
    return K, V


PUSH_PAD = (-(1 << 30), 1)  # an unused entry's window: over long before tick 0


def pad_pushes(pushes, B):
    """B lists of (start, duration, F (3,), M (3,)) -> (B,n_max,2) int32 and (B,n_max,6) float64."""
    if len(pushes) != B:
        raise ValueError("pushes=: one list of (start, duration, F, M) per robot")
    n = max([len(p) for p in pushes] + [0])
    if n > qrw_hip.JOY_MAX_PUSHES:
        raise ValueError("pushes=: at most %d per robot" % qrw_hip.JOY_MAX_PUSHES)
    K, W = np.empty((B, n, 2), np.int32), np.zeros((B, n, 6))
    K[:] = PUSH_PAD
    for b, entries in enumerate(pushes):
        for e, (start, duration, F, M) in enumerate(entries):
            K[b, e] = (int(start), int(duration))
            W[b, e, :3], W[b, e, 3:] = np.asarray(F, dtype=np.float64), np.asarray(M, dtype=np.float64)
    return K, W


class Joystick_batch:
    def __init__(self, controller, profiles=None, ramp=None, gamepad=None, codes=None, pushes=None):
        """controller: the single-handle Controller_batch the stage feeds (it works on that controller's own handle, as
        Simulator_batch does; a Controller_groups is refused), or a qrw_hip.Batch.  Exactly one of
          profiles=[(k_switch (n,), v_switch (6,n)), ...]   one pair per robot, n <= 32, k_switch non-decreasing from <= 0
          ramp=dict(v=(B,3) Vx Vy Vw, k_start=480)          the reference's k_start is k_mpc * 16 * 3
          gamepad=True | dict(alpha=, deadband=)            step(k, v_gp=...) then takes the command of the tick
        and optionally codes=[[(tick, code), ...], ...] and pushes=[[(start, duration, F (3,), M (3,)), ...], ...], one list per
        robot.  The library validates the tables: qrw_hip.QrwError names the robot and the entry."""
        import torch

        from Simulator import check_controller

        check_controller(controller)
        self._ctl = controller if hasattr(controller, "_b") else None
        self._b = controller._b if self._ctl is not None else controller
        if not isinstance(self._b, qrw_hip.Batch):
            raise ValueError("Joystick_batch: a single-handle Controller_batch or a qrw_hip.Batch")
        self.B = B = self._b.B
        if sum(x is not None and x is not False for x in (profiles, ramp, gamepad)) != 1:
            raise ValueError("Joystick_batch: exactly one of profiles=, ramp=, gamepad=")
        kw = {}
        if profiles is not None:
            self.mode = qrw_hip.JOY_PROFILE
            kw["k_switch"], kw["v_switch"] = pad_profiles(profiles, B)
        elif ramp is not None:
            self.mode = qrw_hip.JOY_RAMP
            ramp = dict(ramp) if isinstance(ramp, dict) else dict(v=ramp)
            if set(ramp) - {"v", "k_start"} or "v" not in ramp:
                raise ValueError("ramp=: dict(v=(B,3), k_start=480)")
            kw["ramp_v"], kw["k_start"] = np.asarray(ramp["v"], dtype=np.float64).reshape(B, 3), int(ramp.get("k_start", 480))
        else:
            self.mode = qrw_hip.JOY_GAMEPAD
            gp = {} if gamepad is True else dict(gamepad)
            if set(gp) - {"alpha", "deadband"}:
                raise ValueError("gamepad=: True or dict(alpha=, deadband=)")
            kw["gp_alpha"], kw["gp_deadband"] = gp.get("alpha", qrw_hip.JOY_GP_ALPHA), gp.get("deadband", qrw_hip.JOY_GP_DEADBAND)
        if codes is not None:
            kw["code_k"], kw["code_v"] = pad_codes(codes, B)
        if pushes is not None:
            kw["push_k"], kw["push_w"] = pad_pushes(pushes, B)
        self._tables = kw
        dev = torch.device("cuda", self._b.device)
        # the three tensors the consumers read; they never move (Controller_batch's bound iteration recognises them by identity)
        self.v_ref = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        self.code = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.f_ext = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        self.reset()

    def reset(self):
        """Re-initialise: the same tables, the filter state zero, k_stop -1 (qrw_joystick_init again)."""
        self._b.joystick_init(self.mode, **self._tables)

    def step(self, k, v_gp=None):
        """The stage for tick k on the current stream: v_ref, code and f_ext are rewritten.  v_gp (B,6) CUDA float64: the gamepad
        command of the tick (that mode only).  The stop flags are the controller's error_flag tensor once it exists."""
        stop = getattr(self._ctl, "error_flag", None)
        self._b.joystick_step(k, self.v_ref, code=self.code, f_ext=self.f_ext, v_gp=v_gp, stop=stop)
        return self.v_ref, self.code, self.f_ext

    def k_stop(self):
        """(B,) int64: the tick at which each robot's error flag was first seen, -1 for a robot that never stopped (the
        reference's control_loop returning `finished`).  Synchronises with the last step."""
        return self._b.joystick_get("k_stop")

    def filter_state(self, b=0):
        """The gamepad filter's v_ref of robot b, (6,)."""
        return self._b.joystick_get("v_ref", b)

    @classmethod
    def for_analysis(cls, controller, des_vel, dt_wbc, acceleration_rate=0.1, steady=3.0, **kw):
        """The analysis scenario of scripts/main_solo12_control.py:113-119 + Joystick.update_for_analysis (:317-326) per robot:
        des_vel (B,6) -> k_switch [0, 500, N_analysis, N_analysis + N_steady], v_switch [0, 0, des_vel, des_vel] with
        N_analysis = int(max|des_vel| / acceleration_rate / dt_wbc) + 1, N_steady = int(steady / dt_wbc).  Returns
        (Joystick_batch, N_SIMULATION): the largest N_analysis + N_steady of the fleet (a robot whose own run is shorter holds
        its target).  A target so slow that N_analysis < 500 leaves the reference's table out of order; its scan then jumps to
        des_vel at tick 500 and holds it, which the ordered table [0, 500, 500, N_analysis + N_steady] gives bit for bit."""
        des = np.asarray(des_vel, dtype=np.float64)
        B = des.shape[0]
        if des.shape != (B, 6):
            raise ValueError("for_analysis: des_vel (B,6)")
        n_steady = int(steady / dt_wbc)
        profiles, n_sim = [], 0
        for b in range(B):
            n_analysis = int(np.max(np.abs(des[b])) / acceleration_rate / dt_wbc) + 1
            if n_analysis + n_steady < 500:
                raise ValueError("for_analysis: robot %d: N_analysis + N_steady < 500" % b)
            v = np.zeros((6, 4))
            v[:, 2] = v[:, 3] = des[b]
            profiles.append(([0, 500, max(n_analysis, 500), n_analysis + n_steady], v))
            n_sim = max(n_sim, n_analysis + n_steady)
        return cls(controller, profiles=profiles, **kw), n_sim
