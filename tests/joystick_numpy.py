"""Checker of the joystick stage: a numpy restatement of scripts/Joystick.py and scripts/PyBulletSimulator.py:402-431 that keeps
the reference's STATEFUL form -- one object per robot, v_ref persists between calls, handle_v_switch's scan, apply_external_force's
window test, computeCode's one-shot -- so that the kernel's stateless evaluation is held against the original's behaviour, the hold
after the last switch included.  Written from those lines (cited below); it imports nothing of the reference.

The operations are numpy's and Python's own: int64 powers converted to double, true division, float64 + - * /, every one correctly
rounded once -- the sequence csrc/joystick_profile.h evaluates with contraction off."""
import numpy as np


class JoystickNumpy:
    """One robot.  update_v_ref(k) as scripts/Joystick.py:60-79 dispatches it; the result is self.v_ref (6,) and
    self.joystick_code; apply_external_forces(k) returns the tick's wrench (6,)."""

    def __init__(self, k_switch=None, v_switch=None, ramp=None, k_start=0, gamepad=False, alpha=0.0020 / 0.02, deadband=0.005,
                 codes=(), pushes=()):
        self.v_ref = np.zeros(6)  # (:17)
        self.alpha = alpha        # (:27-29: dT / tc)
        self.deadband = deadband
        self.joystick_code = 0    # (:58)
        self.mode = "profile" if k_switch is not None else ("ramp" if ramp is not None else "gamepad")
        assert (self.mode == "gamepad") == bool(gamepad)
        if self.mode == "profile":
            self.k_switch = np.asarray(k_switch, dtype=np.int64)
            self.v_switch = np.asarray(v_switch, dtype=np.float64).reshape(6, self.k_switch.shape[0])
        if self.mode == "ramp":
            self.Vx_ref, self.Vy_ref, self.Vw_ref = (float(x) for x in ramp)  # (:49-51)
            self.k_start = int(k_start)                                        # (:303: self.k_mpc*16*3)
        self.codes = [(int(k), int(c)) for k, c in codes]
        self.pushes = [(int(s), int(d), np.asarray(F, dtype=np.float64), np.asarray(M, dtype=np.float64)) for s, d, F, M in pushes]
        self.buttons = [False] * 4  # north, east, south, west (:54-57)

    # ---- scripts/Joystick.py:160-190
    def handle_v_switch(self, k):
        i = 1
        while (i < self.k_switch.shape[0]) and (self.k_switch[i] <= k):  # (:167-169)
            i += 1
        if i != self.k_switch.shape[0]:                                    # (:170)
            self.apply_velocity_change(k, i)

    def apply_velocity_change(self, k, i):
        ev = k - self.k_switch[i - 1]                                      # (:183)
        t1 = self.k_switch[i] - self.k_switch[i - 1]                       # (:184)
        A3 = 2 * (self.v_switch[:, i - 1] - self.v_switch[:, i]) / t1**3   # (:185-186)
        A2 = (-3 / 2) * t1 * A3                                            # (:187)
        self.v_ref = self.v_switch[:, i - 1] + A2 * ev**2 + A3 * ev**3     # (:188)

    # ---- :289-315
    def update_v_ref_multi_simu(self, k_loop):
        beta_x = int(max(abs(self.Vx_ref) * 10000, 100.0))                               # (:302)
        alpha_x = np.max([np.min([(k_loop - self.k_start) / beta_x, 1.0]), 0.0])         # (:303)
        beta_y = int(max(abs(self.Vy_ref) * 10000, 100.0))                               # (:305)
        alpha_y = np.max([np.min([(k_loop - self.k_start) / beta_y, 1.0]), 0.0])
        beta_w = int(max(abs(self.Vw_ref) * 2500, 100.0))                                # (:308)
        alpha_w = np.max([np.min([(k_loop - self.k_start) / beta_w, 1.0]), 0.0])
        self.v_ref = np.array([self.Vx_ref * alpha_x, self.Vy_ref * alpha_y, 0.0, 0.0, 0.0, self.Vw_ref * alpha_w])  # (:312-313)

    # ---- :135-137
    def update_v_ref_gamepad(self, v_gp):
        v_gp = np.asarray(v_gp, dtype=np.float64)
        self.v_ref = self.alpha * v_gp + (1 - self.alpha) * self.v_ref                       # (:136)
        self.v_ref[(self.v_ref < self.deadband) & (self.v_ref > -self.deadband)] = 0.0       # (:137)

    # ---- :144-158: a button pressed on tick k gives its code on that tick and is released
    def computeCode(self):
        self.joystick_code = 0
        for n in range(4):
            if self.buttons[n]:
                self.joystick_code = n + 1
                self.buttons[n] = False
                break

    def press_scheduled_buttons(self, k):
        """The schedule stands for the gamepad thread: of the pairs of tick k the LAST one is the button that is down (:114-133
        keep one button at a time); codes above 4 (the walk, 5) have no button in the reference and are passed through."""
        self._direct = None
        for kk, code in self.codes:
            if kk == k:
                self.buttons = [False] * 4
                self._direct = None
                if 1 <= code <= 4:
                    self.buttons[code - 1] = True
                else:
                    self._direct = code

    def update_v_ref(self, k, v_gp=None):
        if self.mode == "ramp":
            self.update_v_ref_multi_simu(k)        # (:70-71)
        elif self.mode == "profile":
            self.handle_v_switch(k)                # (:72-73, :286)
        else:
            self.update_v_ref_gamepad(v_gp)        # (:77)
        self.press_scheduled_buttons(k)
        self.computeCode()                         # (:140)
        if self._direct is not None:
            self.joystick_code = self._direct
        return self.v_ref, self.joystick_code

    # ---- scripts/PyBulletSimulator.py:402-431, called once per entry and tick as at :354-356; Bullet sums the applied wrenches
    def apply_external_force(self, k, start, duration, F, M):
        if (k < start) or (k > (start + duration)):   # (:415)
            return None
        ev = k - start                                 # (:420)
        t1 = duration                                  # (:421)
        A4 = 16 / (t1**4)                              # (:422)
        A3 = - 2 * t1 * A4                             # (:423)
        A2 = t1**2 * A4                                # (:424)
        alpha = A2 * ev**2 + A3 * ev**3 + A4 * ev**4   # (:425)
        return np.concatenate([alpha * F, alpha * M])  # (:429)

    def apply_external_forces(self, k):
        total = np.zeros(6)
        for start, duration, F, M in self.pushes:
            w = self.apply_external_force(k, start, duration, F, M)
            if w is not None:
                total = total + w
        return total


def bell(ev, t1):
    """alpha of apply_external_force alone (F = 1)."""
    return JoystickNumpy(gamepad=True).apply_external_force(ev, 0, t1, np.ones(3), np.zeros(3))[0]


def run(robots, ticks, v_gp=None):
    """Every robot stepped through `ticks` (increasing); returns v_ref (T,B,6), code (T,B), f_ext (T,B,6).  v_gp: (T,B,6)."""
    T, B = len(ticks), len(robots)
    v, c, f = np.empty((T, B, 6)), np.empty((T, B), np.int64), np.empty((T, B, 6))
    for i, k in enumerate(ticks):
        for b, r in enumerate(robots):
            v[i, b], c[i, b] = r.update_v_ref(int(k), None if v_gp is None else v_gp[i, b])
            f[i, b] = r.apply_external_forces(int(k))
    return v, c, f
