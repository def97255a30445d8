"""A fleet of simulated Solo12 robots on the device: what closes the loop around Controller_batch.

    sim = Simulator_batch(B, q_init)                       # first measurement in sim.sensors
    ctl = Controller_batch(B, q_init, estimator=dict(h_init=...))
    r = ctl.compute_sensors(joy, **sim.sensors)
    for k in range(n):
        sim.step(r)                                        # SendCommand + the next UpdateMeasurment, one kernel
        r = ctl.compute_sensors(joy, **sim.sensors)        # estimator + control iteration on the same tensors

One tick is qrw_sim_step (csrc/sim_kernel.hip): the reference's PD+ law (scripts/PyBulletSimulator.py:679-688), `substeps`
semi-implicit Euler steps of the forward dynamics with penalty contact on a flat plane, and the readings of UpdateMeasurment
(:588-633) in the layouts the estimator takes.  NOT PyBullet: no constraint solver, no other terrain, no joint limits.
The single-robot, reference-named drop-in is PyBulletSimulator.py.  Stream groups (Controller_groups) are not supported: every
group steps on streams of its own, the simulator is one launch on one stream."""
import numpy as np

import qrw_hip


class Simulator_batch:
    def __init__(self, batch, q_init, dt=0.002, controller=None, device=0, **params):
        """q_init: (12,) / (19,) for every robot, or (B,12) / (B,19) (12: the joints, base level at base_height).  params: substeps,
        kn, dn, mu, vs, foot_radius, base_height (qrw_hip.SIM_DEFAULTS).  controller: the single-handle Controller_batch it will be
        stepped against; its handle then holds the simulator's state too (a Controller_groups is refused)."""
        import torch

        check_controller(controller)
        self.B = int(batch)
        self.params = dict(params, dt=float(dt))
        qrw_hip.sim_params(**self.params)  # (unknown names are refused before anything is allocated)
        # the controller's own handle when there is one (the simulator's state is one more buffer of it), else a handle of its own
        shared = getattr(controller, "_b", None)
        if shared is not None and shared.B != self.B:
            raise ValueError("Simulator_batch: batch %d, the controller's is %d" % (self.B, shared.B))
        self._own = shared is None
        self._b = qrw_hip.Batch(self.B, dt_wbc=float(dt), device=device) if self._own else shared
        self.dev = torch.device("cuda", self._b.device)
        q = np.asarray(q_init, dtype=np.float64)
        if q.ndim == 1:
            q = np.tile(q, (self.B, 1))
        self._q_init = torch.from_numpy(np.ascontiguousarray(q)).to(self.dev)
        self.out = self._b.sim_outputs()
        # the dict Controller_batch.compute_sensors takes; true_pos / true_b_vel go with a perfect estimator only
        self.sensors = {n: self.out[n] for n in ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")}
        self.sensors_perfect = dict(self.sensors, true_pos=self.out["true_pos"], true_b_vel=self.out["true_b_vel"])
        self.reset()

    def reset(self):
        """Back to q_init at rest (tick and status zero), first measurement rewritten.  Enqueues on the current stream."""
        self._b.sim_init(self._q_init, self.out, **self.params)

    def step(self, command, f_ext=None):
        """One tick for every robot.  command: a Controller Result (P, D, q_des, v_des, tau_ff: read in place from the controller's
        result tensor) or a tuple of those five (B,12) tensors; f_ext: (B,6) world force and moment at the base origin, or None.
        Enqueues on the current stream (under `with torch.cuda.stream(ctl.loop_stream)` in the asynchronous mode); returns the
        output tensors (the same every tick)."""
        check_controller(command)
        if not isinstance(command, (tuple, list)):
            command = (command.P, command.D, command.q_des, command.v_des, command.tau_ff)
        if len(command) != 5:
            raise ValueError("step: a Result or the five tensors P, D, q_des, v_des, tau_ff")
        return self._b.sim_step(*command, self.out, f_ext=f_ext)

    @property
    def status(self):
        """(B,) numpy: 0, or 1 for a robot frozen because its state stopped being finite.  Synchronises with the last tick."""
        return self._b.sim_state()["status"]

    def state(self):
        """dict(q (B,19), v (B,18), prev_o_imuVel (B,3), tick (B,), status (B,)) as numpy arrays; synchronises with the last tick."""
        return self._b.sim_state()

    def set_state(self, q, v, prev_o_imuVel=None, tick=0, status=0):
        """Overwrite the whole state (the measurement tensors are rewritten by the next tick, not here)."""
        prev = np.zeros((self.B, 3)) if prev_o_imuVel is None else prev_o_imuVel
        self._b.sim_set_state(q, v, prev, tick, status)

    def close(self):
        if self._own:
            self._b.close()


def check_controller(obj):
    """Stream groups are out of the simulator's scope: say so instead of stepping a fleet whose groups run on other streams."""
    if obj is None:
        return
    for klass in type(obj).__mro__:
        if klass.__name__ == "Controller_groups":
            raise ValueError("Simulator_batch does not support Controller_groups (stream groups): step a single-handle "
                             "Controller_batch(..., groups=1) against it")
