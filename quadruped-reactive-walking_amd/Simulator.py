"""A fleet of simulated Solo12 robots on the device: what closes the loop around Controller_batch.

    sim = Simulator_batch(B, q_init)                       # first measurement in sim.sensors
    ctl = Controller_batch(B, q_init, estimator=dict(h_init=...))
    r = ctl.compute_sensors(joy, **sim.sensors)
    for k in range(n):
        sim.step(r)                                        # SendCommand + the next UpdateMeasurment, one kernel
        r = ctl.compute_sensors(joy, **sim.sensors)        # estimator + control iteration on the same tensors

One tick is qrw_sim_step (csrc/sim_kernel.hip): the reference's PD+ law (scripts/PyBulletSimulator.py:679-688), `substeps`
semi-implicit Euler steps of the forward dynamics with penalty contact on a flat plane, and the readings of UpdateMeasurment
(:588-633) in the layouts the estimator takes.  NOT PyBullet: no constraint solver, no joint limits.

Rough ground: terrain=dict(heights=(rows, cols), dx=, dy=, x0=, y0=) puts ONE triangulated heightfield under the whole fleet
(qrw_sim_set_terrain; the contact law is the plane's, taken along the normal of the triangle under each foot), terrain_origin=
(B,2) looks it up at an offset per robot, so that every robot walks a patch of its own while its own coordinates start at 0.
reference_rough_ground() is the field the reference builds for use_flat_plane=False.  The terrain is the fleet's own model, not
Bullet's heightfield collision; outside the field the surface continues as the clamped edge (unphysical).
The single-robot, reference-named drop-in is PyBulletSimulator.py.  Stream groups (Controller_groups) are not supported: every
group steps on streams of its own, the simulator is one launch on one stream."""
import numpy as np

import qrw_hip


class Simulator_batch:
    def __init__(self, batch, q_init, dt=0.002, controller=None, device=0, terrain=None, terrain_origin=None, **params):
        """q_init: (12,) / (19,) for every robot, or (B,12) / (B,19) (12: the joints, base level at base_height).  params: substeps,
        kn, dn, mu, vs, foot_radius, base_height (qrw_hip.SIM_DEFAULTS).  controller: the single-handle Controller_batch it will be
        stepped against; its handle then holds the simulator's state too (a Controller_groups is refused).  terrain: None (the
        plane z = 0) or dict(heights=, dx=, dy=, x0=0, y0=0), numpy or CUDA float64; terrain_origin: (B,2) or None (see above).
        With 12-joint q_init the level base then starts base_height above the highest ground under its feet."""
        import torch

        check_controller(controller)
        terrain = check_terrain(terrain, terrain_origin)
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
        if terrain is not None:
            self.set_terrain(origin=terrain_origin, **terrain)
        self.reset()

    def set_terrain(self, heights, dx, dy, x0=0.0, y0=0.0, origin=None):
        """A (new) heightfield under the fleet, from the next tick or reset() on.  Enqueues on the current stream for CUDA tensors."""
        self._b.sim_set_terrain(heights, dx, dy, x0=x0, y0=y0, origin=origin)

    def clear_terrain(self):
        """Back to the plane z = 0."""
        self._b.sim_clear_terrain()

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


def check_terrain(terrain, terrain_origin):
    """terrain=: None or a dict with heights, dx, dy and optionally x0, y0; unknown or missing keys are refused before anything
    is allocated.  Returns the dict (a copy) or None."""
    if terrain is None:
        if terrain_origin is not None:
            raise ValueError("terrain_origin= without terrain=")
        return None
    terrain = dict(terrain)
    unknown, missing = set(terrain) - {"heights", "dx", "dy", "x0", "y0"}, {"heights", "dx", "dy"} - set(terrain)
    if unknown or missing:
        raise ValueError("terrain=: unknown keys %s, missing keys %s (heights, dx, dy, x0, y0)" % (sorted(unknown), sorted(missing)))
    return terrain


def reference_rough_ground(center=True):
    """The heightfield the reference builds for use_flat_plane=False (scripts/PyBulletSimulator.py:43-61), as
    dict(heights (512,512), dx=0.05, dy=0.05, x0, y0) for Simulator_batch(terrain=...).

    Restated: Python's random.seed(41) (:44); for j over 256 column pairs, for i over 256 row pairs (:52-53), one
    random.uniform(0, 0.05) per (j, i) (:55); the flat list holds, at 2i + 2j*512 and 2i + (2j+1)*512, the mean of this draw and the
    previous one, and at 2i+1 + 2j*512 and 2i+1 + (2j+1)*512 the draw itself (:57-60); height_prev starts at 0 and carries over
    from one j to the next (:51, :61).  The flat list is taken as [row][column] with the column (x) running fastest, and
    meshScale (.05, .05, 1) (:64) makes the cells 5 cm: 512 x 512 samples centred on the origin, x0 = y0 = -0.05 * 511 / 2.

    Unpinned assumption (no Bullet in this project to check against): Bullet centres a heightfield's local frame on the middle of
    its height range, so the body placed at z = 0 (:70) shows heights shifted by -(min + max)/2.  center=True applies that
    shift; center=False returns the raw values in [0, 0.05]."""
    import random

    n, amp = 512, 0.05
    rng = random.Random(41)  # (the generator random.seed(41) seeds, without touching the caller's global one)
    flat = np.zeros(n * n)
    prev = 0.0
    for j in range(n // 2):
        for i in range(n // 2):
            height = rng.uniform(0, amp)
            mean = (height + prev) * 0.5
            flat[2 * i + 2 * j * n] = flat[2 * i + (2 * j + 1) * n] = mean
            flat[2 * i + 1 + 2 * j * n] = flat[2 * i + 1 + (2 * j + 1) * n] = height
            prev = height
    heights = flat.reshape(n, n)
    if center:
        heights = heights - 0.5 * (heights.min() + heights.max())
    half = -0.5 * 0.05 * (n - 1)
    return dict(heights=heights, dx=0.05, dy=0.05, x0=half, y0=half)


def check_controller(obj):
    """Stream groups are out of the simulator's scope: say so instead of stepping a fleet whose groups run on other streams."""
    if obj is None:
        return
    for klass in type(obj).__mro__:
        if klass.__name__ == "Controller_groups":
            raise ValueError("Simulator_batch does not support Controller_groups (stream groups): step a single-handle "
                             "Controller_batch(..., groups=1) against it")
