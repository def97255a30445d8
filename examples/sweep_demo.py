#!/usr/bin/env python3
"""The reference's analysis sweep as ONE fleet: a grid of target velocities (vx, yaw rate), one robot per cell, closed loop.

    python examples/sweep_demo.py [nx=25] [nw=25] [--vmax=1.5] [--wmax=2.0]

The reference maps its grid over a process pool, one PyBullet simulation per target (crocoddyl_eval/test_4/run_scenarios.py with
scripts/main_solo12_control.py:113-129 and Joystick.update_for_analysis): every run accelerates to its target at 0.1 m/s^2, holds
it for 3 s and reports whether the controller survived.  Here the nx * nw runs are the robots of one Controller_batch, stepped
against Simulator_batch; the per-robot profiles live on the device (Joystick.Joystick_batch.for_analysis), so a tick is
joystick stage -> estimator -> control iteration -> simulator with no host arithmetic and no upload.  Unpaced, synchronous MPC.

Printed: the survival map -- per cell the tick at which the robot's error flag rose (k_stop), `.` for a robot that finished, `#`
for one the simulator froze --, the simulator status, the distance covered, and the wall time of the sweep.  The robot model file
is unpinned and the contact law is NOT PyBullet's (Simulator.py): the map says what THIS fleet does, not what the reference
would."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from Controller import Controller_batch  # noqa: E402
from Joystick import Joystick_batch  # noqa: E402
from Simulator import Simulator_batch  # noqa: E402

opt = {a.split("=")[0]: float(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--") and "=" in a}
argv = [a for a in sys.argv[1:] if not a.startswith("--")]
nx, nw = (int(argv[0]) if len(argv) > 0 else 25), (int(argv[1]) if len(argv) > 1 else 25)
vmax, wmax = opt.get("--vmax", 1.5), opt.get("--wmax", 2.0)
max_ticks = int(opt.get("--ticks", 0))  # (0: the whole scenario; a smaller number cuts the sweep short)
B, dt = nx * nw, 0.002
q_init = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])  # scripts/main_solo12_control.py:111

des = np.zeros((B, 6))
vx, wz = np.meshgrid(np.linspace(0.0, vmax, nx), np.linspace(-wmax, wmax, nw) if nw > 1 else np.zeros(1), indexing="ij")
des[:, 0], des[:, 5] = vx.reshape(-1), wz.reshape(-1)
dev = torch.device("cuda", 0)
with torch.cuda.stream(torch.cuda.Stream(dev)):
    ctl = Controller_batch(B, q_init, dt_wbc=dt, estimator=dict(h_init=0.22294615))
    sim = Simulator_batch(B, q_init, dt=dt, controller=ctl)
    joy, n_sim = Joystick_batch.for_analysis(ctl, des, dt)
    ticks = min(n_sim, max_ticks) if max_ticks else n_sim
    torch.cuda.current_stream().synchronize()
    t0 = time.perf_counter()
    for k in range(ticks):
        joy.step(k)
        r = ctl.compute_sensors(joy.v_ref, **sim.sensors, joystick_code=joy.code)
        sim.step(r, f_ext=joy.f_ext)
    torch.cuda.current_stream().synchronize()
    wall = time.perf_counter() - t0
    k_stop, st, flags = joy.k_stop(), sim.state(), ctl.error_flag.cpu().numpy()

finished = (k_stop < 0) & (st["status"] == 0)
print("%d x %d targets (vx 0..%.2f m/s, yaw rate %+.2f..%+.2f rad/s) = %d robots, %d ticks of %.0f ms (%.1f s simulated each): "
      "wall time %.2f s, %.1f us per fleet tick, %.0f robot-ticks/s"
      % (nx, nw, vmax, -wmax, wmax, B, ticks, 1e3 * dt, ticks * dt, wall, 1e6 * wall / ticks, B * ticks / wall))
print("survival map (rows: vx, columns: yaw rate; k_stop in hundreds of ticks, '.' finished, '#' frozen by the simulator):")
for i in range(nx):
    cells = []
    for j in range(nw):
        b = i * nw + j
        cells.append("  #" if st["status"][b] else "  ." if k_stop[b] < 0 else "%3d" % (k_stop[b] // 100))
    print("vx %.2f |%s" % (vx[i, 0], "".join(cells)))
dist = np.hypot(st["q"][:, 0], st["q"][:, 1])
print("finished %d of %d; stopped by the controller's error flag %d (codes %s), frozen by the simulator %d; distance covered by the "
      "finished robots: median %.2f m, max %.2f m; base height of the finished robots: median %.3f m, %d below 0.12 m"
      % (int(finished.sum()), B, int((k_stop >= 0).sum()), dict(zip(*[x.tolist() for x in np.unique(flags[flags != 0], return_counts=True)])),
         int((st["status"] != 0).sum()), float(np.median(dist[finished])) if finished.any() else float("nan"),
         float(dist[finished].max()) if finished.any() else float("nan"),
         float(np.median(st["q"][finished, 2])) if finished.any() else float("nan"), int((st["q"][finished, 2] < 0.12).sum())))
