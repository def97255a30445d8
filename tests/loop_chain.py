"""One checker object per robot for the WHOLE control loop: joystick -> estimator -> controller chain -> simulator.  TEST CODE.

It writes no physics of its own.  The stages are the checkers the device's stages are already held to one by one:
  joystick    joystick_numpy.JoystickNumpy, with the stop latch of csrc/joystick_kernel.hip around it (the reference leaves its loop
              at the first error, scripts/main_solo12_control.py:180; the fleet zeroes that robot's three outputs instead)
  estimator   estimator_numpy.Estimator or estimator_kalman_numpy.Estimator
  controller  controller_oracle.ControllerGlue + oracle.Planner / MPC / WbcController, chained as tests/test_gpu_controller.py's
              _closed_loop chains them, the asynchronous delivery bookkeeping (a fixed lag, _shift_last_available) included
  simulator   sim_numpy.SimNumpy or sim_terrain_numpy.SimTerrainNumpy
in the order of the reference's loop (scripts/main_solo12_control.py, scripts/Controller.py:210-236):
  1. the joystick of tick k sees the error flag tick k - 1 left;
  2. the estimator reads the gait and the foot goals BEFORE the planners step (:213-214);
  3. the planners take the joystick's code of this tick (:222);
  4. the MPC runs on k % k_mpc == 0 (:246);
  5. the simulator takes this tick's Result and this tick's push.

tick(k) free-runs: every stage reads the chain's own previous outputs.  tick(k, forced=...) is teacher forcing: every stage reads
the supplied record of ITS inputs (a device's), the simulator through set_state from the recorded previous state; the stateful
stages (estimator, planners, the MPC's warm start, glue, latch) keep their own state and only take forced inputs."""
import copy

import numpy as np

import controller_oracle as co
import estimator_kalman_numpy as ekn
import estimator_numpy as en
import joystick_numpy as jn
import oracle
import sim_numpy as sn
import sim_terrain_numpy as stn

SENSOR_KEYS = ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")
EST_KEYS = ("q_filt", "v_filt", "rpy", "v_secu")
SIM_STATE_KEYS = ("q", "v", "prev_o_imuVel")
SIM_OUT_KEYS = ("q_mes", "v_mes", "quat", "ang_vel", "lin_acc", "o_imu_vel", "true_pos", "true_b_vel", "contact_forces", "joint_torques")


def shift_last_available(res, gait, n_steps):
    """scripts/MPC_Wrapper.py:89-102, as tests/test_gpu_controller.py restates it."""
    res[12:(12 + n_steps), :] = np.roll(res[12:(12 + n_steps), :], -1, axis=1)
    pt = 0
    while np.any(gait[pt, :]):
        pt += 1
    if not np.array_equal(gait[0, :], gait[pt - 1, :]):
        F = 9.81 * 2.5 / np.sum(gait[pt - 1, :])
        res[12:, n_steps - 1] = 0.0
        for i in range(4):
            if gait[pt - 1, i] == 1:
                res[12 + 3 * i + 2, n_steps - 1] = F


def rel(got, ref):
    """|got - ref|_inf relative to max(1, |ref|_inf): the measure of tests/test_gpu_sim.py and of _closed_loop."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max() / max(1.0, np.abs(ref).max()))


def moved_by_one_ulp(x):
    return np.nextafter(np.asarray(x, dtype=np.float64), np.inf)


class LoopChain:
    def __init__(self, cfg, q_init, h_init, profile, codes=(), pushes=(), kalman=False, terrain=None, origin=(0.0, 0.0), lag=None,
                 measure_spread=False):
        """cfg: the controller's timing (tests/test_gpu_controller.py's DEFAULT_CFG); profile: (k_switch, v_switch) of this robot;
        terrain: None or dict(heights, dx, dy, x0, y0); lag: None = synchronous MPC, n = the asynchronous mode adopting every
        result n iterations after it was issued; measure_spread: keep a second simulator (and estimator) that repeats every
        free-run tick from inputs moved up by one ulp (tick_spread of tests/test_gpu_sim.py on the loop's own signals)."""
        self.cfg, self.k_mpc, self.lag = cfg, cfg["k_mpc"], lag
        self.n_steps = int(round(cfg["T_mpc"] / cfg["dt_mpc"]))
        self.joy = jn.JoystickNumpy(k_switch=profile[0], v_switch=profile[1], codes=codes, pushes=pushes)
        self.k_stop = -1
        mk_est = (lambda: ekn.Estimator(cfg["dt_wbc"], h_init, kalman=True)) if kalman else (lambda: en.Estimator(cfg["dt_wbc"], h_init))
        self.est = mk_est()
        self.glue = co.ControllerGlue(q_init, cfg["h_ref"], cfg["dt_wbc"])
        self.plan = oracle.Planner(dt_mpc=cfg["dt_mpc"], dt_wbc=cfg["dt_wbc"], T_gait=cfg["T_gait"], T_mpc=cfg["T_mpc"],
                                   N_gait=cfg["N_gait"], k_mpc=self.k_mpc, h_ref=cfg["h_ref"])
        self.mpc = oracle.MPC(cfg["dt_mpc"], self.n_steps, cfg["T_gait"], cfg["N_gait"])
        self.wbc = oracle.WbcController(cfg["dt_wbc"])
        first = np.zeros((24, self.n_steps))  # scripts/MPC_Wrapper.py:64-71
        first[2, 0] = cfg["h_ref"]
        first[12:, 0] = [0.0, 0.0, 8.0] * 4
        self.last_available, self.issued, self.not_first = first, [], False
        if terrain is None:
            mk_sim = lambda: sn.SimNumpy(q_init, dt=cfg["dt_wbc"])
        else:
            field = stn.Terrain(terrain["heights"], terrain["dx"], terrain["dy"], terrain.get("x0", 0.0), terrain.get("y0", 0.0))
            mk_sim = lambda: stn.SimTerrainNumpy(q_init, field, origin, dt=cfg["dt_wbc"])
        self.sim = mk_sim()
        self.flag = 0                      # the error flag the last controller stage left
        self.result = None
        self.spread = dict(sim=0.0, est=0.0) if measure_spread else None
        if measure_spread:
            self.sim_p = mk_sim()
        self.trace = []                    # one dict per tick: what the scenario assertions read

    # ------------------------------------------------------------------------------------------- stages
    def joystick_stage(self, k, flag_prev):
        """v_ref (6,), code, f_ext (6,) of tick k.  The latch closes on the first tick that SEES a flag: k_stop = that tick; the
        three outputs are zero from then on and the checker is not stepped any more (its filter state is frozen)."""
        if self.k_stop < 0 and flag_prev != 0:
            self.k_stop = k
        if self.k_stop >= 0:
            return np.zeros(6), 0, np.zeros(6)
        v, code = self.joy.update_v_ref(k)
        return np.array(v, dtype=np.float64), int(code), self.joy.apply_external_forces(k)

    def estimator_stage(self, sensors):
        """Estimator.run_filter on the gait and the foot goals the planners hold BEFORE this tick's step."""
        gait, goals = self.plan.gaits()[1], self.plan.feet()[0]
        moved = None
        if self.spread is not None:
            # the checker against itself on this tick: a copy of its state, every sensor input moved up by one ulp
            # (scripts/kalman_tolerance.py's variant (a)); the four outputs relative to max(1, |item|_inf)
            moved = copy.deepcopy(self.est)
            moved.run_filter(gait, goals, *[moved_by_one_ulp(sensors[n]) for n in SENSOR_KEYS])
        self.est.run_filter(gait, goals, *[sensors[n] for n in SENSOR_KEYS])
        if moved is not None:
            r = self.est
            for x, y in ((r.q_filt, moved.q_filt), (r.v_filt, moved.v_filt), (r.RPY, moved.RPY), (r.v_secu, moved.v_secu)):
                self.spread["est"] = max(self.spread["est"], rel(y, x))
        return dict(q_filt=self.est.q_filt.copy(), v_filt=self.est.v_filt.copy(), rpy=self.est.RPY.copy(), v_secu=self.est.v_secu.copy())

    def controller_stage(self, k, v_ref, code, est):
        """updateState -> planners -> MPC every k_mpc-th tick -> WBC targets -> WBC -> result + security_check.  Returns
        dict(result (5,12), flag, solve = (iterations, status) or None, ratios = the three tested quantities over their limits)."""
        g, plan = self.glue, self.plan
        oRh, oTh = g.update_state(v_ref, est["q_filt"], est["v_filt"], est["rpy"])
        plan.step(k, g.q[:7, 0], g.h_v[:6, 0], g.v_ref[:6, 0], int(code))
        xref, (fsteps, _, _), cgait = plan.xref(), plan.footsteps(), plan.gaits()[1]
        solve = None
        if k % self.k_mpc == 0:
            self.mpc.run(k, xref, fsteps)
            self.issued.append((k, self.mpc.get_latest_result().copy()))
            solve = (int(self.mpc.iter), int(self.mpc.status))
            if self.lag is not None and k > 2:  # MPC_Wrapper.solve's bookkeeping (:89-102): dead code in the synchronous mode
                shift_last_available(self.last_available, cgait, self.n_steps)
        if self.not_first:  # get_latest_result (:106-126): the first call returns the default without looking
            for k0, res in list(self.issued):
                if k >= k0 + (self.lag or 0):
                    self.last_available = res
                    self.issued = [p for p in self.issued if p[0] != k0]
        self.not_first = True
        pos, vel, acc, _, _ = plan.feet()
        xw, qw, bv = g.wbc_inputs(self.last_available, xref, oRh, oTh, pos, vel, acc)
        ratios = dict(q=float((np.abs(est["q_filt"][7:]) / g.q_security).max()), v=float(np.abs(est["v_secu"]).max() / 50.0), tau=0.0)
        if not g.error:  # scripts/Controller.py:273: the WBC block is skipped once an error has been raised
            self.wbc.compute(qw, bv, xw[12:], cgait[0, :], g.feet_p_cmd, g.feet_v_cmd, g.feet_a_cmd)
            ratios["tau"] = float(np.abs(self.wbc.tau_ff).max() / 8.0)
            out = g.result(self.wbc.tau_ff, self.wbc.qdes, self.wbc.vdes[:, 0], est["q_filt"], est["v_secu"])
        else:
            out = g.result(np.zeros(12), g.qdes, g.vdes[:, 0], est["q_filt"], est["v_secu"])
        self.flag = int(g.error_flag)
        return dict(result=np.stack(out), flag=self.flag, solve=solve, ratios=ratios, gait_row0=cgait[0].copy(), gait=cgait.copy())

    def simulator_stage(self, result, f_ext, state=None):
        """One tick under the Result (5,12) and the push; state: dict(q, v, prev_o_imuVel, tick, status) to start from, None = the
        checker's own."""
        if state is not None:
            self.sim.set_state(state["q"], state["v"], state["prev_o_imuVel"], state["tick"], state["status"])
        elif self.spread is not None:
            s, p = self.sim, self.sim_p
            qp = moved_by_one_ulp(s.q)
            qp[3:7] = s.q[3:7]  # (the quaternion stays a unit one)
            p.set_state(qp, moved_by_one_ulp(s.v), moved_by_one_ulp(s.prev), s.tick, s.status)
            p.out = s.out
        self.sim.step(*result, f_ext)
        if state is None and self.spread is not None:
            s, p = self.sim, self.sim_p
            p.step(*result, f_ext)
            for x, y in [(s.q, p.q), (s.v, p.v), (s.prev, p.prev)] + [(s.out[n], p.out[n]) for n in SIM_OUT_KEYS]:
                self.spread["sim"] = max(self.spread["sim"], rel(y, x))
        return self.sim

    # ------------------------------------------------------------------------------------------- one tick
    def tick(self, k, forced=None):
        """forced: None (free run) or dict(flag_prev, sensors, v_ref, code, f_ext, est, result, sim_state): the record of what each
        stage read on the device.  Returns dict(v_ref, code, f_ext, est, ctl, sim) with this chain's outputs."""
        f = forced or {}
        v_ref, code, f_ext = self.joystick_stage(k, f.get("flag_prev", self.flag))
        est = self.estimator_stage(f.get("sensors", self.sim.out))
        ctl = self.controller_stage(k, f.get("v_ref", v_ref), f.get("code", code), f.get("est", est))
        sim = self.simulator_stage(f.get("result", ctl["result"]), f.get("f_ext", f_ext), f.get("sim_state"))
        feet = int((sim.out["contact_forces"][:, 2] > 0).sum())
        self.trace.append(dict(k=k, flag=ctl["flag"], ratios=ctl["ratios"], gait_row0=ctl["gait_row0"], gait=ctl["gait"], feet=feet,
                               v_ref=v_ref, code=code, f_ext=f_ext, status=sim.status))
        return dict(v_ref=v_ref, code=code, f_ext=f_ext, est=est, ctl=ctl, sim=sim)
