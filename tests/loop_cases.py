"""The scenarios of the whole-loop tests (tests/test_loop_cpu.py free-runs the checkers on them, tests/test_gpu_loop.py records the
device loop on them and audits it): plain data and table builders, one joystick table set per robot.

Every velocity table is a two- or four-column profile of scripts/Joystick.py's handle_v_switch (zero at tick 0, the target held
after the last switch); a push is (start, duration, F, M) under joy::push_alpha's bell 16 x^2 (1 - x)^2, so F and M are its
PEAK, reached in the middle of the window.  The gait codes are src/Gait.cpp:197-219's: 1 pacing, 2 bounding, 3 trot, 4 static
(the only one that sets is_static_; 5, the walk, is this project's).  A new gait enters at the END of the current table, so it
reaches row 0 sixteen MPC steps (160 ticks) after the first roll that follows its code."""
import numpy as np

Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])  # scripts/main_solo12_control.py:120
H_INIT = 0.22294615
DEFAULT_CFG = dict(dt_wbc=0.002, dt_mpc=0.02, k_mpc=10, T_gait=0.32, T_mpc=0.32, N_gait=20, h_ref=0.2229)  # (test_gpu_controller.py's)
SECURITY_MARGIN = 1e-3  # ten times the 1e-4 the controller comparison allows: how far from its threshold a flag must rise

# row 0 of the gait table once the code's gait is the current one
ROW0_OF_CODE = {1: ((1, 0, 1, 0), (0, 1, 0, 1)), 2: ((1, 1, 0, 0), (0, 0, 1, 1)), 3: ((1, 0, 0, 1), (0, 1, 1, 0)), 4: ((1, 1, 1, 1),)}


def ramp(target, over, back=None):
    """(k_switch, v_switch): 0 -> target (vx, vy, wz) over `over` ticks; back=(k0, k1): held until k0, back to zero at k1."""
    vx, vy, wz = target
    v = np.array([vx, vy, 0.0, 0.0, 0.0, wz])
    if back is None:
        return np.array([0, over]), np.stack([np.zeros(6), v], axis=1)
    return np.array([0, over, back[0], back[1]]), np.stack([np.zeros(6), v, v, np.zeros(6)], axis=1)


def push(start, duration, F, M=(0.0, 0.0, 0.0)):
    return (int(start), int(duration), np.array(F, dtype=np.float64), np.array(M, dtype=np.float64))


# name -> dict(profile, codes, pushes, stops): stops = None for a robot meant to walk through the whole run, or the window
# (first tick, last tick) in which its error flag must rise
SCENARIOS = {
    "forward_yaw": dict(profile=ramp((0.3, 0.0, 0.4), 100), codes=[], pushes=[], stops=None),
    "pacing_at_60": dict(profile=ramp((0.2, 0.0, 0.0), 100), codes=[(60, 1)], pushes=[], stops=None),
    # the static gait at a tick that is no multiple of k_mpc; the robot is told to stand again before the four-stance rows come
    "static_at_47": dict(profile=ramp((0.15, 0.0, 0.0), 60, back=(120, 180)), codes=[(47, 4)], pushes=[], stops=None),
    "push_moderate": dict(profile=ramp((0.2, 0.0, 0.0), 100), codes=[], pushes=[push(100, 60, (0.0, 60.0, 0.0))], stops=None),
    # the second push is still scheduled when the latch closes: it must never arrive
    "push_strong": dict(profile=ramp((0.2, 0.0, 0.0), 100), codes=[],
                        pushes=[push(100, 40, (0.0, 400.0, 0.0)), push(200, 40, (0.0, 30.0, 0.0), (0.0, 0.0, 0.3))], stops=(100, 250)),
    "fast_ramp": dict(profile=ramp((1.5, 0.0, 2.0), 60), codes=[], pushes=[], stops=(100, 250)),
    "back_yaw_push": dict(profile=ramp((-0.2, 0.0, -0.3), 80), codes=[],
                          pushes=[push(120, 50, (6.0, -8.0, 4.0), (0.4, -0.3, 0.5))], stops=None),
    "stand_late_code": dict(profile=ramp((0.0, 0.0, 0.0), 10), codes=[(133, 2)], pushes=[], stops=None),
    # the short asynchronous run: everything earlier
    "pacing_at_23": dict(profile=ramp((0.2, 0.0, 0.0), 60), codes=[(23, 1)], pushes=[], stops=None),
    # the same tables on the rough field: the checkers' free run loses this robot to flag 2 (joint speed) when the pacing rows come
    "pacing_at_23_rough": dict(profile=ramp((0.2, 0.0, 0.0), 60), codes=[(23, 1)], pushes=[], stops=(100, 230)),
    "static_at_17": dict(profile=ramp((0.15, 0.0, 0.0), 40, back=(60, 100)), codes=[(17, 4)], pushes=[], stops=None),
    "push_moderate_early": dict(profile=ramp((0.2, 0.0, 0.0), 60), codes=[(35, 2)], pushes=[push(40, 50, (0.0, 60.0, 0.0))], stops=None),
    "push_strong_early": dict(profile=ramp((0.2, 0.0, 0.0), 60), codes=[],
                              pushes=[push(30, 40, (0.0, 400.0, 0.0)), push(85, 30, (0.0, 30.0, 0.0), (0.0, 0.0, 0.3))], stops=(30, 110)),
}

# variant -> the fleet.  rough_kalman: Simulator.reference_rough_ground() under every robot, looked up at an origin of its own,
# and the Kalman estimator; async_lag3: the asynchronous MPC adopted three iterations late, on the plane.
VARIANTS = {
    "plane": dict(T=320, kalman=False, rough=False, lag=None, feet=(0, 1, 2, 3, 4),
                  robots=("forward_yaw", "pacing_at_60", "static_at_47", "push_moderate", "push_strong", "fast_ramp", "back_yaw_push",
                          "stand_late_code")),
    "rough_kalman": dict(T=240, kalman=True, rough=True, lag=None, feet=(0, 1, 2, 3, 4),
                         robots=("forward_yaw", "pacing_at_23_rough", "static_at_17", "push_moderate", "push_strong", "back_yaw_push")),
    # (120 ticks: no code's gait reaches row 0, so the trot's two feet and the pushed robots' 0, 1 and 3 are what is seen)
    "async_lag3": dict(T=120, kalman=False, rough=False, lag=3, feet=(0, 1, 2, 3),
                       robots=("forward_yaw", "pacing_at_23", "static_at_17", "push_moderate_early", "push_strong_early")),
}

# As measured by tests/test_loop_cpu.py's free run of the checkers (scripts/loop_tolerance.py prints them), three digits:
#   sim: the simulator checker against itself, every tick of every robot once more from the state moved up by one ulp, every state
#        item and output relative to max(1, |item|_inf) (tick_spread of tests/test_gpu_sim.py on the loop's own states and commands)
#   est: the estimator checker against itself, every sensor input of the tick moved up by one ulp, the four outputs in the same measure
#   min_abs_d: the smallest |d| over every sub-step of every robot, the moved copies included
LOOP_TICK_SPREAD = {
    "plane": dict(sim=1.46e-10, est=5.48e-16, min_abs_d=1.04e-07),
    "rough_kalman": dict(sim=2.24e-11, est=4.81e-16, min_abs_d=8.02e-07),
    "async_lag3": dict(sim=1.49e-11, est=4.18e-16, min_abs_d=1.99e-06),
}


def origins(n):
    """(n,2): every robot of the rough variant on a patch of its own, well inside the 25.6 m field."""
    return np.stack([np.array([1.7 * b - 4.0, 3.0 - 1.3 * b]) for b in range(n)])


def fleet(variant):
    """dict(T, B, kalman, rough, lag, names, profiles, codes, pushes, stops) of a variant, in the layout Joystick_batch takes."""
    v = VARIANTS[variant]
    sc = [SCENARIOS[n] for n in v["robots"]]
    return dict(T=v["T"], B=len(sc), feet=v["feet"], kalman=v["kalman"], rough=v["rough"], lag=v["lag"], names=v["robots"],
                profiles=[s["profile"] for s in sc], codes=[list(s["codes"]) for s in sc], pushes=[list(s["pushes"]) for s in sc],
                stops=[s["stops"] for s in sc])


def chains(variant, measure_spread=False):
    """One loop_chain.LoopChain per robot of the variant."""
    import loop_chain

    f = fleet(variant)
    terrain = None
    if f["rough"]:
        from Simulator import reference_rough_ground

        terrain = reference_rough_ground()
    org = origins(f["B"])
    return [loop_chain.LoopChain(DEFAULT_CFG, Q_INIT, H_INIT, f["profiles"][b], f["codes"][b], f["pushes"][b], kalman=f["kalman"],
                                 terrain=terrain, origin=tuple(org[b]), lag=f["lag"], measure_spread=measure_spread)
            for b in range(f["B"])]


def free_run(variant, measure_spread=False):
    """The chained checkers as a closed loop for the variant's T ticks; returns the chains (their .trace, .spread, .k_stop)."""
    cs = chains(variant, measure_spread)
    for k in range(fleet(variant)["T"]):
        for c in cs:
            c.tick(k)
    return cs


# ---------------------------------------------------------------------------------------------------- what a run must show
def flag_tick(flags):
    """First tick with a nonzero flag, or -1."""
    nz = np.flatnonzero(np.asarray(flags) != 0)
    return int(nz[0]) if nz.size else -1


def check_scenario(variant, flags, k_stop, v_ref, code, f_ext, gait_row0, feet, status):
    """The assertions that do not depend on the exact trajectory, on a record of the loop (the checkers' free run or the device's):
    flags (T,B), k_stop (B,), v_ref (T,B,6), code (T,B), f_ext (T,B,6), gait_row0 (T,B,4), feet (T,B) feet in contact, status (T,B)."""
    f = fleet(variant)
    T, B = f["T"], f["B"]
    assert np.shape(flags) == (T, B) and np.shape(gait_row0) == (T, B, 4)
    for b in range(B):
        name, kf = f["names"][b], flag_tick(flags[:, b])
        if f["stops"][b] is None:
            assert kf < 0 and k_stop[b] == -1 and not np.any(status[:, b]), (name, kf, k_stop[b])
        else:
            lo, hi = f["stops"][b]
            assert lo <= kf <= hi, (name, kf)
            assert np.all(flags[kf:, b] == flags[kf, b]), name            # sticky
            assert k_stop[b] == kf + 1, (name, kf, k_stop[b])              # the latch closes one tick after the flag
            assert not v_ref[kf + 1:, b].any() and not code[kf + 1:, b].any() and not f_ext[kf + 1:, b].any(), name
            assert v_ref[kf, b].any(), name                                 # ... and not before
        for k_code, c in f["codes"][b]:
            assert code[k_code, b] == c or 0 <= k_stop[b] <= k_code, (name, k_code)
            first_roll = -(-k_code // 10) * 10
            if first_roll + 160 < T:  # the code's gait is row 0 before the end of the run
                rows = {tuple(int(x) for x in r) for r in gait_row0[first_roll + 160:, b]}
                assert rows & set(ROW0_OF_CODE[c]), (name, k_code, rows)
                if c == 4:
                    assert rows == {(1, 1, 1, 1)}, (name, rows)
    seen = sorted(set(int(x) for x in np.unique(feet)))
    assert set(f["feet"]) <= set(seen), (variant, seen)
    return seen


FLAG_OF = {1: "q", 2: "v", 3: "tau"}  # security_check (scripts/Controller.py:341-355): the later comparison overwrites the earlier


def check_margins(name, flags, ratios):
    """ratios: per tick dict(q, v, tau) = the tested quantity over its limit (|q| / q_security, |v_secu| / 50, |tau_ff| / 8).  Every
    tick before the flag keeps all three SECURITY_MARGIN inside; on the raising tick the flag's own quantity is that far outside
    and the comparisons that would have overwritten it that far inside.  Returns (tick, flag, ratio before, ratio at the flag)."""
    kf = flag_tick(flags)
    for k in range(len(flags) if kf < 0 else kf):
        assert max(ratios[k].values()) <= 1.0 - SECURITY_MARGIN, (name, k, ratios[k])
    if kf < 0:
        return None
    flag = int(flags[kf])
    assert ratios[kf][FLAG_OF[flag]] >= 1.0 + SECURITY_MARGIN, (name, kf, flag, ratios[kf])
    for later in range(flag + 1, 4):
        assert ratios[kf][FLAG_OF[later]] <= 1.0 - SECURITY_MARGIN, (name, kf, flag, ratios[kf])
    return kf, flag, ratios[kf - 1][FLAG_OF[flag]], ratios[kf][FLAG_OF[flag]]


def arrays(cs):
    """The arguments of check_scenario from the chains of a run (free or forced)."""
    col = lambda key, dtype=None: np.array([[t[key] for t in c.trace] for c in cs], dtype=dtype).swapaxes(0, 1)
    return dict(flags=col("flag", np.int64), k_stop=np.array([c.k_stop for c in cs]), v_ref=col("v_ref"), code=col("code", np.int64),
                f_ext=col("f_ext"), gait_row0=col("gait_row0"), feet=col("feet", np.int64), status=col("status", np.int64))


def measured(cs):
    """dict(sim, est, min_abs_d) of a free run with measure_spread=True: the figures LOOP_TICK_SPREAD records."""
    return dict(sim=max(c.spread["sim"] for c in cs), est=max(c.spread["est"] for c in cs),
                min_abs_d=min(min(c.sim.min_abs_d, c.sim_p.min_abs_d) for c in cs))
