"""The planner tests' configurations off the defaults, their input sequences, the oracle's run over them (computed once and
shared) and the tolerances: tests/test_gpu_planner_limits.py, tests/test_gpu_planner_params.py, tests/test_planner_cases_cpu.py
and scripts/planner_tolerance.py all read this module.  No GPU is touched here.

Tolerances.  Gait matrices, contacts and flags compare exactly.  For a floating-point output the figure compared is
    err = max |got - ref| / max(1, max |ref|)          over the output's block of one robot at one iteration,
and its bound is 100 x the oracle's own spread: the largest err between the oracle's run and its run with one of the inputs
(q7, hv, vref) moved by one ulp (every non-zero element; exact zeros stay, they select branches), over the same sequence.  The
spreads are measured by spread() -- scripts/planner_tolerance.py prints them -- and recorded in SPREAD below;
tests/test_planner_cases_cpu.py holds the record against the measurement.  The swing polynomial divides by powers of the time
left in the swing, so a shorter lock_time raises the spread of the foot trajectories: every case has its own figures."""
import numpy as np

DEFAULT_SHOULDERS = np.array([[0.1946, 0.1946, -0.1946, -0.1946], [0.14695, -0.14695, 0.14695, -0.14695], [0.0, 0.0, 0.0, 0.0]])
# four different x, four different y (and four different z: the reference carries the row along, FootstepPlanner.cpp:45-47)
TUNED_SHOULDERS = np.array([[0.2110, 0.1830, -0.1720, -0.2030], [0.1610, -0.1330, 0.1520, -0.1240], [0.004, -0.003, 0.002, 0.001]])
TARGET_OFFSETS = np.array([[0.011, -0.007, 0.013, 0.005], [-0.009, 0.012, 0.006, -0.014], [0.002, 0.001, -0.001, 0.003]])
FOOT_OFFSETS = np.array([[-0.015, 0.009, -0.004, 0.017], [0.008, 0.016, -0.012, -0.006], [0.004, 0.0, 0.006, 0.002]])

FLOAT_OUTPUTS = ("xref", "fsteps", "target", "pos", "vel", "acc")
STATE_EVERY = 23  # iterations between two comparisons of the planner's state items

_T4 = dict(k_mpc=4, dt_wbc=0.005)  # k_mpc * dt_wbc = dt_mpc, as everywhere in the reference's configurations
_BASE = dict(N=16, N_gait=20, T_gait=0.32, dt_mpc=0.02, dt_wbc=0.002, k_mpc=10, geometry={}, B=9)


def _case(**kw):
    return dict(_BASE, **kw)


CASES = {
    # ---- the table limits (default geometry)
    "full20": _case(T_gait=0.40, seq="limits"),                             # 20 rows per period = N_gait: the full table
    "walk_fills": _case(T_gait=0.36, seq="limits"),                         # 18 rows, the walk writes 4 * 5 = 20
    "odd": _case(N=12, T_gait=0.30, seq="limits"),                          # 15 rows, the trot writes 2 * 8 = 16
    "wide": _case(N=32, N_gait=63, T_gait=1.22, seq="limits", **_T4),       # 61 rows, a 62-row trot, a 33-row past gait
    "tight": _case(N=8, N_gait=9, T_gait=0.16, seq="limits"),               # 8 rows in 9, n_steps + 1 = N_gait
    # ---- off the 0.02 s MPC step (k_mpc * dt_wbc = dt_mpc; neither T_gait nor dt_mpc is a binary fraction: lround sees quotients computed from rounded operands)
    "step10": _case(N=16, N_gait=24, T_gait=0.20, dt_mpc=0.010, k_mpc=5, seq="limits"),                 # 20 rows per period
    "step40": _case(N=8, N_gait=20, T_gait=0.48, dt_mpc=0.040, k_mpc=20, seq="limits"),                 # 12 rows
    "step16": _case(N=20, N_gait=24, T_gait=0.32, dt_mpc=0.016, k_mpc=8, seq="limits"),                 # 20 rows
    "step24": _case(N=12, N_gait=20, T_gait=0.36, dt_mpc=0.024, k_mpc=12, seq="limits"),                # 15 rows, trot and walk write 16
    "step25": _case(N=12, N_gait=20, T_gait=0.40, dt_mpc=0.025, k_mpc=5, dt_wbc=0.005, seq="limits"),   # 16 rows
    # ---- off the default geometry
    "TUNED": _case(seq="tuned", iters=400, **_T4,
                   geometry=dict(shoulders=TUNED_SHOULDERS, h_ref=0.24, max_height=0.08, lock_time=0.04,
                                 init_target=TUNED_SHOULDERS + TARGET_OFFSETS, init_foot_pos=TUNED_SHOULDERS + FOOT_OFFSETS)),
    "base": _case(seq="alone", iters=300, **_T4),
    "shoulders": _case(seq="alone", iters=300, **_T4, geometry=dict(shoulders=TUNED_SHOULDERS)),
    "h_ref": _case(seq="alone", iters=300, **_T4, geometry=dict(h_ref=0.24)),
    "max_height": _case(seq="alone", iters=300, **_T4, geometry=dict(max_height=0.08)),
    "lock_time": _case(seq="alone", iters=300, **_T4, geometry=dict(lock_time=0.04)),
    "init_target": _case(seq="alone", iters=300, **_T4, geometry=dict(init_target=DEFAULT_SHOULDERS + TARGET_OFFSETS)),
    "init_foot_pos": _case(seq="alone", iters=300, **_T4, geometry=dict(init_foot_pos=DEFAULT_SHOULDERS + FOOT_OFFSETS)),
    # a lock time longer than any swing: the x / y coefficients are never updated and stay zero, as in the reference
    "lock_long": _case(seq="alone", iters=300, **_T4, geometry=dict(lock_time=0.5)),
    # ---- held against the second implementation only (tests/test_planner_second_impl.py, CPU)
    "default": _case(seq="plain", iters=300, B=3),
    "alt": _case(N=12, N_gait=26, T_gait=0.40, dt_wbc=0.001, k_mpc=20, geometry=dict(h_ref=0.21), seq="plain", iters=500, B=3),
    "short_period": _case(N=4, N_gait=24, T_gait=0.08, seq="plain", iters=300, B=3),
    "wild": _case(seq="wild", iters=400, B=4),  # the inputs of test_planner_on_wild_inputs_matches_oracle
}
ALONE = ("shoulders", "h_ref", "max_height", "lock_time", "init_target", "init_foot_pos")
LIMITS = ("full20", "walk_fills", "odd", "wide", "tight")
STEPS = ("step10", "step40", "step16", "step24", "step25")


def lround(x):
    f = np.floor(abs(x))
    return int(f + (1 if abs(x) - f >= 0.5 else 0))


def rows_needed(case):
    c = CASES[case]
    r = c["T_gait"] / c["dt_mpc"]
    return max(2 * lround(0.5 * c["T_gait"] / c["dt_mpc"]), 4 * lround(0.25 * c["T_gait"] / c["dt_mpc"]), lround(r))


def handle_kwargs(case):
    c = CASES[case]
    return dict(n_steps=c["N"], N_gait=c["N_gait"], dt_mpc=c["dt_mpc"], T_gait=c["T_gait"], dt_wbc=c["dt_wbc"])


def planner_init_kwargs(case):
    c = CASES[case]
    return dict(k_mpc=c["k_mpc"], **c["geometry"])


def oracle_planner(oracle_mod, case):
    c = CASES[case]
    g = dict(c["geometry"])
    return oracle_mod.Planner(c["dt_mpc"], c["dt_wbc"], c["T_gait"], c["N"] * c["dt_mpc"], c["N_gait"], c["k_mpc"],
                              g.pop("h_ref", 0.2229), g.pop("shoulders", None), g.pop("max_height", 0.05), g.pop("lock_time", 0.07),
                              g.pop("init_target", None), g.pop("init_foot_pos", None))


def code_schedule(case):
    """{iteration: {robot: code}}: every robot changes gait at its own times, on iterations that roll the gait and on ones
    that do not, through static (4) and away from it again, and the run goes on for two of the longest periods after the last."""
    c = CASES[case]
    B, period = c["B"], rows_needed(case) * c["k_mpc"]
    events = {}
    if c["seq"] == "limits":
        # (a new gait enters at the END of the current horizon: the spacing lets some changes arrive during a transition)
        starts = (period // 7 + 3, period // 2 + 11, period + 17, period + period // 2 + 29)
        for b in range(B):
            codes = (1 + (b % 5), 4, (1 + (b + 1) % 3) if b % 2 else 5, (3, 5, 1, 2)[b % 4])  # (away from static: never 4 again)
            for i, (s, code) in enumerate(zip(starts, codes)):
                events.setdefault(s + (3 + 2 * i) * b, {})[b] = code
        last = max(events)
        iters = last + 2 * period + c["k_mpc"]
    else:
        iters = c["iters"]
        for b in range(B):
            events.setdefault(41 + 3 * b, {})[b] = 1 + (b % 5)
            if c["seq"] == "tuned" or b % 2:
                events.setdefault(iters // 2 + 5 * b + 2, {})[b] = 1 + ((b + 2) % 5)
    return events, iters


_seq_cache, _run_cache = {}, {}


def sequence(case):
    """The inputs of every iteration: q7 (K, B, 7), hv (K, B, 6), vref (K, B, 6), code (K, B) int32.  The base moves and turns,
    the measured velocity is the reference plus noise (so the footstep targets move inside a swing), the reference velocity is
    re-drawn twice, and the yaw rate is exactly 0 on robot 0 (and, after the first re-draw, on robot 1)."""
    c = CASES[case]
    key = (c["seq"], case if c["seq"] in ("limits", "plain", "wild") else "")
    if key in _seq_cache:
        return _seq_cache[key]
    events, K = code_schedule(case)
    B = c["B"]
    rng = np.random.default_rng([2027, sum(map(ord, c["seq"])), len(key[1]), K])
    q7, hv, vref, code = np.zeros((K, B, 7)), np.zeros((K, B, 6)), np.zeros((K, B, 6)), np.zeros((K, B), np.int32)
    v = rng.uniform(-0.5, 0.5, (B, 6)) * np.array([2, 1, 0, 0, 0, 1.4])
    v[0, 5] = 0.0
    for k in range(K):
        if k in (K // 3, 2 * K // 3):
            v = rng.uniform(-0.5, 0.5, (B, 6)) * np.array([2, 1, 0, 0, 0, 1.4])
            v[1 if k == K // 3 else 0, 5] = 0.0
        q7[k, :, :2] = rng.uniform(-1, 1, (B, 2))
        q7[k, :, 2] = 0.2229 + rng.uniform(-0.01, 0.01, B)
        quat = np.stack([rng.uniform(-0.03, 0.03, B), rng.uniform(-0.03, 0.03, B), rng.uniform(-0.2, 0.2, B), np.ones(B)], 1)
        q7[k, :, 3:] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        vref[k] = v
        hv[k] = v + rng.uniform(-0.1, 0.1, (B, 6))
        for b, cd in events.get(k, {}).items():
            code[k, b] = cd
    if c["seq"] == "wild":
        q7, hv, vref, code = _wild(rng, K, B)
    _seq_cache[key] = dict(q7=q7, hv=hv, vref=vref, code=code)
    return _seq_cache[key]


def _wild(rng, K, B):
    """Far outside the joystick's range: any yaw, roll / pitch up to 0.5 rad, positions metres away, reference velocities up to
    3 m/s and 3 rad/s re-drawn every 40 iterations (the Raibert terms run into their clamp), measured velocities a metre per
    second off, yaw rate exactly 0 on robot 0, codes in bursts (consecutive iterations, during a transition, code 0)."""
    q7, hv, vref, code = np.zeros((K, B, 7)), np.zeros((K, B, 6)), np.zeros((K, B, 6)), np.zeros((K, B), np.int32)
    burst = np.zeros(B, np.int64)
    for k in range(K):
        if k % 40 == 0:
            v = rng.uniform(-1, 1, (B, 6)) * np.array([3.0, 1.5, 0, 0, 0, 3.0])
            v[0, 5] = 0.0
            v[B - 1, :2] = 0.0
        q7[k, :, :2], q7[k, :, 2] = rng.uniform(-5, 5, (B, 2)), 0.2229 + rng.uniform(-0.05, 0.05, B)
        yaw, pitch, roll = rng.uniform(-np.pi, np.pi, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B)
        cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
        q7[k, :, 3:] = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
        vref[k] = v
        hv[k] = v + rng.uniform(-1.0, 1.0, (B, 6)) * np.array([1, 1, 0.3, 0.5, 0.5, 1])
        for b in range(B):
            if burst[b] > 0:
                code[k, b], burst[b] = rng.integers(0, 6), burst[b] - 1
            elif rng.random() < 0.03:
                code[k, b], burst[b] = rng.integers(1, 6), rng.integers(0, 4)
    return q7, hv, vref, code


def oracle_run(oracle_mod, case, moved=None):
    """The oracle over the case's sequence: every output of every iteration stacked over (K, B), the flags (newPhase, is_static,
    remainingTime, number of swing feet) likewise, and every STATE_EVERY-th iteration the past / desired gait and the trajectory
    generator's target.  moved: one of "q7", "hv", "vref" -- that input one ulp up (not cached)."""
    if moved is None and case in _run_cache:
        return _run_cache[case]
    c, seq = CASES[case], sequence(case)
    K, B = seq["code"].shape
    inp = {k: v for k, v in seq.items()}
    if moved is not None:
        x = seq[moved]
        inp[moved] = np.where(x != 0.0, np.nextafter(x, np.inf), x)
    refs = [oracle_planner(oracle_mod, case) for _ in range(B)]
    Ng, N = c["N_gait"], c["N"]
    out = dict(gait=np.zeros((K, B, Ng, 4)), xref=np.zeros((K, B, 12, N + 1)), fsteps=np.zeros((K, B, Ng, 12)), target=np.zeros((K, B, 3, 4)),
               pos=np.zeros((K, B, 3, 4)), vel=np.zeros((K, B, 3, 4)), acc=np.zeros((K, B, 3, 4)), flags=np.zeros((K, B, 4)), tsw=np.zeros((K, B, 4)), state={})
    for k in range(K):
        for b, r in enumerate(refs):
            r.step(k, inp["q7"][k, b], inp["hv"][k, b], inp["vref"][k, b], int(inp["code"][k, b]))
            out["gait"][k, b] = r.gaits()[1]
            out["xref"][k, b] = r.xref()
            out["fsteps"][k, b], _, out["target"][k, b] = r.footsteps()
            out["pos"][k, b], out["vel"][k, b], out["acc"][k, b], _, out["tsw"][k, b] = r.feet()
            f = r.flags()
            out["flags"][k, b] = [f["new_phase"], f["is_static"], f["remaining_time"], f["n_swing"]]
        if k % STATE_EVERY == STATE_EVERY - 1 or k == K - 1:
            out["state"][k] = [(r.gaits()[0], r.gaits()[2], r.ft_target()) for r in refs]
    if moved is None:
        _run_cache[case] = out
    return out


def err(got, ref):
    """max |got - ref| / max(1, max |ref|) per robot over the trailing axes of (..., B, *block); returns the largest."""
    got, ref = np.asarray(got), np.asarray(ref)
    lead = ref.ndim - 2  # (every output's block has two axes)
    g, r = got.reshape(got.shape[:lead] + (-1,)), ref.reshape(ref.shape[:lead] + (-1,))
    return float((np.abs(g - r).max(-1) / np.maximum(1.0, np.abs(r).max(-1))).max())


def spread(oracle_mod, case):
    """{output: the largest err between the oracle's run and its runs with q7, hv, vref moved by one ulp}."""
    base = oracle_run(oracle_mod, case)
    s = dict.fromkeys(FLOAT_OUTPUTS, 0.0)
    for moved in ("q7", "hv", "vref"):
        run = oracle_run(oracle_mod, case, moved)
        assert np.array_equal(run["gait"], base["gait"]) and np.array_equal(run["flags"], base["flags"])
        for name in FLOAT_OUTPUTS:
            s[name] = max(s[name], err(run[name], base[name]))
    return s


def effect(oracle_mod, case, other="base"):
    """{output: the largest err between the oracle's runs of two cases that share a sequence}, "ft_target" included."""
    a, b = oracle_run(oracle_mod, case), oracle_run(oracle_mod, other)
    e = {name: err(a[name], b[name]) for name in FLOAT_OUTPUTS}
    e["ft_target"] = max(err(np.stack([x[2] for x in a["state"][k]]), np.stack([x[2] for x in b["state"][k]])) for k in a["state"])
    return e


# ---- the record: spread() of every case as scripts/planner_tolerance.py printed it (bound = 100 x)
SPREAD = {
    "full20": dict(xref=2.50e-16, fsteps=3.05e-16, target=4.36e-16, pos=4.48e-10, vel=2.04e-09, acc=4.28e-08),  # 811 iterations x 9 robots
    "walk_fills": dict(xref=3.61e-16, fsteps=1.61e-15, target=1.69e-15, pos=1.13e-10, vel=2.21e-10, acc=2.21e-09),  # 811 iterations x 9 robots
    "odd": dict(xref=2.22e-16, fsteps=2.50e-16, target=4.18e-16, pos=3.38e-11, vel=3.96e-10, acc=1.30e-08),  # 671 iterations x 9 robots
    "wide": dict(xref=3.05e-16, fsteps=4.72e-16, target=4.44e-16, pos=6.93e-08, vel=1.50e-07, acc=4.11e-07),  # 973 iterations x 9 robots
    "tight": dict(xref=2.22e-16, fsteps=1.11e-15, target=1.11e-15, pos=1.25e-12, vel=2.18e-11, acc=2.62e-10),  # 391 iterations x 9 robots
    "step10": dict(xref=2.22e-16, fsteps=1.67e-16, target=2.22e-16, pos=2.06e-12, vel=2.03e-11, acc=2.91e-10),  # 456 iterations x 9 robots
    "step40": dict(xref=2.22e-16, fsteps=5.00e-16, target=4.29e-16, pos=1.24e-09, vel=2.51e-09, acc=8.38e-09),  # 961 iterations x 9 robots
    "step16": dict(xref=4.44e-16, fsteps=1.17e-15, target=1.22e-15, pos=2.23e-11, vel=2.47e-10, acc=5.82e-09),  # 669 iterations x 9 robots
    "step24": dict(xref=1.11e-16, fsteps=2.00e-15, target=2.11e-15, pos=2.37e-10, vel=1.51e-09, acc=1.91e-08),  # 785 iterations x 9 robots
    "step25": dict(xref=2.22e-16, fsteps=5.00e-16, target=5.36e-16, pos=9.07e-10, vel=6.96e-09, acc=5.36e-08),  # 386 iterations x 9 robots
    "TUNED": dict(xref=3.13e-16, fsteps=1.22e-15, target=1.22e-15, pos=2.88e-09, vel=3.47e-08, acc=1.62e-07),  # 400 iterations x 9 robots
    "base": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=6.66e-11, vel=4.84e-10, acc=2.97e-09),  # 300 iterations x 9 robots
    "shoulders": dict(xref=2.22e-16, fsteps=5.00e-16, target=4.44e-16, pos=3.93e-11, vel=3.49e-10, acc=2.56e-09),  # 300 iterations x 9 robots
    "h_ref": dict(xref=2.22e-16, fsteps=5.55e-16, target=5.00e-16, pos=3.90e-11, vel=3.49e-10, acc=3.03e-09),  # 300 iterations x 9 robots
    "max_height": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=6.66e-11, vel=4.84e-10, acc=2.97e-09),  # 300 iterations x 9 robots
    "lock_time": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=3.46e-09, vel=3.41e-08, acc=2.96e-07),  # 300 iterations x 9 robots
    "init_target": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=6.66e-11, vel=4.84e-10, acc=2.97e-09),  # 300 iterations x 9 robots
    "init_foot_pos": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=7.92e-11, vel=6.48e-10, acc=3.96e-09),  # 300 iterations x 9 robots
    "default": dict(xref=2.22e-16, fsteps=5.55e-16, target=3.33e-16, pos=2.55e-11, vel=2.26e-10, acc=1.51e-09),  # 300 iterations x 3 robots
    "alt": dict(xref=2.22e-16, fsteps=1.94e-16, target=2.22e-16, pos=3.82e-11, vel=1.32e-10, acc=1.51e-09),  # 500 iterations x 3 robots
    # (0.04 s swings, shorter than the lock time: as lock_long below)
    "short_period": dict(xref=1.11e-16, fsteps=5.55e-17, target=2.22e-16, pos=0.00e+00, vel=0.00e+00, acc=0.00e+00),  # 300 iterations x 3 robots
    "wild": dict(xref=3.57e-16, fsteps=7.17e-16, target=4.44e-16, pos=1.38e-10, vel=1.89e-10, acc=2.79e-09),  # 400 iterations x 4 robots
    # (no input reaches the foot trajectories here -- x / y stay exactly zero, z depends on the gait alone: see z_bound)
    "lock_long": dict(xref=2.22e-16, fsteps=5.55e-16, target=4.44e-16, pos=0.00e+00, vel=0.00e+00, acc=0.00e+00),  # 300 iterations x 9 robots
}


def bound(case, name):
    return 100.0 * SPREAD[case]["target" if name == "ft_target" else name]


def z_bound(oracle_mod, case):
    """(K, B, 3) bounds on |device - oracle| of the z row of foot position / velocity / acceleration, from the number format alone
    (used where no input reaches the trajectories, so that the spread above is zero).  With e = t + dt <= d the reference's
    z(e) = Az3 e^3 + Az2 e^4 + Az1 e^5 + Az0 e^6, Az = 64 h (d^3, -3 d^2, 3 d, -1) / d^6 (FootTrajectoryGenerator.cpp:96-105), is a sum
    of four terms of magnitude at most 64 h (1, 3, 3, 1); its derivatives multiply them by (3, 4, 5, 6) / d and (6, 12, 20, 30) / d^2.
    Each term costs either side at most ten roundings (pow to under an ulp there, repeated multiplication here, the division, the
    products, the sum), so the two differ by at most 2 * 10 * eps * (the sum of the magnitudes): 512 h, 2304 h / d, 8448 h / d^2.
    d is the shortest swing any foot of the robot has had so far (a stance foot keeps the values of its last swing)."""
    run = oracle_run(oracle_mod, case)
    h = CASES[case]["geometry"].get("max_height", 0.05)
    d = np.where(run["tsw"] > 0.0, run["tsw"], np.inf).min(-1)
    d = np.minimum.accumulate(d, axis=0)
    eps20 = 20 * np.finfo(np.float64).eps
    return np.stack([np.full_like(d, eps20 * 512 * h), eps20 * 2304 * h / d, eps20 * 8448 * h / d ** 2], -1)
