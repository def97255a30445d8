"""GPU parity tests of the Kalman variant of the batched state estimator (estimator_kernel<true> and csrc/kalman_filter.h
through the C ABI and Controller_batch.compute_sensors) against the numpy checker tests/estimator_kalman_numpy.py, which keeps the
reference's dense form (18 x 18 P, np.linalg.inv), one object per robot.

Tolerances.  What the Kalman filter produces (q_filt, v_filt, X, P) is held to KALMAN_BOUND, in the measure of
scripts/kalman_tolerance.py: |got - ref| / max(1, |ref|) per entry, P scaled by its own largest entry.  The bound is 100 x the
largest difference that script finds, on the input sequences of THIS file (sequences() below), between the dense checker and
itself with (a) every sensor input moved by one ulp, (b) solve instead of inv, (c) the per-axis, one-measurement-at-a-time
arrangement the kernel uses.  What the two filters share (RPY, v_secu, Z -- kinematics and a rotation, like FK_xyz -- and the
state items) keeps the tolerance of tests/test_gpu_estimator.py: rtol 1e-9, atol 1e-11, integers exact.  No robot is excused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])  # scripts/main_solo12_control.py:120
H_INIT = 0.22294615
DT = 0.002
N_GAIT = 20
RTOL, ATOL = 1e-9, 1e-11
# scripts/kalman_tolerance.py: (a) 4.2e-15, (b) 2.1e-13, (c) 4.3e-13 on sequences() -> 100 x 4.3e-13.  The sequences at the other
# time step and gait table length (alt_trot_b17, alt_planner) give 1.99e-13 and 1.26e-13 at the most: below, so the constant stays.
KALMAN_BOUND = 4.3e-11
EXACT = ("k_since_contact", "close_from_contact", "k_log")
SENSOR_KEYS = ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")
IDENT = np.array([0.0, 0.0, 0.0, 1.0])
TUNED = dict(sigma_kin=0.07, sigma_h=0.6, sigma_a=0.25, sigma_dp=0.04, gamma=12.0)  # all five away from the reference's values
CORNERS = ("all_stance", "all_swing", "one_foot", "switch_on_tick_20", "attitude", "perfect")


# ------------------------------------------------------------------------------------------------ input sequences (no GPU)
def trot_tables(synth_mod, B, k, n_gait=N_GAIT, k_mpc=10, full=(), still=()):
    """Gait matrices (B, n_gait, 4) of tick k: a 16-row trot period that advances one row every k_mpc ticks, robot b two
    rows ahead of robot b - 1; rows 16.. are zero rows, as in the planners' matrices.  The robots of `full` have the period
    repeated through all n_gait rows (no zero row); those of `still` n_gait rows equal to their row 0 -- one stance pair for
    good, so that the scan for the first row that differs from row 0 ends at n_gait."""
    g = np.zeros((B, n_gait, 4))
    period = synth_mod.gait_pattern("trot", 16)
    for b in range(B):
        rolled = np.roll(period, -(k // k_mpc + 2 * b), axis=0)
        g[b, :16] = rolled
        if b in full:
            g[b] = rolled[np.arange(n_gait) % 16]
        if b in still:
            g[b] = period[(2 * b) % 16]
    return g


def _plain(B, rng):
    return dict(lin_acc=rng.uniform(-0.5, 0.5, (B, 3)), ang_vel=rng.uniform(-0.3, 0.3, (B, 3)), quat=np.tile(IDENT, (B, 1)),
                q_mes=Q_INIT + rng.uniform(-0.05, 0.05, (B, 12)), v_mes=rng.uniform(-1.0, 1.0, (B, 12)))


def _table(row0, B):
    g = np.zeros((B, N_GAIT, 4))
    g[:, :8] = np.asarray(row0, dtype=np.float64).reshape(-1, 1, 4)
    g[:, 8:16] = [0, 1, 1, 0]
    return g


def _yaw_quat(a):
    return np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])


def trot_sequence(synth_mod, B, ticks, seed, dt=DT, **tables):
    sen = synth_mod.SyntheticSensors(B, seed, dt)
    goals = np.random.default_rng(seed).uniform(-0.2, 0.2, (B, 3, 4))
    return [dict(sensors=sen.step(k), gait=trot_tables(synth_mod, B, k, **tables), goals=goals) for k in range(ticks)]


# the other configuration (tests/test_gpu_controller.py's ALT_CFG): the tick halved, gait matrices of 26 rows
ALT_DT, ALT_N_GAIT, ALT_K_MPC = 0.001, 26, 20
ALT_HANDLE = dict(n_steps=12, N_gait=ALT_N_GAIT, dt_mpc=0.02, T_gait=0.40, dt_wbc=ALT_DT)
ALT_PLANNER = dict(dt_mpc=0.02, dt_wbc=ALT_DT, T_gait=0.40, T_mpc=0.24, N_gait=ALT_N_GAIT, k_mpc=ALT_K_MPC, h_ref=0.21)
ALT_OPTIONS = dict(dt=ALT_DT, handle=ALT_HANDLE, planner_init=dict(k_mpc=ALT_K_MPC, h_ref=0.21))  # (sequences()' options)
ALT_FULL, ALT_STILL = (2, 9), (5, 16)  # robots whose 26 rows hold no zero row / are all their row 0 (block 1's only quad among them)


def alt_trot_sequence(synth_mod, B=17, ticks=120, seed=17):
    return trot_sequence(synth_mod, B, ticks, seed, ALT_DT, n_gait=ALT_N_GAIT, k_mpc=ALT_K_MPC, full=ALT_FULL, still=ALT_STILL)


def planner_sequence(oracle_mod, synth_mod, B=5, ticks=60, seed=8, **planner):
    """Gait and foot positions of oracle planners stepped after the estimator on every tick (scripts/Controller.py:213-236), gait
    codes changing on tick 35: what the handle's own planner holds when it is given the same q7 / vref / code.  planner: the
    oracle planners' configuration where it is not the default one."""
    plan = [oracle_mod.Planner(**planner) for _ in range(B)]
    sen = synth_mod.SyntheticSensors(B, seed, planner.get("dt_wbc", DT))
    vref = np.random.default_rng(seed).uniform(-0.4, 0.4, (B, 6)) * np.array([1.5, 0.8, 0, 0, 0, 1.0])
    q7 = np.tile(np.array([0.0, 0.0, planner.get("h_ref", 0.2229), 0.0, 0.0, 0.0, 1.0]), (B, 1))
    seq = []
    for k in range(ticks):
        code = np.array([[1, 2, 3, 4, 5][b % 5] if k == 35 else 0 for b in range(B)], np.int32)
        seq.append(dict(sensors=sen.step(k), gait=np.stack([p.gaits()[1] for p in plan]), goals=np.stack([p.feet()[0] for p in plan]),
                        plan=(q7, vref, code)))
        for b, p in enumerate(plan):
            p.step(k, q7[b], vref[b], vref[b], int(code[b]))
    return seq


def corner_sequence(corner, B=4, ticks=40):
    """Hand-made rows, one stance pattern per robot.  Returns (perfect, sequence)."""
    rng = np.random.default_rng(41 + CORNERS.index(corner))
    goals = rng.uniform(-0.2, 0.2, (B, 3, 4))
    eye4 = np.eye(4)
    first = dict(all_stance=[[1, 1, 1, 1]] * 4, all_swing=[[0, 0, 0, 0]] * 4, one_foot=eye4,
                 switch_on_tick_20=[[1, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0]],
                 attitude=[[1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 1]], perfect=[[1, 0, 0, 1]] * 4)[corner]
    second = [[0, 1, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 1, 1]]  # switch_on_tick_20: each robot's other pattern
    seq = []
    for k in range(ticks):
        d = _plain(B, rng)
        tick = dict(sensors=d, gait=_table(second if corner == "switch_on_tick_20" and k >= 20 else first, B), goals=goals)
        if corner == "attitude" and k >= 2:  # (the first two calls latch a zero yaw offset)
            # yaw just inside +pi and -pi; pitch clamped to +-pi/2 (2 qy qw = 1.125: a reading moved by one ulp is still clamped,
            # so that the tolerance measurement does not sit on the edge tests/test_gpu_estimator.py already pins)
            d["quat"] = np.array([_yaw_quat(np.pi - 1e-6), _yaw_quat(-np.pi + 1e-6), [0.0, 0.75, 0.0, 0.75], [0.0, -0.75, 0.0, 0.75]])
        if corner == "perfect":
            tick["true_pos"], tick["true_b_vel"] = rng.uniform(-1, 1, (B, 3)), rng.uniform(-1, 1, (B, 3))
        seq.append(tick)
    return corner == "perfect", seq


def sequences(oracle_mod, synth_mod):
    """Every input sequence this file compares against the checker: (name, B, estimator options, sequence).  What
    scripts/kalman_tolerance.py measures the bound on."""
    yield "trot_b17", 17, dict(), trot_sequence(synth_mod, 17, 200, 7)
    yield "trot_b1", 1, dict(), trot_sequence(synth_mod, 1, 200, 9)
    yield "planner", 5, dict(), planner_sequence(oracle_mod, synth_mod)
    for corner in CORNERS:
        perfect, seq = corner_sequence(corner)
        yield corner, 4, dict(perfect=perfect), seq
    yield "tuned", 4, dict(kalman=TUNED), trot_sequence(synth_mod, 4, 40, 11)
    yield "alt_trot_b17", 17, ALT_OPTIONS, alt_trot_sequence(synth_mod)
    yield "alt_planner", 5, ALT_OPTIONS, planner_sequence(oracle_mod, synth_mod, seed=18, **ALT_PLANNER)


def kalman_err(got, ref):
    """|got - ref| / max(1, |ref|), worst entry"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.max(np.where(np.isnan(e), np.inf, e)))


def covariance_err(got, ref):
    """P scaled by its own largest entry"""
    return kalman_err(np.asarray(got) / np.abs(ref).max(), np.asarray(ref) / np.abs(ref).max())


def checker_step(r, tick, b):
    r.run_filter(tick["gait"][b], tick["goals"][b], *[tick["sensors"][k][b] for k in SENSOR_KEYS],
                 true_pos=None if "true_pos" not in tick else tick["true_pos"][b],
                 true_b_vel=None if "true_b_vel" not in tick else tick["true_b_vel"][b])


# ------------------------------------------------------------------------------------------------ device against the checker
def _t(x, dtype=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def ekn(oracle_mod):
    import estimator_kalman_numpy

    return estimator_kalman_numpy


def _close(got, ref, what):
    assert np.allclose(got, ref, rtol=RTOL, atol=ATOL), (what, np.abs(np.asarray(got) - np.asarray(ref)).max(), got, ref)


def _device_step(eng, tick, planner=False, out=None):
    import torch

    opt = lambda name: None if name not in tick else _t(tick[name])
    o = eng.estimator_step(*[_t(tick["sensors"][k]) for k in SENSOR_KEYS], gait=None if planner else _t(tick["gait"]),
                           goals=None if planner else _t(tick["goals"]), true_pos=opt("true_pos"), true_b_vel=opt("true_b_vel"),
                           out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _compare(eng, out, refs, k, worst, robots=None):
    """robots: the instances of the handle the checker objects stand for (None: 0, 1, ...)."""
    import qrw_hip

    for b, r in enumerate(refs) if robots is None else zip(robots, refs):
        where = (k, b)
        figures = dict(q_filt=kalman_err(out["q_filt"][b], r.q_filt), v_filt=kalman_err(out["v_filt"][b], r.v_filt),
                       X=kalman_err(eng.estimator_kalman_get("X", b), r.X), P=covariance_err(eng.estimator_kalman_get("P", b), r.P))
        for name, e in figures.items():
            worst[name] = max(worst.get(name, 0.0), e)
            assert e <= KALMAN_BOUND, (name, where, e)
        _close(out["rpy"][b], r.RPY, ("rpy",) + where)
        _close(out["v_secu"][b], r.v_secu, ("v_secu",) + where)
        _close(eng.estimator_kalman_get("Z", b), r.Z, ("Z",) + where)
        want = r.items()
        assert set(want) == set(qrw_hip.ESTIMATOR_ITEMS)
        for name, ref in want.items():
            got = eng.estimator_get(name, b)
            if name in EXACT:
                assert np.array_equal(got, ref), (name, where, got, ref)
            else:
                _close(got, ref, (name,) + where)


def _run_against_checker(ekn, B, options, seq, planner=False):
    import torch

    import qrw_hip

    eng = qrw_hip.Batch(B, **options.get("handle", dict(n_steps=16, N_gait=N_GAIT)))
    if planner:
        eng.planner_init(**options.get("planner_init", {}))
    kalman = options.get("kalman", True)
    eng.estimator_init(H_INIT, options.get("perfect", False), kalman=kalman)
    refs = [ekn.Estimator(options.get("dt", DT), H_INIT, options.get("perfect", False), kalman=kalman) for _ in range(B)]
    worst, pout = {}, None
    for k, tick in enumerate(seq):
        out = _device_step(eng, tick, planner)
        for b, r in enumerate(refs):
            checker_step(r, tick, b)
        _compare(eng, out, refs, k, worst)
        if planner:
            q7, vref, code = tick["plan"]
            pout = eng.planner_step(k, _t(q7), _t(vref), _t(vref), _t(code, np.int32), out=pout)
            torch.cuda.synchronize()
    print("worst differences from the dense checker (bound %.2g): %s" % (KALMAN_BOUND, {n: "%.3g" % e for n, e in worst.items()}))
    return eng, refs


@pytest.mark.parametrize("B", [17, 1])
def test_trot_run_matches_the_dense_checker(oracle_mod, synth_mod, ekn, B):
    """B = 17 (one full wavefront of 16 quads plus one quad in a second block) and B = 1, 200 ticks of an explicit trot table
    (every foot switches ten times; robot b two rows ahead of b - 1), noisy sensors: q_filt, v_filt, rpy, v_secu, X, P, Z and
    every shared state item on every tick."""
    eng, refs = _run_against_checker(ekn, B, {}, trot_sequence(synth_mod, B, 200, 7 if B == 17 else 9))
    assert all(r.k_log == 200 for r in refs)
    assert eng.state_bytes() >= B * (47 + 142) * 8
    # the complementary filters are not stepped in this mode, and the height went into X[2] (scripts/Estimator.py:282-285)
    assert all(not eng.estimator_get(n, B - 1).any() for n in ("HP_lin_vel", "LP_lin_vel", "HP_lin_pos", "LP_lin_pos"))


def test_run_on_the_handles_planner_state(oracle_mod, synth_mod, ekn):
    """d_gait / d_goals NULL, 60 ticks: the filter's foot status comes from the planner's 64-bit column masks."""
    _run_against_checker(ekn, 5, {}, planner_sequence(oracle_mod, synth_mod), planner=True)


@pytest.mark.parametrize("corner", CORNERS)
def test_hand_made_rows(oracle_mod, ekn, corner):
    """B = 4, 40 ticks, one stance pattern per robot: all stance; all swing (every trust 0.01); exactly one foot; a switch on tick
    20; yaw just inside +-pi and pitch clamped; perfect=True with true_pos / true_b_vel."""
    perfect, seq = corner_sequence(corner)
    eng, refs = _run_against_checker(ekn, 4, dict(perfect=perfect), seq)
    if corner == "perfect":
        import torch

        out = _device_step(eng, seq[-1])  # (one more tick on the same readings: the override is what comes out)
        torch.cuda.synchronize()
        assert np.array_equal(out["q_filt"][:, 2], seq[-1]["true_pos"][:, 2] - 0.0155)
    if corner == "attitude":
        rpy = np.stack([r.RPY for r in refs])
        assert rpy[0, 2] > 3.14 and rpy[1, 2] < -3.14 and rpy[2, 1] == np.pi / 2 and rpy[3, 1] == -np.pi / 2


def test_other_time_step_and_gait_table_length(oracle_mod, synth_mod, ekn):
    """dt_wbc = 0.001 and gait matrices of 26 rows (ALT_HANDLE), B = 17, 120 ticks, noisy sensors: Q = sigma^2 dt^2, the
    prediction and the two first-order filters' coefficients all take the handle's dt.  Robots 2 and 9 have no zero row in their
    26, robots 5 and 16 have 26 equal rows (the scan for the end of the phase ends at N_gait); the tables advance six rows, so
    that about half of the others switch their stance pair.  And the time step matters: the checker at 0.002 gives another X."""
    seq = alt_trot_sequence(synth_mod)
    assert all(t["gait"].shape == (17, ALT_N_GAIT, 4) for t in seq)
    assert all(seq[0]["gait"][b].any(axis=1).all() for b in ALT_FULL + ALT_STILL) and not seq[0]["gait"][0, 16:].any()
    assert all((seq[-1]["gait"][b] == seq[-1]["gait"][b, 0]).all() for b in ALT_STILL)
    eng, refs = _run_against_checker(ekn, 17, ALT_OPTIONS, seq)
    assert all(r.k_log == 120 for r in refs) and {r.remaining_steps for r in refs} >= {ALT_N_GAIT, 1, 7}
    plain = ekn.Estimator(DT, H_INIT)
    for tick in seq:
        checker_step(plain, tick, 0)
    assert kalman_err(plain.X, refs[0].X) > 1e3 * KALMAN_BOUND


def test_other_configuration_on_the_handles_planner_state(oracle_mod, synth_mod, ekn):
    """The same configuration with d_gait / d_goals NULL: the handle's planner (k_mpc = 20, T_gait = 0.40, 26-row matrices as
    64-bit column masks) against oracle planners of that configuration, B = 5, 60 ticks."""
    _run_against_checker(ekn, 5, ALT_OPTIONS, planner_sequence(oracle_mod, synth_mod, seed=18, **ALT_PLANNER), planner=True)


def test_non_default_tuning(oracle_mod, synth_mod, ekn):
    """All five tuning values changed, in the kernel and in the checker; and they matter: the default tuning gives another X."""
    seq = trot_sequence(synth_mod, 4, 40, 11)
    eng, refs = _run_against_checker(ekn, 4, dict(kalman=TUNED), seq)
    plain = ekn.Estimator(DT, H_INIT)
    for tick in seq:
        checker_step(plain, tick, 0)
    assert kalman_err(plain.X, refs[0].X) > 1e3 * KALMAN_BOUND


# ------------------------------------------------------------------------------------------------ re-initialisation, NaN
def _record(eng, seq, B):
    """Outputs and (in Kalman mode) X / P / Z of every robot after every tick."""
    import qrw_hip

    rec = []
    for tick in seq:
        out = _device_step(eng, tick)
        row = [out[n] for n in ("q_filt", "v_filt", "rpy", "v_secu")]
        row += [np.stack([eng.estimator_get(n, b) for b in range(B)]) for n in qrw_hip.ESTIMATOR_ITEMS]
        if eng.estimator_kalman:
            row += [np.stack([eng.estimator_kalman_get(n, b) for b in range(B)]) for n in ("X", "P", "Z")]
        rec.append(row)
    return rec


def _identical(rec_a, rec_b, robots=slice(None)):
    assert len(rec_a) == len(rec_b)
    for k, (a, b) in enumerate(zip(rec_a, rec_b)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x[robots], y[robots], equal_nan=True), (k, i)


B83 = 83  # six blocks of 16 quads (the last holding three) for the step kernels, two blocks of 64 robots for estimator_init_kernel


def block_coverage(synth_mod, kalman, make_ref, compare):
    """estimator_init and 20 ticks at B = 83, robot i fed the inputs of robot src[i] of the 17-robot trot sequence (a fixed
    permutation, so that equal robots do not sit 17 apart): every output and item of robot i is bit for bit that of robot src[i]
    in a B = 17 handle on every tick, and the first tick of robots 64..82 -- initialised by the init kernel's second block --
    is compared with the checker (make_ref() -> a fresh checker object; compare(eng, out, refs, robots))."""
    import qrw_hip

    seq = trot_sequence(synth_mod, 17, 20, 19)
    src = np.random.default_rng(83).permutation(B83) % 17
    assert set(src) == set(range(17))
    wide = [dict(sensors={n: v[src] for n, v in t["sensors"].items()}, gait=t["gait"][src], goals=t["goals"][src]) for t in seq]
    small, large = qrw_hip.Batch(17, 16, N_GAIT), qrw_hip.Batch(B83, 16, N_GAIT)
    for eng in (small, large):
        eng.estimator_init(H_INIT, kalman=kalman)
    rec = _record(large, wide[:1], B83)
    second_block = list(range(64, B83))
    refs = [make_ref() for _ in second_block]
    for b, r in zip(second_block, refs):
        checker_step(r, wide[0], b)
    compare(large, dict(zip(("q_filt", "v_filt", "rpy", "v_secu"), rec[0][:4])), refs, second_block)
    rec += _record(large, wide[1:], B83)
    want = _record(small, seq, 17)
    assert len(rec) == len(want) == 20
    for k, (a, b) in enumerate(zip(rec, want)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y[src], equal_nan=True), (k, i, np.nonzero(np.any((x != y[src]).reshape(B83, -1), axis=1))[0])
    assert all(np.isfinite(x).all() for x in rec[-1])


def test_block_coverage(oracle_mod, synth_mod, ekn):
    """block_coverage for the Kalman filter: X, P and Z among the items."""
    block_coverage(synth_mod, True, lambda: ekn.Estimator(DT, H_INIT),
                   lambda eng, out, refs, robots: _compare(eng, out, refs, 0, {}, robots))


def test_reinitialisation_in_either_direction_is_a_fresh_handle(synth_mod):
    """Bit for bit: init_kalman -> 10 steps -> init_kalman reproduces the first run; init_kalman -> steps -> estimator_init ->
    steps is a fresh complementary handle; the reverse is a fresh Kalman handle."""
    import qrw_hip

    B = 4
    seq = trot_sequence(synth_mod, B, 10, 13)
    fresh_kalman = qrw_hip.Batch(B, 16, N_GAIT)
    fresh_kalman.estimator_init(H_INIT, kalman=True)
    want_kalman = _record(fresh_kalman, seq, B)
    fresh_plain = qrw_hip.Batch(B, 16, N_GAIT)
    fresh_plain.estimator_init(H_INIT)
    bytes_plain = fresh_plain.state_bytes()
    want_plain = _record(fresh_plain, seq, B)
    assert fresh_plain.state_bytes() == bytes_plain and fresh_kalman.state_bytes() == bytes_plain + B * 142 * 8

    eng = qrw_hip.Batch(B, 16, N_GAIT)
    eng.estimator_init(H_INIT, kalman=True)
    _identical(_record(eng, seq, B), want_kalman)
    eng.estimator_init(H_INIT, kalman=True)
    _identical(_record(eng, seq, B), want_kalman)
    eng.estimator_init(H_INIT)
    _identical(_record(eng, seq, B), want_plain)
    eng.estimator_init(H_INIT, kalman=True)
    _identical(_record(eng, seq, B), want_kalman)
    assert eng.state_bytes() == bytes_plain + B * 142 * 8  # (allocated once)


def test_a_nan_reading_stays_with_its_robot(synth_mod):
    """A NaN acceleration for robot 3 of 17 from tick 5 on: the other 16 robots are bit-identical to the run without it over 20
    ticks, and robot 3's filter state is not finite from then on, as in the reference."""
    import qrw_hip

    B = 17
    seq = trot_sequence(synth_mod, B, 20, 14)
    bad = [dict(t, sensors=dict(t["sensors"], lin_acc=t["sensors"]["lin_acc"].copy())) for t in seq]
    for t in bad[5:]:
        t["sensors"]["lin_acc"][3, 1] = np.nan
    recs = []
    for s in (seq, bad):
        eng = qrw_hip.Batch(B, 16, N_GAIT)
        eng.estimator_init(H_INIT, kalman=True)
        recs.append(_record(eng, s, B))
    others = [b for b in range(B) if b != 3]
    _identical(recs[0], recs[1], others)
    _identical(recs[0][:5], recs[1][:5])
    assert all(not np.isfinite(recs[1][k][-3][3]).all() for k in range(5, 20))  # X of robot 3
    assert all(np.isfinite(row[-3][others]).all() and np.isfinite(row[-2][others]).all() for row in recs[1])


# ------------------------------------------------------------------------------------------------ fleet
def _fleet_inputs(synth_mod, B, ticks, seed):
    sen = synth_mod.SyntheticSensors(B, seed)
    rng = np.random.default_rng(seed)
    vref = rng.uniform(-0.4, 0.4, (B, 6)) * np.array([1.5, 0.8, 0, 0, 0, 1.0])
    return vref, [sen.step(k) for k in range(ticks)]


def _run_fleet(ctl, vref, ticks, separate=False):
    """compute_sensors over the ticks (separate: compute() fed with the outputs of a separate Kalman estimator_step on ctl's
    handle); returns per tick (result, error flags, q_filt, v_filt, rpy, v_secu) as host arrays."""
    import torch

    vr, rec, o = _t(vref), [], None
    result = ctl._fleet_result if hasattr(ctl, "_fleet_result") else None  # (stream groups: the fleet's tensor)
    if separate:
        ctl._b.estimator_init(H_INIT, kalman=True)
    for d in ticks:
        s = [_t(d[k]) for k in SENSOR_KEYS]
        if separate:
            o = ctl._b.estimator_step(*s, out=o)
            ctl.compute(vr, o["q_filt"], o["v_filt"], o["rpy"], o["v_secu"])
            est = [o[n] for n in ("q_filt", "v_filt", "rpy", "v_secu")]
        else:
            ctl.compute_sensors(vr, *s)
            est = [ctl.q_filt, ctl.v_filt, ctl.rpy, ctl.v_secu]
        torch.cuda.current_stream().synchronize()
        rec.append([x.cpu().numpy().copy() for x in [ctl._res["result"] if result is None else result, ctl.error_flag] + est])
    return rec


KALMAN_FLEET = dict(h_init=H_INIT, kalman=True)


def test_fleet_compute_sensors_is_estimator_step_then_compute(synth_mod):
    """Controller_batch(B=32, estimator=dict(kalman=True)).compute_sensors over 30 ticks (three solves): bit for bit compute() fed
    with a separate Kalman estimator_step; and not what the complementary filters give."""
    from Controller import Controller_batch

    B, T = 32, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 31)
    ctl = Controller_batch(B, Q_INIT, estimator=KALMAN_FLEET)
    a = _run_fleet(ctl, vref, ticks)
    assert ctl._b.estimator_kalman and ctl._b.estimator_kalman_get("P", B - 1).shape == (18, 18)
    _identical(a, _run_fleet(Controller_batch(B, Q_INIT), vref, ticks, separate=True))
    plain = _run_fleet(Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT)), vref, ticks)
    assert not np.array_equal(a[-1][2][:, :3], plain[-1][2][:, :3])


def test_fleet_stream_groups_are_bit_identical_to_one_handle(synth_mod):
    from Controller import Controller_batch, Controller_groups

    B, T = 32, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 32)
    one = _run_fleet(Controller_batch(B, Q_INIT, estimator=KALMAN_FLEET), vref, ticks)
    ctl = Controller_batch(B, Q_INIT, groups=2, estimator=KALMAN_FLEET)
    assert isinstance(ctl, Controller_groups) and all(g._b.estimator_kalman for g in ctl.groups)
    _identical(one, _run_fleet(ctl, vref, ticks))


def test_fleet_asynchronous_mode_matches_its_synchronous_estimator_counterpart(synth_mod):
    """multiprocessing=True, mpc_lag=3: the Kalman estimator enqueued on the loop's stream by compute_sensors against the same
    controller fed by a separate estimator_step on the caller's stream."""
    import torch
    from Controller import Controller_batch

    B, T = 32, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 33)
    with torch.cuda.stream(torch.cuda.Stream()):
        ca = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=KALMAN_FLEET)
        a = _run_fleet(ca, vref, ticks)
        ca.stop_parallel_loop()
        cb = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3)
        b = _run_fleet(cb, vref, ticks, separate=True)
        cb.stop_parallel_loop()
    _identical(a, b)


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_handle_usable(oracle_mod, ekn):
    import qrw_hip

    B = 2
    rng = np.random.default_rng(23)
    eng = qrw_hip.Batch(B, 16, N_GAIT)
    tick = dict(sensors=_plain(B, rng), gait=_table([1, 1, 1, 1], B), goals=np.zeros((B, 3, 4)))
    get = lambda which, b, count: qrw_hip._check(
        eng._lib.qrw_estimator_kalman_get_host(eng._handle, which, b, count, qrw_hip._p(np.empty(400))), "qrw_estimator_kalman_get_host")
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_kalman_get_host: not in Kalman mode"):
        eng.estimator_kalman_get("X", 0)  # (no estimator at all yet)
    eng.estimator_init(H_INIT)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_kalman_get_host: not in Kalman mode"):
        eng.estimator_kalman_get("X", 0)
    with pytest.raises(qrw_hip.QrwError, match=r"kalman=: unknown keys \['sigma'\]"):
        eng.estimator_init(H_INIT, kalman=dict(sigma=1.0))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_init_kalman: the sigmas must be > 0"):
        eng.estimator_init(H_INIT, kalman=dict(sigma_h=0.0))
    _device_step(eng, tick)  # (still the complementary estimator, and usable)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_kalman_get_host: not in Kalman mode"):
        get(0, 0, 18)
    eng.estimator_init(H_INIT, kalman=True)
    for which, b, count, text in ((3, 0, 1, "bad item"), (-1, 0, 1, "bad item"), (0, 0, 19, "bad item"), (1, 0, 325, "bad item"),
                                  (2, 0, 17, "bad item"), (0, B, 18, "bad argument"), (0, -1, 18, "bad argument"),
                                  (0, 0, 0, "bad argument")):
        with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_kalman_get_host: " + text):
            get(which, b, count)
    assert np.array_equal(eng.estimator_kalman_get("X", 1), np.concatenate([[0.0, 0.0, H_INIT], np.zeros(15)]))
    assert np.array_equal(eng.estimator_kalman_get("P", 1), np.eye(18)) and not eng.estimator_kalman_get("Z", 1).any()
    refs = [ekn.Estimator(DT, H_INIT) for _ in range(B)]
    out = _device_step(eng, tick)
    for b, r in enumerate(refs):
        checker_step(r, tick, b)
    _compare(eng, out, refs, 0, {})
