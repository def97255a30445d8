"""oracle/planner_oracle.c held against a second implementation of the planners, tests/planner_numpy.py, which is written from
the reference's C++ and differs in method where it can (dense matrices and np.roll, argmin instead of row walks, the swing's
height in factored form, the swing's x / y quintic solved from its boundary conditions in longdouble).  A misreading of the
reference shared by the oracle and the kernel would show here; the GPU tests keep comparing with the oracle.  CPU only."""
import numpy as np
import pytest

import planner_cases as pc
import planner_numpy as pn

CONFIGS = ("default", "alt", "short_period", "full20", "wide", "TUNED", "wild") + pc.STEPS
ROBOTS = 3  # of the case's robots (the oracle's run over all of them is shared with the other tests)


def test_solved_quintic_is_the_closed_form():
    """The polynomial solved from the six boundary conditions, expanded into powers of absolute time, against the reference's
    closed-form coefficients (FootTrajectoryGenerator.cpp:57-62) over 2 000 random (t, d, x0, dx0, ddx0, target) with the lock time
    respected (d - t >= 0.04): every coefficient agrees to rounding.  The closed form divides by 2 (t - d)^5 written as an
    expanded cubic times a square, which cancels to about eps d^3 / (d - t)^3 <= 4e-13 of the largest term; the bound is 1e-10
    of the largest term A[n] d^(5-n).  Largest ratio seen: 7.9e-13.  And the solved polynomial meets its boundary conditions."""
    rng = np.random.default_rng(12)
    worst = 0.0
    for _ in range(2000):
        d = rng.uniform(0.06, 0.62)
        t = rng.uniform(0.0, d - 0.04)
        x0, dx0, ddx0, tg = rng.uniform(-0.3, 0.3), rng.uniform(-2, 2), rng.uniform(-50, 50), rng.uniform(-0.3, 0.3)
        c = pn.solve_quintic(d - t, x0, dx0, ddx0, tg)
        A, ref = pn.monomials(c, t), pn.closed_form(t, d, x0, dx0, ddx0, tg)
        terms = np.abs(ref) * d ** np.arange(6)[::-1]
        ratio = float((np.abs(np.asarray(A, dtype=np.float64) - ref) * d ** np.arange(6)[::-1]).max() / terms.max())
        worst = max(worst, ratio)
        D = np.longdouble(d - t)
        end = [sum(c[n] * D ** n for n in range(6)), sum(n * c[n] * D ** (n - 1) for n in range(1, 6)), sum(n * (n - 1) * c[n] * D ** (n - 2) for n in range(2, 6))]
        assert abs(float(end[0]) - tg) < 1e-15 and abs(float(end[1])) < 1e-12 and abs(float(end[2])) < 1e-9
        assert (float(c[0]), float(c[1]), float(2 * c[2])) == (x0, dx0, ddx0)
    print("solved quintic against the closed form: largest difference of a term / largest term %.2g" % worst)
    assert worst < 1e-10


def test_swing_height_factored_form_is_the_four_monomials():
    """h 64 (e (d - e))^3 / d^6 and its two derivatives against the reference's Az (FootTrajectoryGenerator.cpp:76-80,103-105)."""
    rng = np.random.default_rng(13)
    for _ in range(500):
        d, h = rng.uniform(0.04, 0.62), rng.uniform(0.02, 0.1)
        e = rng.uniform(0.0, d)
        dz = (d / 2) ** 3 * (d - d / 2) ** 3
        Az = [-h / dz, 3 * d * h / dz, -3 * d ** 2 * h / dz, d ** 3 * h / dz]
        ref = (Az[3] * e ** 3 + Az[2] * e ** 4 + Az[1] * e ** 5 + Az[0] * e ** 6,
               3 * Az[3] * e ** 2 + 4 * Az[2] * e ** 3 + 5 * Az[1] * e ** 4 + 6 * Az[0] * e ** 5,
               6 * Az[3] * e + 12 * Az[2] * e ** 2 + 20 * Az[1] * e ** 3 + 30 * Az[0] * e ** 4)
        u, du, scale = e * (d - e), d - 2 * e, 64.0 * h / d ** 6
        got = (scale * u ** 3, scale * 3 * u ** 2 * du, scale * (6 * u * du ** 2 - 6 * u ** 2))
        eps20 = 20 * np.finfo(np.float64).eps  # (planner_cases.z_bound: the sums of the magnitudes of the four terms)
        assert abs(got[0] - ref[0]) <= eps20 * 512 * h and abs(got[1] - ref[1]) <= eps20 * 2304 * h / d and abs(got[2] - ref[2]) <= eps20 * 8448 * h / d ** 2


def test_rule_and_refusals_agree_with_the_oracle(oracle_mod):
    lib = oracle_mod.load()
    for N_gait in (2, 9, 15, 16, 18, 20, 63, 64):
        for n_steps in (1, 8, 16, 32):
            for T in (0.16, 0.30, 0.32, 0.36, 0.40, 1.22, 1.24, 1.26):
                assert pn.table_fits(N_gait, n_steps, T, 0.02) == bool(lib.planner_oracle_table_fits(N_gait, n_steps, T, 0.02)), (N_gait, n_steps, T)
    # off the 0.02 s step: periods of 1 .. 64 rows (T = rows * dt as the caller would compute it) and periods with halves in them
    yes = no = 0
    for dt in (0.01, 0.016, 0.024, 0.025, 0.04):
        for N_gait in (2, 9, 15, 16, 18, 20, 24, 63, 64):
            for n_steps in (1, 8, 12, 16, 20, 32):
                for T in [rows * dt for rows in (1, 2, 7, 8, 12, 15, 16, 18, 19, 20, 21, 24, 61, 62, 63, 64)] + [7.5 * dt, 12.5 * dt, 0.20, 0.32, 0.36, 0.40, 0.48]:
                    fits = pn.table_fits(N_gait, n_steps, T, dt)
                    assert fits == bool(lib.planner_oracle_table_fits(N_gait, n_steps, T, dt)), (N_gait, n_steps, T, dt)
                    yes, no = yes + fits, no + (not fits)
    assert yes > 500 and no > 500, (yes, no)
    with pytest.raises(ValueError):
        pn.Planner(N_gait=63, T_gait=1.24)
    with pytest.raises(ValueError):
        pn.Planner(N_gait=10)


@pytest.mark.parametrize("case", CONFIGS)
def test_oracle_matches_the_second_implementation(oracle_mod, case):
    """Every output of every iteration of the oracle's run (planner_cases.oracle_run) against planner_numpy over the case's
    sequence, robots 0..2: gait matrices (past, current, desired), contacts and flags exactly; xref, fsteps, target, foot position /
    velocity / acceleration within 100 x the oracle's own spread (planner_cases.SPREAD, scripts/planner_tolerance.py), swing
    durations and clocks exactly."""
    c, seq, ref = pc.CASES[case], pc.sequence(case), pc.oracle_run(oracle_mod, case)
    K = seq["code"].shape[0]
    g = dict(c["geometry"])
    robots = range(min(ROBOTS, c["B"]))
    mine = [pn.Planner(c["dt_mpc"], c["dt_wbc"], c["T_gait"], c["N"] * c["dt_mpc"], c["N_gait"], c["k_mpc"], g.get("h_ref", 0.2229),
                       g.get("shoulders"), g.get("max_height", 0.05), g.get("lock_time", 0.07), g.get("init_target"), g.get("init_foot_pos"))
            for _ in robots]
    worst = dict.fromkeys(pc.FLOAT_OUTPUTS, 0.0)
    locked = pc.SPREAD[case]["pos"] == 0.0  # (short_period: every swing is shorter than the lock time)
    zb = pc.z_bound(oracle_mod, case) if locked else None
    for k in range(K):
        for b, p in zip(robots, mine):
            p.step(k, seq["q7"][k, b], seq["hv"][k, b], seq["vref"][k, b], int(seq["code"][k, b]))
            past, cur, des = p.gaits()
            assert np.array_equal(cur, ref["gait"][k, b]), (case, k, b)
            f = p.flags()
            assert [f["new_phase"], f["is_static"], f["remaining_time"], f["n_swing"]] == list(ref["flags"][k, b]), (case, k, b)
            fs, _, otg = p.footsteps()
            pos, vel, acc, _, tsw = p.feet_state()
            assert np.array_equal(tsw, ref["tsw"][k, b]), (case, k, b)
            got = dict(xref=p.xref(), fsteps=fs, target=otg, pos=pos, vel=vel, acc=acc)
            for name in pc.FLOAT_OUTPUTS:
                if locked and name in ("pos", "vel", "acc"):
                    # no input reaches the trajectories (spread 0): x / y exactly, z within the number format's bound
                    assert np.array_equal(got[name][:2], ref[name][k, b][:2]), (case, k, b, name)
                    assert np.abs(got[name][2] - ref[name][k, b][2]).max() <= zb[k, b, ("pos", "vel", "acc").index(name)], (case, k, b, name)
                    continue
                e = pc.err(got[name], ref[name][k, b])
                worst[name] = max(worst[name], e)
                assert e <= pc.bound(case, name), (case, k, b, name, e, pc.bound(case, name))
            if k in ref["state"]:
                opast, odes, oft = ref["state"][k][b]
                assert np.array_equal(past, opast) and np.array_equal(des, odes), (case, k, b)
                assert pc.err(p.ft_target(), oft) <= pc.bound(case, "ft_target"), (case, k, b)
    print("%s: oracle against the second implementation, err / bound: %s" % (case, "  ".join("%s %.2e / %.2e" % (n, w, pc.bound(case, n)) for n, w in worst.items())))
