"""tests/planner_cases.py held against itself on the CPU: the recorded spreads are the measured ones, every geometry parameter
changed alone moves the oracle's outputs by far more than a bound, the cases are what their names say, and the oracle's
behaviour with a lock time longer than the swing is the reference's."""
import numpy as np
import pytest

import planner_cases as pc


@pytest.mark.parametrize("case", list(pc.CASES))
def test_recorded_spreads_are_the_measured_ones(oracle_mod, case):
    """planner_cases.SPREAD[case] is spread() of the case to its three digits (scripts/planner_tolerance.py prints the record);
    libm differences between machines stay far below the factor 2 allowed here.  The bounds are 100 x these figures."""
    measured = pc.spread(oracle_mod, case)
    print(case, "  ".join("%s %.2e" % (n, measured[n]) for n in pc.FLOAT_OUTPUTS))
    for name in pc.FLOAT_OUTPUTS:
        rec = pc.SPREAD[case][name]
        assert 0.5 * rec <= measured[name] <= 2.0 * rec, (case, name, measured[name], rec)
        assert pc.bound(case, name) == pytest.approx(100.0 * rec)
    # the figures are spreads of a double-precision computation, not slack: nothing above 1e-6 even where the swing polynomial
    # amplifies most (the 1.22 s gait of `wide`), and a rounding error at least wherever an input reaches the output
    assert all(v < 1e-6 for v in pc.SPREAD[case].values())
    assert all(pc.SPREAD[case][n] > 5e-17 for n in ("xref", "fsteps", "target"))


# the outputs each parameter must move (scripts/planner_tolerance.py prints every ratio)
MOVES = dict(shoulders=("fsteps", "target", "pos"), h_ref=("xref", "fsteps", "target"), max_height=("pos", "vel", "acc"),
             lock_time=("pos", "vel", "acc"), init_target=("ft_target",), init_foot_pos=("pos", "vel", "acc"))


@pytest.mark.parametrize("case", pc.ALONE)
def test_each_parameter_alone_moves_the_oracle_by_more_than_1000_bounds(oracle_mod, case):
    """The oracle's run with one geometry parameter changed against its run with the defaults, same sequence: the outputs the
    parameter feeds differ by more than 1000 bounds somewhere in the run, so a device that ignored the parameter could not pass
    tests/test_gpu_planner_params.py.  init_target reaches nothing but the trajectory generator's own copy of the target (item 17
    of qrw_planner_get_host), which is why the GPU tests compare that item."""
    e = pc.effect(oracle_mod, case)
    for name in MOVES[case]:
        assert e[name] > 1000.0 * pc.bound(case, name), (case, name, e[name], pc.bound(case, name))
    if case == "init_target":
        assert all(e[n] == 0.0 for n in pc.FLOAT_OUTPUTS)


def test_cases_are_what_their_names_say(oracle_mod):
    want = dict(full20=(20, 20), walk_fills=(18, 20), odd=(15, 16), wide=(61, 62), tight=(8, 8),
                step10=(20, 20), step40=(12, 12), step16=(20, 20), step24=(15, 16), step25=(16, 16))
    for case, (rows, need) in want.items():
        c = pc.CASES[case]
        assert pc.lround(c["T_gait"] / c["dt_mpc"]) == rows and pc.rows_needed(case) == need
        assert oracle_mod.load().planner_oracle_rows_needed(c["T_gait"], c["dt_mpc"]) == need
        assert oracle_mod.load().planner_oracle_table_fits(c["N_gait"], c["N"], c["T_gait"], c["dt_mpc"])
        events, K = pc.code_schedule(case)
        codes = {b: [cd for k in sorted(events) for bb, cd in events[k].items() if bb == b] for b in range(c["B"])}
        assert all(any(x == 4 and y != 4 for x, y in zip(v, v[1:])) for v in codes.values())  # static and away again, every robot
        assert {cd for v in codes.values() for cd in v} == {1, 2, 3, 4, 5}
        assert K - 1 - max(events) >= 2 * need * c["k_mpc"]                               # two of the longest periods after the last change
        assert any(k % c["k_mpc"] for k in events) and any(k % c["k_mpc"] == 0 for k in events)
    assert pc.CASES["tight"]["N"] + 1 == pc.CASES["tight"]["N_gait"] and pc.CASES["wide"]["N_gait"] == 63
    assert set(want) == set(pc.LIMITS + pc.STEPS)
    for case in pc.STEPS:  # off the 0.02 s step, with the loop's step a whole fraction of the MPC's
        c = pc.CASES[case]
        assert c["dt_mpc"] != 0.02 and c["k_mpc"] * c["dt_wbc"] == pytest.approx(c["dt_mpc"], rel=1e-15) and c["seq"] == "limits"
    for case in pc.CASES:
        seq = pc.sequence(case)
        assert (seq["vref"][:, 0, 5] == 0.0).any() and (seq["code"] != 0).any() and np.abs(seq["hv"] - seq["vref"]).max() > 0.05


def test_lock_time_longer_than_the_swing_leaves_the_coefficients_zero(oracle_mod):
    """The oracle with lock_time = 0.5: a swinging foot whose clock is inside its swing has x / y position, velocity and
    acceleration exactly 0 (the never-updated coefficients, FootTrajectoryGenerator.cpp:28-29,53,76-86), z follows the usual bump,
    and no input reaches the trajectories at all (spread 0)."""
    run = pc.oracle_run(oracle_mod, "lock_long")
    swing = run["gait"][:, :, 0, :] == 0
    assert swing.any() and not swing.all()
    for name in ("pos", "vel", "acc"):
        xy = run[name][:, :, :2]
        assert (xy[np.broadcast_to(swing[:, :, None, :], xy.shape)] == 0.0).all(), name
    assert run["pos"][:, :, 2].max() > 0.049 and run["pos"][:, :, 2].min() > -1e-9
    assert all(pc.SPREAD["lock_long"][n] == 0.0 for n in ("pos", "vel", "acc"))
    zb = pc.z_bound(oracle_mod, "lock_long")
    assert np.isfinite(zb).all() and zb[-1].max() < 1e-8 and (zb[:, :, 0] > 1e-15).all()
