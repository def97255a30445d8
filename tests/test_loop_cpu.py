"""The whole-loop scenarios of tests/loop_cases.py are what they claim, on the reference side alone (no GPU): the chained checkers
of tests/loop_chain.py free-run every variant as a closed loop -- simulator -> estimator -> controller chain -> simulator, the
joystick in front -- and the run is held to what tests/test_gpu_loop.py relies on: who walks and who stops, with which margin
the flags rise, that the latch, the codes and the contact switch behave as the scenario table says, and that the recorded
one-ulp spreads (LOOP_TICK_SPREAD) are the measured ones.  About 35 s in all, the spread measurement included."""
import numpy as np
import pytest

import joystick_numpy as jn
import loop_cases as lc

MIN_ABS_D = 1e-9  # tests/test_gpu_sim.py's: no state may come nearer to the contact law's switch
_RUNS = {}


@pytest.fixture
def run(oracle_mod, request):
    """The free run of a variant, made once per session."""
    variant = request.param
    if variant not in _RUNS:
        _RUNS[variant] = lc.free_run(variant, measure_spread=True)
    return variant, _RUNS[variant]


every_variant = pytest.mark.parametrize("run", list(lc.VARIANTS), indirect=True)


@every_variant
def test_walkers_walk_stoppers_stop_and_the_latch_follows_the_flag(run):
    """Robots meant to walk never raise a flag and the simulator never freezes them; the others raise theirs inside their window,
    the latch closes on the next tick and v_ref, code and f_ext are zero from there on -- a push still scheduled included --;
    every commanded code reaches gait row 0 where the run is long enough; the variant's contact counts are all seen."""
    variant, cs = run
    f, a = lc.fleet(variant), lc.arrays(cs)
    seen = lc.check_scenario(variant, **a)
    stopped = [b for b in range(f["B"]) if f["stops"][b] is not None]
    assert stopped, variant
    pushed = [b for b in stopped if f["pushes"][b]]
    assert pushed, variant
    for b in pushed:  # a push is still scheduled when the latch closes, and would have acted inside the run
        k_stop = int(a["k_stop"][b])
        unlatched = jn.JoystickNumpy(k_switch=f["profiles"][b][0], v_switch=f["profiles"][b][1], pushes=f["pushes"][b])
        assert any(unlatched.apply_external_forces(k).any() for k in range(k_stop, f["T"])), (variant, f["names"][b], k_stop)
    print("%s: flags %s, k_stop %s, feet in contact seen %s" % (variant, [lc.flag_tick(a["flags"][:, b]) for b in range(f["B"])],
                                                               a["k_stop"].tolist(), seen))


@every_variant
def test_flags_rise_with_a_margin(run):
    """|tau_ff| against 8, |v_secu| against 50 and |q| against q_security stay 1e-3 (relative) inside on every tick before a flag
    and the raising quantity is 1e-3 outside on the raising tick: ten times what the controller comparison allows, so the device
    cannot raise the flag a tick earlier or later without failing that comparison first."""
    variant, cs = run
    f, a = lc.fleet(variant), lc.arrays(cs)
    for b, c in enumerate(cs):
        got = lc.check_margins(f["names"][b], a["flags"][:, b], [t["ratios"] for t in c.trace])
        assert (got is None) == (f["stops"][b] is None)
        if got is not None:
            print("%s %s: flag %d at tick %d, its quantity %.4f of the limit the tick before, %.4f on it" % ((variant, f["names"][b], got[1], got[0]) + got[2:]))


@pytest.mark.parametrize("run", ["plane"], indirect=True)
def test_the_plane_fleet_travels_yaws_and_is_pushed_off_its_pattern(run):
    """Robot 0 ends beyond 0.1 m with a yaw above 0.15 rad; the moderately pushed robot leaves the four-feet / two-feet pattern and
    is moved sideways; the strongly pushed one raises flag 3, the fast ramp a flag; the backwards robot went back and yawed."""
    cs = run[1]
    names = lc.fleet("plane")["names"]
    q = cs[names.index("forward_yaw")].sim.q
    yaw = np.arctan2(2.0 * (q[6] * q[5] + q[3] * q[4]), 1.0 - 2.0 * (q[4] ** 2 + q[5] ** 2))
    assert np.hypot(q[0], q[1]) > 0.1 and yaw > 0.15, (q[:7], yaw)
    pushed = cs[names.index("push_moderate")]
    assert {1, 3} & {t["feet"] for t in pushed.trace[100:]} and abs(pushed.sim.q[1]) > 0.1
    assert cs[names.index("push_strong")].trace[-1]["flag"] == 3 and cs[names.index("fast_ramp")].trace[-1]["flag"] != 0
    back = cs[names.index("back_yaw_push")].sim.q
    assert back[0] < -0.03 and back[5] < -0.02, back[:7]


@every_variant
def test_no_state_sits_on_the_contact_switch_and_the_recorded_spreads_are_the_measured_ones(run):
    """LOOP_TICK_SPREAD[variant] is what this free run measures (scripts/loop_tolerance.py prints the record): the simulator and the
    estimator checkers against themselves from inputs moved up by one ulp, and the smallest |d| of the run.  Differences of libm
    or BLAS between machines stay far below the factor 2 allowed.  tests/test_gpu_loop.py's bounds are 100 x the spreads."""
    variant, cs = run
    m, rec = lc.measured(cs), lc.LOOP_TICK_SPREAD[variant]
    print(variant, "  ".join("%s %.3g" % kv for kv in m.items()))
    assert all(min(c.sim.min_abs_d, c.sim_p.min_abs_d) > MIN_ABS_D for c in cs), m
    for name in ("sim", "est", "min_abs_d"):
        assert 0.5 * rec[name] <= m[name] <= 2.0 * rec[name], (variant, name, m[name], rec[name])
    assert 5e-17 < rec["est"] < rec["sim"] < 1e-8  # spreads of double-precision computations, not slack
