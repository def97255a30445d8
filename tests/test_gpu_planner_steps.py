"""GPU tests of the batched planners off the 0.02 s MPC step (planner_kernel.hip in its thread form through qrw_planner_step)
against the oracle.  dt_mpc advances the clocks of the live rows (dtc_prev + dt_mpc), builds the time vector of xref, sets
T_mpc = dt_mpc * n_steps, sizes the gait generators (lround(0.5 T_gait / dt_mpc), ...) and scales getPhaseDuration
(cnt * dt_mpc); every other planner test passes 0.02.  Cases, sequences, the oracle's runs and the bounds come from
tests/planner_cases.py (STEPS); tests/test_planner_second_impl.py and tests/test_gait_masks_cpu.py hold the oracle and the mask
arithmetic at these steps on the CPU."""
import pytest

import planner_cases as pc
from test_gpu_planner_limits import run_against_the_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pc.STEPS)
def test_planner_at_other_steps_matches_oracle(oracle_mod, case):
    """B = 9, every robot with its own gait changes (the `limits` schedule: codes 1..5, static and away again, on rolling and
    non-rolling iterations), at steps of 0.010, 0.040, 0.016, 0.024 and 0.025 s with k_mpc = dt_mpc / dt_wbc loop iterations
    between two rolls.  Measured on the device (err, see planner_cases; the bound is 100 x the oracle's spread,
    planner_cases.SPREAD), worst over the run:
        step10   xref 1.1e-16  fsteps 3.9e-16  target 4.4e-16  pos 1.1e-11  vel 2.2e-11  acc 2.4e-10
        step40   xref 1.1e-16  fsteps 1.8e-15  target 1.6e-15  pos 1.5e-09  vel 6.1e-09  acc 9.4e-09
        step16   xref 1.1e-16  fsteps 1.1e-15  target 1.1e-15  pos 4.9e-11  vel 5.9e-10  acc 6.3e-09
        step24   xref 1.1e-16  fsteps 6.1e-16  target 6.7e-16  pos 7.6e-10  vel 9.2e-10  acc 1.4e-08
        step25   xref 1.1e-16  fsteps 6.7e-16  target 7.0e-16  pos 1.4e-09  vel 4.1e-09  acc 1.7e-08"""
    c = pc.CASES[case]
    assert c["dt_mpc"] != 0.02 and pc.rows_needed(case) <= c["N_gait"] and c["N"] + 1 <= c["N_gait"]
    ref = pc.oracle_run(oracle_mod, case)
    assert (ref["gait"].any(-1).sum(-1) == c["N"]).all()  # the current gait keeps n_steps live rows through every change
    run_against_the_oracle(oracle_mod, case)
