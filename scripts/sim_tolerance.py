#!/usr/bin/env python3
"""The simulator tests' tolerances as measured (no GPU): the numpy checker tests/sim_numpy.py held against itself on the states
of tests/test_gpu_sim.py.  Prints the spreads behind FD_SPREAD / TICK_SPREAD there, the smallest |d| of the checker's free run
of the teacher-forced case (the contact law switches at d = 0) and the numbers of feet in contact that run sees."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import sim_numpy as sn  # noqa: E402
import test_gpu_sim as t  # noqa: E402

solve, ulp = t.fd_spread(sn, t._fd_states(sn))
print("forward dynamics: float64 vs longdouble solve %.3g, inputs moved by one ulp %.3g (FD_SPREAD %.3g, FD_BOUND %.3g)"
      % (solve, ulp, t.FD_SPREAD, t.FD_BOUND))
spread, smallest, seen = t.tick_spread(sn)
print("one tick: state moved by one ulp %.3g (TICK_SPREAD %.3g, TICK_BOUND %.3g); smallest |d| %.3g; feet in contact seen %s"
      % (spread, t.TICK_SPREAD, t.TICK_BOUND, smallest, sorted(seen)))
