#!/usr/bin/env python3
"""The planner tests' tolerances as measured (no GPU): the oracle held against itself, with each input moved by one ulp, over the
sequences of tests/planner_cases.py.  Prints, per case and output, the spread and the bound (100 x) in the form of the SPREAD
record there, then what each geometry parameter changed alone does to the oracle's outputs, in bounds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import oracle  # noqa: E402
import planner_cases as pc  # noqa: E402

oracle.build()
measured = {}
for case in pc.CASES:
    measured[case] = pc.spread(oracle, case)
    K, B = pc.sequence(case)["code"].shape
    print('    "%s": dict(%s),  # %d iterations x %d robots' % (case, ", ".join("%s=%.2e" % (n, measured[case][n]) for n in pc.FLOAT_OUTPUTS), K, B))
for case in pc.CASES:
    print("%-14s bounds: %s" % (case, "  ".join("%s %.2e" % (n, 100 * measured[case][n]) for n in pc.FLOAT_OUTPUTS)))
for case in pc.ALONE + ("lock_long",):
    e = pc.effect(oracle, case)
    print("%-14s alone changes the oracle's outputs by (in bounds of that case): %s" % (case, "  ".join(
        "%s %.3g" % (n, e[n] / max(100 * measured[case]["target" if n == "ft_target" else n], 1e-300)) for n in e)))
