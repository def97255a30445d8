#!/usr/bin/env python3
"""The whole-loop tests' tolerances as measured (no GPU): the chained checkers of tests/loop_chain.py free-run every variant of
tests/loop_cases.py, the simulator and the estimator checkers repeating every tick from inputs moved up by one ulp.  Prints the
LOOP_TICK_SPREAD record in the form it has there, the bounds (100 x), and per robot the tick and margin of its flag."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import oracle  # noqa: E402

oracle.build()
import loop_cases as lc  # noqa: E402

for variant in lc.VARIANTS:
    cs = lc.free_run(variant, measure_spread=True)
    m, f, a = lc.measured(cs), lc.fleet(variant), lc.arrays(cs)
    print('    "%s": dict(sim=%.3g, est=%.3g, min_abs_d=%.3g),' % (variant, m["sim"], m["est"], m["min_abs_d"]))
    print("        bounds: simulator %.3g, estimator (only where the existing tolerances do not hold) %.3g; recorded %s"
          % (100 * m["sim"], 100 * m["est"], lc.LOOP_TICK_SPREAD[variant]))
    for b, c in enumerate(cs):
        got = lc.check_margins(f["names"][b], a["flags"][:, b], [t["ratios"] for t in c.trace])
        print("        %-22s %s; feet in contact seen %s; simulator spread %.3g" % (
            f["names"][b], "walks" if got is None else "flag %d at tick %d (%.4f -> %.4f of its limit)" % (got[1], got[0], got[2], got[3]),
            sorted({t["feet"] for t in c.trace}), c.spread["sim"]))
