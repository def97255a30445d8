#!/usr/bin/env python3
"""The WBC recomposition tests' tolerances as measured (no GPU): over every input family of tests/wbc_recompose.py, the change of
each recomposed quantity (qdes, vdes, feet, ddq_res*, tau* with f held fixed) when every floating-point input moves by one ulp in
a seeded random direction.  Prints the spreads in the form of the SPREAD record there, the bounds (100 x), what the identities
leave on the oracle's own outputs, and the strict oracle's distance to the QP's optimum."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import oracle  # noqa: E402
import synth  # noqa: E402
import wbc_recompose as wr  # noqa: E402

oracle.build()
measured = {}
for name in wr.FAMILIES:
    measured[name] = wr.spread(oracle, synth, name)
    calls = wr.family(name, synth, oracle)
    print('    "%s": dict(%s),  # %d calls x %d robots' % (name, ", ".join("%s=%.2e" % (k, measured[name][k]) for k in wr.OUTPUTS),
                                                           len(calls), len(calls[0]["q"])))
for name in wr.FAMILIES:
    print("%-9s bounds: %s" % (name, "  ".join("%s %.2e" % (k, 100 * measured[name][k]) for k in wr.OUTPUTS)))
for name in wr.FAMILIES:
    calls, outs = wr.family(name, synth, oracle), wr.oracle_run(oracle, synth, name)
    w = [wr.batch_worst(oracle, d, o) for d, o in zip(calls, outs)]
    dist = np.concatenate([x["opt_dist"] for x in w])
    print("%-9s the oracle's own residuals (in bounds): %s; tight solves solved %d of %d; distance to the optimum max %.2e median %.2e "
          "99th percentile %.2e N, worst bound violation %.2e N"
          % (name, "  ".join("%s %.3g" % (k, max(x[k].max() for x in w) / max(100 * measured[name][k], 1e-300)) for k in wr.OUTPUTS),
             int(sum(x["solved"].sum() for x in w)), dist.size, dist.max(), np.median(dist), np.percentile(dist, 99),
             max(x["bound_viol"].max() for x in w)))
