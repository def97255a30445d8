#!/usr/bin/env python3
"""The Kalman estimator tests' tolerance as measured (no GPU): the dense numpy checker tests/estimator_kalman_numpy.py held
against itself on the input sequences of tests/test_gpu_estimator_kalman.py, in the three variants that bound what a correct
implementation may differ by:
  (a) every sensor input (acceleration, gyro, quaternion, joint angles and velocities) moved by one ulp;
  (b) np.linalg.solve instead of np.linalg.inv in the correction;
  (c) the arrangement csrc/kalman_filter.h uses: three per-axis 6-state filters, the measurement rows taken one at a time.
Measure: |a - b| / max(1, |a|) over q_filt, v_filt and X, P scaled by its own largest entry; the worst over all ticks and
robots.  KALMAN_BOUND in the tests is 100 x the largest of the three.  Also checked on the way, over every tick of every
sequence: the cross-axis entries of the dense P are exactly 0.0 and P's asymmetry stays below 1e-12 of its largest entry."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import oracle  # noqa: E402
import synth  # noqa: E402

oracle.build()
import estimator_kalman_numpy as ekn  # noqa: E402
import test_gpu_estimator_kalman as t  # noqa: E402


def moved_by_one_ulp(tick):
    return dict(tick, sensors={k: np.nextafter(v, np.inf) for k, v in tick["sensors"].items()})


def cross_axis_mask():
    axis = np.arange(18) % 3  # state s belongs to axis s % 3 (position, velocity, and 6 + 3 i + j)
    return axis[:, None] != axis[None, :]


def measure():
    variants = {"a: inputs moved by one ulp": dict(), "b: solve instead of inv": dict(solve=True),
                "c: per-axis blocks, sequential scalar updates": dict(filter_class=ekn.AxisFilter)}
    worst = {v: 0.0 for v in variants}
    where = {v: None for v in variants}
    cross, asym, by_sequence = cross_axis_mask(), 0.0, {}
    for name, B, options, seq in t.sequences(oracle, synth):
        mk = lambda **kw: [ekn.Estimator(options.get("dt", t.DT), t.H_INIT, options.get("perfect", False), kalman=options.get("kalman", True), **kw)
                           for _ in range(B)]
        base, others = mk(), {v: mk(**kw) for v, kw in variants.items()}
        for k, tick in enumerate(seq):
            for b in range(B):
                t.checker_step(base[b], tick, b)
                P = base[b].P
                assert not P[cross].any(), ("cross-axis entries of P are not exactly zero", name, k, b)
                asym = max(asym, np.abs(P - P.T).max() / np.abs(P).max())
                for v, refs in others.items():
                    t.checker_step(refs[b], moved_by_one_ulp(tick) if v.startswith("a") else tick, b)
                    e = max(t.kalman_err(refs[b].q_filt, base[b].q_filt), t.kalman_err(refs[b].v_filt, base[b].v_filt),
                            t.kalman_err(refs[b].X, base[b].X), t.covariance_err(refs[b].P, P))
                    by_sequence[name] = max(by_sequence.get(name, 0.0), e)
                    if e > worst[v]:
                        worst[v], where[v] = e, (name, k, b)
    return worst, where, asym, by_sequence


if __name__ == "__main__":
    worst, where, asym, by_sequence = measure()
    for v, e in worst.items():
        print("(%s) %.3g at (sequence, tick, robot) %s" % (v, e, where[v]))
    print("largest %.3g -> bound 100 x = %.3g (KALMAN_BOUND in the tests: %.3g)" % (max(worst.values()), 100 * max(worst.values()),
                                                                                     t.KALMAN_BOUND))
    print("largest of the three by sequence: %s" % ", ".join("%s %.3g" % item for item in by_sequence.items()))
    print("cross-axis entries of P exactly 0.0 on every tick; largest asymmetry of P %.3g of its largest entry" % asym)
