"""tests/wbc_recompose.py held against itself on the CPU: the recorded spreads are the measured ones, the oracle's own outputs pass
the helper within the bounds on every input family, and the helper rejects outputs that are wrong in the ways the relative 1e-4 of
the GPU tests could not see."""
import numpy as np
import pytest

import wbc_recompose as wr


@pytest.mark.parametrize("name", wr.FAMILIES)
def test_recorded_spreads_are_the_measured_ones(oracle_mod, synth_mod, name):
    """wbc_recompose.SPREAD[name] is spread() of the family (scripts/wbc_tolerance.py prints the record); libm differences between
    machines stay far below the factor 2 allowed here.  The bounds are 100 x these figures."""
    measured = wr.spread(oracle_mod, synth_mod, name)
    print(name, "  ".join("%s %.2e" % (k, measured[k]) for k in wr.OUTPUTS))
    for k in wr.OUTPUTS:
        rec = wr.SPREAD[name][k]
        assert 0.5 * rec <= measured[k] <= 2.0 * rec, (name, k, measured[k], rec)
        assert wr.bound(name, k) == pytest.approx(100.0 * rec)
    # spreads of a double-precision computation on quantities of size 1 ... 100, not slack: a few ulps to a few thousand
    assert all(5e-17 < v < 1e-12 for v in wr.SPREAD[name].values())


def analysis(oracle_mod, synth_mod, name):
    """(the oracle's own batch_worst() per call, (the limit on the distance to the optimum, the limit over the swing feet alone))."""
    w, limit = wr.oracle_analysis(oracle_mod, synth_mod, name)
    return w, (limit, 2.0 * max(float(x["opt_dist_swing"].max()) for x in w))


def rejected(name, w, limit):
    """(B,) bool: the robot's outputs miss a recomposition bound, the distance to the optimum, the QP's bounds or the tight solve."""
    bad = np.zeros(len(w["tau_ff"]), bool)
    for k in wr.OUTPUTS:
        bad |= ~(w[k] <= wr.bound(name, k))
    if "opt_dist" in w:
        limit, swing_limit = limit
        bad |= ~(w["opt_dist"] <= limit) | ~(w["opt_dist_swing"] <= swing_limit) | ~(w["bound_viol"] <= limit) | (w["solved"] == 0)
    return bad


@pytest.mark.parametrize("name", wr.FAMILIES)
def test_oracle_outputs_pass_the_helper(oracle_mod, synth_mod, name):
    """The strict oracle over the family: every residual within its bound (measured: below 1 % of it -- the identities hold to
    a few ulps, 1.8e-15 N m on torques of 5.9 N m on the wild inputs), every tight solve solved, and the figures behind the pooled
    bound on the distance to the optimum as DESIGN.md 2 quotes them for the wild inputs (largest 6.4e-4 N, median 1.5e-5 N)."""
    w, limit = analysis(oracle_mod, synth_mod, name)
    for c, x in enumerate(w):
        wr.check(name, x, (c,))
        assert x["solved"].all(), (name, c)
        assert not rejected(name, x, limit).any()
    dist = np.concatenate([x["opt_dist"] for x in w])
    viol = max(x["bound_viol"].max() for x in w)
    print("%s: residuals in bounds %s; distance to the optimum max %.2e median %.2e N, bound violation %.2e N"
          % (name, "  ".join("%s %.3g" % (k, max(x[k].max() for x in w) / wr.bound(name, k)) for k in wr.OUTPUTS), dist.max(),
             np.median(dist), viol))
    assert viol <= limit[0] and limit[1] <= limit[0] and dist.max() < 1e-3  # inside the QP's own tolerances (eps 1e-5 on rows of size <= 25)
    if name.startswith("wild"):
        assert 3e-4 < dist.max() < 1.3e-3 and 5e-6 < np.median(dist) < 5e-5


def _mutation_calls(name, calls):
    return range(len(calls)) if len(calls[0]["q"]) < 100 else (0, len(calls) - 1)  # two of the ten wild calls: 288 robot-calls


@pytest.mark.parametrize("name", wr.FAMILIES)
def test_helper_rejects_a_wrong_torque_and_a_wrong_base_acceleration(oracle_mod, synth_mod, name):
    """One torque moved by ten bounds (6e-12 N m on the wild inputs); ddq_res[5] without its gamma (A (f - f_cmd) alone): rejected
    on every robot-call (the second wherever gamma[5] itself is above ten bounds: all but a few)."""
    calls, outs = wr.family(name, synth_mod, oracle_mod), wr.oracle_run(oracle_mod, synth_mod, name)
    n = n_gamma = 0
    for c in _mutation_calls(name, calls):
        d, o = calls[c], outs[c]
        B = len(d["q"])
        m = {k: v.copy() for k, v in o.items()}
        m["tau_ff"][np.arange(B), (np.arange(B) * 5 + c) % 12] += 10.0 * wr.bound(name, "tau_ff") * np.where(np.arange(B) % 2, 1, -1)
        assert rejected(name, wr.batch_worst(oracle_mod, d, m, False), np.inf).all(), (name, c)
        m = {k: v.copy() for k, v in o.items()}
        gamma5 = np.zeros(B)
        for b in range(B):
            inp = wr.robot(d, b)
            _, _, _, A, gamma = wr.qp_data(oracle_mod, inp, wr.pre_qp(oracle_mod, inp))
            m["ddq_res"][b, 5] = (A @ (o["f_with_delta"][b] - d["f_cmd"][b]))[5]
            gamma5[b] = gamma[5]
        big = np.abs(gamma5) > 10.0 * wr.bound(name, "ddq_res")
        assert rejected(name, wr.batch_worst(oracle_mod, d, m, False), np.inf)[big].all(), (name, c)
        n, n_gamma = n + B, n_gamma + int(big.sum())
    assert n_gamma >= 0.9 * n, (name, n_gamma, n)


@pytest.mark.parametrize("name", wr.FAMILIES)
def test_helper_rejects_wrong_forces(oracle_mod, synth_mod, name):
    """f_z of one swing foot set to 1e-3 N, and f projected onto the friction cone of mu = 0.8.  The first moves neither ddq_res*
    nor tau* (a swing foot's rows of Jc are zero): it is for the distance to the optimum alone.  The limit on that distance
    pooled over all feet (2 x the strict oracle's largest) is 1.3e-3 N on the wild inputs and could not see it; pooled over the
    swing feet alone it is 6.4e-4 N there (3.3e-4, 4.8e-5 and 7.7e-9 N on the periodic families), and 1e-3 N on a swing foot is
    rejected on EVERY robot-call that has one, on every family.  The projection is rejected wherever it moves f by more than
    2 x the limit: more than half of the wild robot-calls, a few of the periodic ones (most of their forces lie inside the
    narrower cone already)."""
    calls, outs = wr.family(name, synth_mod, oracle_mod), wr.oracle_run(oracle_mod, synth_mod, name)
    _, limit = analysis(oracle_mod, synth_mod, name)
    n_swing = n_swing_rejected = n_proj = 0
    for c in _mutation_calls(name, calls):
        d, o = calls[c], outs[c]
        B = len(d["q"])
        m = {k: v.copy() for k, v in o.items()}
        has = np.zeros(B, bool)
        for b in range(B):
            sw = np.nonzero(d["contacts"][b] == 0)[0]
            if len(sw):
                m["f_with_delta"][b, 3 * sw[(b + c) % len(sw)] + 2] = 1e-3
                has[b] = True
        rej = rejected(name, wr.batch_worst(oracle_mod, d, m), limit)
        assert not rej[~has].any()
        n_swing, n_swing_rejected = n_swing + int(has.sum()), n_swing_rejected + int(rej[has].sum())
        assert rej[has].all(), (name, c)
        m = {k: v.copy() for k, v in o.items()}
        f = m["f_with_delta"].reshape(B, 4, 3)
        cap = 0.8 * np.maximum(f[:, :, 2:3], 0.0)
        f[:, :, :2] = np.clip(f[:, :, :2], -cap, cap)
        moved = np.abs(m["f_with_delta"] - o["f_with_delta"]).max(1) > 2.0 * limit[0]
        rej = rejected(name, wr.batch_worst(oracle_mod, d, m), limit)
        assert rej[moved].all(), (name, c)
        n_proj += int(moved.sum())
    print("%s: limits %.2e N, swing feet %.2e N; 1e-3 N on a swing foot rejected on %d of %d robot-calls; projection onto mu = 0.8 rejected on %d"
          % (name, limit[0], limit[1], n_swing_rejected, n_swing, n_proj))
    assert n_swing_rejected == n_swing and 1e-3 > 1.5 * limit[1]
    if name.startswith("wild"):
        assert n_proj >= 60 and n_swing >= 200
    elif name != "dropin":
        assert n_swing >= 20
