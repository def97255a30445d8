"""The whole-body step split at its box-QP: what a set of WBC outputs must satisfy whichever path the ADMM iteration took, the
input families the WBC tests run, and the tolerances.  tests/test_gpu_wbc.py, tests/test_wbc_recompose_cpu.py and
scripts/wbc_tolerance.py read this module.  No GPU is touched here; only the oracle's free functions (fixed_feet, InvKin, rnea,
crba, feet_jacobians) and, for the distance to the optimum, its OSQP restatement at tight tolerances are used.

scripts/QP_WBC.py:52-131 is three things in a row.
  * Before the QP, and independent of it: the inverse kinematics give q_step, dq_cmd, ddq_cmd; qdes[7:] = q[7:] + q_step,
    vdes[6:] = dq_cmd, feet = (posf', pgoals - posf', vf'); qdes[:7] and vdes[:6] are zero.  Compared directly.
  * The QP: min 1/2 x'Hx + g'x, lo <= G x <= lo + 25, x = f - f_cmd, H = 0.1 A'A + 5 I strictly convex: ONE optimum x*, whatever
    rho, warm start or rounding did on the way.  The candidate's f_with_delta is held to x* by its distance in N and by the
    worst violation of 0 <= G f <= 25 (`optimum`).
  * After the QP, as functions of the f that came out (Jc with its swing rows zeroed, Y the diagonal of the neutral-pose CRBA
    base block):  ddq_res* = Y^-1 (Jc[:, :6]' f - rnea(q, dq, ddq_cmd)[:6]),
                  tau*     = rnea(q, dq, ddq_cmd + [ddq_res; 0])[6:] - Jc[:, 6:]' f     with the candidate's own f and ddq_res.
    A candidate that assembled its own f correctly meets both to rounding, a rounding-sensitive robot included.

Tolerances.  A residual is |candidate - recomposed|, componentwise, in the output's own unit (rad, rad/s, m and m/s, rad/s^2 and
m/s^2, N m).  Its bound is 100 x the spread (the project's convention): the largest change of the recomposed quantity when every
non-zero floating-point input (q, dq, pgoals, vgoals, agoals) moves by one ulp in a seeded random direction while f and ddq_res
stay fixed, over the family's robot-calls and at least SPREAD_SAMPLES draws (exact zeros stay, the contact flags stay: they
select branches).  spread() measures
it, scripts/wbc_tolerance.py prints it, SPREAD below records it and tests/test_wbc_recompose_cpu.py holds the record against the
measurement.  The distance to the optimum is bounded by the reference, never by the kernel: 2 x the largest distance the strict
oracle shows over the same run (one 25-iteration termination check earlier or later), computed by the test that uses it; the
same again over the swing feet alone, which is never the looser of the two."""
import numpy as np

MU = 0.9  # include/qrw/QPWBC.hpp:30
NZ_MAX = 25.0  # src/QPWBC.cpp:337
OUTPUTS = ("qdes", "vdes", "feet", "ddq_res", "tau_ff")
INPUT_KEYS = ("q", "dq", "f_cmd", "contacts", "pgoals", "vgoals", "agoals")
MOVED = ("q", "dq", "pgoals", "vgoals", "agoals")


def G_matrix(mu=MU):
    sc = np.array([[-1, 0, mu], [1, 0, mu], [0, -1, mu], [0, 1, mu], [0, 0, 1.0]])  # src/QPWBC.cpp:10-16
    G = np.zeros((20, 12))
    for i in range(4):
        G[5 * i:5 * i + 5, 3 * i:3 * i + 3] = sc
    return G


_G = G_matrix()
_Y = {}


def base_inertia_diag(oracle_mod):
    """Y: the diagonal of crba's base block at the neutral configuration (scripts/QP_WBC.py:89-93)."""
    if "Y" not in _Y:
        qn = np.zeros(19)
        qn[6] = 1.0
        _Y["Y"] = np.diag(oracle_mod.crba(qn))[:6].copy()
    return _Y["Y"]


def robot(d, b):
    """One robot's inputs out of a batch dict."""
    return {k: np.asarray(d[k][b], dtype=np.float64) for k in INPUT_KEYS}


def candidate(o, b):
    """One robot's outputs out of a batch dict (wbc_compute_host's layout)."""
    return {k: np.asarray(o[k][b], dtype=np.float64).reshape(s) for k, s in
            (("tau_ff", 12), ("qdes", 19), ("vdes", 18), ("f_with_delta", 12), ("ddq_res", 6), ("feet", (3, 3, 4)))}


def oracle_candidate(ctl):
    """The outputs of an oracle.WbcController after compute(), in the same layout."""
    return dict(tau_ff=ctl.tau_ff.copy(), qdes=ctl.qdes.copy(), vdes=ctl.vdes[:, 0].copy(), f_with_delta=ctl.f_with_delta[:, 0].copy(),
                ddq_res=ctl.ddq_res.copy(), feet=np.stack(ctl.feet()))


def pre_qp(oracle_mod, inp):
    """Everything before the QP, from the oracle's pieces: qdes, vdes, feet as the step returns them, ddq_cmd (18), the masked Jc
    (12, 18) and rnea(q, dq, ddq_cmd)[:6]."""
    q, dq, contacts = inp["q"], inp["dq"], inp["contacts"]
    posf, vf, wf, af, Jf = oracle_mod.fixed_feet(q[7:], dq[6:])
    ik = oracle_mod.InvKin(0.002)  # (its time step is stored and never read, src/InvKin.cpp:6)
    ddq_cmd = np.zeros(18)
    ddq_cmd[6:] = ik.refreshAndCompute(contacts, inp["pgoals"], inp["vgoals"], inp["agoals"], posf, vf, wf, af, Jf)
    qdes, vdes = np.zeros(19), np.zeros(18)
    qdes[7:] = q[7:] + ik.get_q_step()
    vdes[6:] = ik.get_dq_cmd()
    feet = np.stack([posf.T, inp["pgoals"] - posf.T, vf.T])
    Jc = oracle_mod.feet_jacobians(q)
    for i in range(4):
        if contacts[i] == 0.0:
            Jc[3 * i:3 * i + 3] = 0.0
    return dict(qdes=qdes, vdes=vdes, feet=feet, ddq_cmd=ddq_cmd, Jc=Jc, rnea6=oracle_mod.rnea(q, dq, ddq_cmd)[:6])


def post_qp(oracle_mod, inp, pre, f, ddq_res):
    """(ddq_res*, tau*) at the given f and ddq_res."""
    Y = base_inertia_diag(oracle_mod)
    ddq_star = (pre["Jc"][:, :6].T @ f - pre["rnea6"]) / Y
    ddq = pre["ddq_cmd"].copy()
    ddq[:6] += ddq_res
    tau_star = oracle_mod.rnea(inp["q"], inp["dq"], ddq)[6:] - pre["Jc"][:, 6:].T @ f
    return ddq_star, tau_star


def qp_data(oracle_mod, inp, pre):
    """H, g, lo of the box-QP in numpy (src/QPWBC.cpp:395-470, as tests/test_oracle_wbc.py builds them)."""
    Y = base_inertia_diag(oracle_mod)
    X = pre["Jc"][:, :6].T
    A = X / Y[:, None]
    gamma = (X @ inp["f_cmd"] - pre["rnea6"]) / Y
    return 0.1 * A.T @ A + 5.0 * np.eye(12), 0.1 * A.T @ gamma, -_G @ inp["f_cmd"], A, gamma


def optimum(oracle_mod, inp, pre):
    """(x*, solved): the QP's one optimum from the oracle's OSQP at eps 1e-12."""
    import scipy.sparse as sp

    H, g, lo, _, _ = qp_data(oracle_mod, inp, pre)
    qp = oracle_mod.OSQP(sp.csc_matrix(np.triu(H)), g, sp.csc_matrix(_G), lo, lo + NZ_MAX, eps_abs=1e-12, eps_rel=1e-12, max_iter=200000)
    x, _ = qp.solve()
    return x, qp.info()["status"] == 1


def recompose(oracle_mod, inp, cand, with_optimum=True, xstar=None):
    """Componentwise residuals of one robot's candidate outputs: dict(qdes (19), vdes (18), feet (3, 3, 4), ddq_res (6), tau_ff (12))
    and, with_optimum, opt_dist = max |f_with_delta - f_cmd - x*| in N, opt_dist_swing = the same over the swing feet alone, bound_viol = the worst violation of 0 <= G f <= 25 in N,
    solved (the tight solve reported status 1) and xstar (12).  xstar: the optimum of these inputs if it is known already (it
    depends on the inputs alone: a second candidate for the same inputs need not solve again)."""
    pre = pre_qp(oracle_mod, inp)
    f = cand["f_with_delta"]
    ddq_star, tau_star = post_qp(oracle_mod, inp, pre, f, cand["ddq_res"])
    res = dict(qdes=cand["qdes"] - pre["qdes"], vdes=cand["vdes"] - pre["vdes"], feet=cand["feet"] - pre["feet"],
               ddq_res=cand["ddq_res"] - ddq_star, tau_ff=cand["tau_ff"] - tau_star)
    if with_optimum:
        x, solved = (xstar, True) if xstar is not None else optimum(oracle_mod, inp, pre)
        Gf = _G @ f
        dist = np.abs(f - inp["f_cmd"] - x).max()
        swing = np.repeat(inp["contacts"] == 0.0, 3)
        dsw = np.abs(f - inp["f_cmd"] - x)[swing].max() if swing.any() else 0.0
        res.update(opt_dist=float(dist) if np.isfinite(dist) else np.inf, opt_dist_swing=float(dsw) if np.isfinite(dsw) else np.inf,
                   solved=solved, xstar=x,
                   bound_viol=float(max(0.0, (-Gf).max(), (Gf - NZ_MAX).max())) if np.isfinite(Gf).all() else np.inf)
    return res


def worst(res):
    """{output: max |residual|} of one recompose() result (a non-finite residual counts as infinite)."""
    out = {}
    for k in OUTPUTS:
        r = np.abs(res[k])
        out[k] = float(r.max()) if np.isfinite(r).all() else np.inf
    return out


def batch_worst(oracle_mod, d, o, with_optimum=True, xstar=None):
    """recompose() over a batch: {output: (B,) max |residual|} and, with_optimum, opt_dist / bound_viol / solved as (B,) and xstar
    (B, 12).  xstar: the optima of an earlier call on the same inputs (every one of them solved)."""
    B = len(d["q"])
    out = {k: np.zeros(B) for k in OUTPUTS + (("opt_dist", "opt_dist_swing", "bound_viol", "solved") if with_optimum else ())}
    if with_optimum:
        out["xstar"] = np.zeros((B, 12))
    for b in range(B):
        r = recompose(oracle_mod, robot(d, b), candidate(o, b), with_optimum, None if xstar is None else xstar[b])
        for k, v in worst(r).items():
            out[k][b] = v
        if with_optimum:
            for k in ("opt_dist", "opt_dist_swing", "bound_viol", "solved", "xstar"):
                out[k][b] = r[k]
    return out


def check_optimum(got, ref, where=()):
    """The pooled bound on the distance to the optimum: got, ref = lists (one entry per call of a run) of batch_worst() results of
    the candidate and of the strict oracle on the same inputs.  Every tight solve solved; every candidate robot-call within
    2 x the oracle's largest distance over the run, its violation of the QP's bounds likewise; the swing feet are pooled a second
    time among themselves (their block of the QP is 5 I alone and separates from the rest: the oracle is closer to the optimum
    there, and the bound over all feet could not see a force on a swing foot below it).  Returns (the candidate's largest
    distance, the oracle's, the candidate's largest bound violation)."""
    assert all(x["solved"].all() for x in ref), where
    ref_max = max(float(x["opt_dist"].max()) for x in ref)
    limit = 2.0 * ref_max
    got_max = max(float(x["opt_dist"].max()) for x in got)
    viol = max(float(x["bound_viol"].max()) for x in got)
    swing_limit = 2.0 * max(float(x["opt_dist_swing"].max()) for x in ref)
    for c, x in enumerate(got):
        assert (x["opt_dist"] <= limit).all(), (c, int(np.argmax(x["opt_dist"])), float(x["opt_dist"].max()), limit) + tuple(where)
        assert (x["opt_dist_swing"] <= swing_limit).all(), (c, int(np.argmax(x["opt_dist_swing"])), float(x["opt_dist_swing"].max()), swing_limit) + tuple(where)
        assert (x["bound_viol"] <= limit).all(), (c, int(np.argmax(x["bound_viol"])), float(x["bound_viol"].max()), limit) + tuple(where)
    return got_max, ref_max, viol


def bound(family, name):
    return 100.0 * SPREAD[family][name]


def check(family, w, where=()):
    """Assert a batch_worst() / worst() result against the family's bounds; returns {output: the largest residual}."""
    big = {k: float(np.max(w[k])) for k in OUTPUTS}
    for k in OUTPUTS:
        assert big[k] <= bound(family, k), (family, k, big[k], bound(family, k), int(np.argmax(w[k]))) + tuple(where)
    return big


# ------------------------------------------------------------------------------------------------ the input families
def f_cmd_for(contacts, rng=None):
    B = contacts.shape[0]
    f = np.zeros((B, 12))
    f[:, 2::3] = contacts * 24.5 / np.maximum(contacts.sum(1, keepdims=True), 1)
    f[:, 0::3] = contacts * 0.7
    f[:, 1::3] = contacts * -0.4
    if rng is not None:
        f += np.repeat(contacts, 3, axis=1) * rng.normal(size=(B, 12))
    return f


def all_contact_sets(B, s):
    return np.array([[(((b + 5 * s) % 16) >> i) & 1 for i in range(4)] for b in range(B)], dtype=np.float64)


def _frozen(dicts):
    """The arrays of a shared result made read-only: a test that wrote into one would change what every later test reads."""
    for d in dicts:
        for v in d.values():
            v.setflags(write=False)
    return dicts


WILD_SEEDS = {16: 20700016, 4: 20700004}  # test_wbc_on_wild_inputs_matches_oracle: seed0 = 20700000 + lanes
_family_cache = {}


def family(name, synth_mod, oracle_mod=None):
    """The calls of an input family, each a dict of (B, ...) arrays with INPUT_KEYS: "sequence" (test_wbc_sequence_matches_oracle:
    B = 21, eight calls, random base poses from the fifth), "patterns" (test_contact_patterns_from_flight_to_full_stance: B = 16, four
    calls, every contact set), "wild16" / "wild4" (test_wbc_on_wild_inputs_matches_oracle: B = 144, ten calls) and "dropin"
    (test_dropin_classes_match_oracle: one robot, five calls, the forces of the oracle's MPC; needs oracle_mod).  Computed once and
    shared: the arrays are read-only."""
    if name in _family_cache:
        return _family_cache[name]
    calls = []
    if name == "sequence":
        B = 21  # not a multiple of 16: exercises the padded quads of the last wavefront
        sb = synth_mod.SyntheticBatch(B, 16, gaits=("trot", "walk", "static"), seed0=91000)
        rng = np.random.default_rng(0)
        for s in range(8):
            d = sb.step(s)
            # random base pose / twist: the reference always passes the identity pose, the kernel must not assume it
            quat = rng.normal(size=(B, 4))
            d["q"][:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True) if s >= 4 else d["q"][:, 3:7]
            d["q"][:, :3] += rng.uniform(-0.2, 0.2, (B, 3)) if s >= 4 else 0
            d["dq"][:, 3:6] = rng.uniform(-0.5, 0.5, (B, 3))
            d["f_cmd"] = f_cmd_for(d["contacts"], rng)
            calls.append({k: np.array(d[k], dtype=np.float64) for k in INPUT_KEYS})
    elif name == "patterns":
        B = 16
        sb = synth_mod.SyntheticBatch(B, 16, gaits=("trot",), seed0=93000)
        rng = np.random.default_rng(5)
        for s in range(4):
            d = sb.step(s)
            d["contacts"] = all_contact_sets(B, s)
            d["f_cmd"] = f_cmd_for(d["contacts"], rng)
            calls.append({k: np.array(d[k], dtype=np.float64) for k in INPUT_KEYS})
    elif name in ("wild16", "wild4"):
        gen = synth_mod.RandomWbcInputs(144, seed0=WILD_SEEDS[int(name[4:])])
        calls = [gen.step(c) for c in range(10)]
    elif name == "dropin":
        N = 16
        sb = synth_mod.SyntheticBatch(1, N, seed0=95000)
        mpc = oracle_mod.MPC(0.02, N, 0.32, 20)
        x0 = None
        for s in range(5):
            d = sb.step(s, x0)
            mpc.run(10 * s, d["xref"][0], d["fsteps"][0])
            r = mpc.get_latest_result()
            x0 = r[:12, 0][None]
            d["f_cmd"] = r[12:, 0][None].copy()
            calls.append({k: np.array(d[k], dtype=np.float64) for k in INPUT_KEYS})
    else:
        raise KeyError(name)
    _family_cache[name] = _frozen(calls)
    return calls


FAMILIES = ("sequence", "patterns", "wild16", "wild4", "dropin")
_oracle_cache = {}


def oracle_run(oracle_mod, synth_mod, name):
    """The strict oracle over a family, warm-started from call to call: a list (per call) of output batch dicts in
    wbc_compute_host's layout plus "iters" (B,) and "k_since_contact" (B, 4).  Computed once and shared: the arrays are read-only."""
    if name in _oracle_cache:
        return _oracle_cache[name]
    calls = family(name, synth_mod, oracle_mod)
    B = len(calls[0]["q"])
    ctl = [oracle_mod.WbcController(0.002) for _ in range(B)]
    outs = []
    for d in calls:
        o = dict(tau_ff=np.zeros((B, 12)), qdes=np.zeros((B, 19)), vdes=np.zeros((B, 18)), f_with_delta=np.zeros((B, 12)),
                 ddq_res=np.zeros((B, 6)), feet=np.zeros((B, 3, 3, 4)), iters=np.zeros(B, np.int32), k_since_contact=np.zeros((B, 4)))
        for b, c in enumerate(ctl):
            assert c.compute(*[d[k][b] for k in INPUT_KEYS]) == 0
            for k, v in oracle_candidate(c).items():
                o[k][b] = v
            o["iters"][b], o["k_since_contact"][b] = c.qp_iter, c.k_since_contact.ravel()
        outs.append(o)
    _oracle_cache[name] = _frozen(outs)
    return outs


_analysis_cache = {}


def oracle_analysis(oracle_mod, synth_mod, name):
    """(batch_worst() of the strict oracle's own outputs per call, the family's limit on the distance to the optimum = 2 x the
    largest of them); computed once and shared, read-only."""
    if name not in _analysis_cache:
        calls, outs = family(name, synth_mod, oracle_mod), oracle_run(oracle_mod, synth_mod, name)
        w = [batch_worst(oracle_mod, d, o) for d, o in zip(calls, outs)]
        _analysis_cache[name] = (_frozen(w), 2.0 * max(float(x["opt_dist"].max()) for x in w))
    return _analysis_cache[name]


SPREAD_SAMPLES = 160  # a family with fewer robot-calls draws several directions per robot-call, so that its largest change is
# taken over at least as many samples as the smallest batched family's (8 x 21): a maximum over five samples would be a bound
# set by luck


def _one_ulp(x, rng):
    up = rng.random(x.shape) < 0.5
    return np.where(x != 0.0, np.nextafter(x, np.where(up, np.inf, -np.inf)), x)


def spread(oracle_mod, synth_mod, name, seed=2028):
    """{output: the largest change of the recomposed quantity over the family when every non-zero element of q, dq, pgoals, vgoals,
    agoals moves by one ulp in a seeded random direction}, f and ddq_res held at the oracle's."""
    calls, outs = family(name, synth_mod, oracle_mod), oracle_run(oracle_mod, synth_mod, name)
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    s = dict.fromkeys(OUTPUTS, 0.0)
    draws = max(1, -(-SPREAD_SAMPLES // (len(calls) * len(calls[0]["q"]))))
    for d, o in zip(calls, outs):
        for b in range(len(d["q"])):
            inp = robot(d, b)
            f, dd = o["f_with_delta"][b], o["ddq_res"][b]
            p0 = pre_qp(oracle_mod, inp)
            a0 = post_qp(oracle_mod, inp, p0, f, dd)
            for _ in range(draws):
                moved = dict(inp, **{k: _one_ulp(inp[k], rng) for k in MOVED})
                p1 = pre_qp(oracle_mod, moved)
                a1 = post_qp(oracle_mod, moved, p1, f, dd)
                for k, x, y in (("qdes", p0["qdes"], p1["qdes"]), ("vdes", p0["vdes"], p1["vdes"]), ("feet", p0["feet"], p1["feet"]),
                                ("ddq_res", a0[0], a1[0]), ("tau_ff", a0[1], a1[1])):
                    s[k] = max(s[k], float(np.abs(x - y).max()))
    return s


# ---- the record: spread() of every family as scripts/wbc_tolerance.py printed it (bound = 100 x), in rad, rad/s, m | m/s,
# rad/s^2 | m/s^2 and N m
SPREAD = {
    "sequence": dict(qdes=1.55e-15, vdes=5.55e-16, feet=2.22e-16, ddq_res=5.68e-14, tau_ff=2.00e-15),  # 8 calls x 21 robots
    "patterns": dict(qdes=1.55e-15, vdes=6.66e-16, feet=1.67e-16, ddq_res=2.84e-14, tau_ff=2.11e-15),  # 4 calls x 16 robots
    "wild16": dict(qdes=2.44e-15, vdes=1.07e-14, feet=1.33e-15, ddq_res=1.99e-13, tau_ff=6.22e-15),  # 10 calls x 144 robots
    "wild4": dict(qdes=2.66e-15, vdes=1.33e-14, feet=1.33e-15, ddq_res=2.27e-13, tau_ff=5.77e-15),  # 10 calls x 144 robots
    "dropin": dict(qdes=1.33e-15, vdes=6.66e-16, feet=1.39e-16, ddq_res=4.00e-14, tau_ff=2.16e-15),  # 5 calls x 1 robots
}
