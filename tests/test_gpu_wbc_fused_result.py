"""The safety check fused into both WBC kernels (qrw_wbc_compute_result: Controller result + security_check, scripts/Controller.py:306-310,
341-365) where it matters: codes 1, 2 and 3, their precedence, the strict `>` at the thresholds, code 4, stickiness, and isolation
between the robots of one wavefront.  wbc16_kernel runs one joint per lane and combines the flags over a 16-lane row, wbc_kernel
one leg per lane over a quad; the control loop runs these two copies, not glue::result (which test_glue_stages_match_oracle covers).

One table of cases (B = 37, six warm-started calls on wild WBC inputs), built and checked on the CPU first: no flag hinges on
rounding -- the oracle's largest |tau_ff| of a robot-call is below 7.9 N m or above 8.1 N m (the wild inputs stay below 6 N m, the
forces being capped at 25 N per foot; a robot meant to trip on torque gets its swing feet's acceleration goals scaled to
+-1500 m/s^2 on that call), and the joint and velocity thresholds are met exactly or missed by one ulp."""
import numpy as np
import pytest

import wbc_recompose as wr

B, K = 37, 6
Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])
Q_SEC = np.array([np.pi * 0.4, np.pi * 80 / 180, np.pi])  # scripts/Controller.py:181, per joint type
UP = np.inf

# robot: [(call, what, ...)]; "q": q_filt[7 + joint] = value, "v": v_secu[joint] = value, "tau": the torque trip, "nan": a NaN goal.
# The flag each robot must show after every call follows in EXPECT.
PLAN = {
    1: [(1, "q", 0, Q_SEC[0]), (3, "q", 0, np.nextafter(Q_SEC[0], UP))],                  # hip roll: at the limit, then one ulp over
    2: [(1, "q", 4, Q_SEC[1]), (2, "q", 4, np.nextafter(Q_SEC[1], UP))],                  # hip pitch
    3: [(0, "q", 8, Q_SEC[2]), (4, "q", 8, np.nextafter(Q_SEC[2], UP))],                  # knee
    4: [(2, "q", 3, -Q_SEC[0]), (3, "q", 3, -np.nextafter(Q_SEC[0], UP))],                # negative
    5: [(1, "v", 2, 50.0), (2, "v", 2, np.nextafter(50.0, UP))],
    6: [(0, "v", 7, -50.0), (1, "v", 7, -np.nextafter(50.0, UP))],                        # negative
    7: [(2, "tau",)],
    8: [(4, "tau",)],
    9: [(2, "q", 10, 1.4), (2, "v", 11, 51.0)],                                           # 1 + 2 -> 2
    10: [(3, "tau",), (3, "v", 0, -60.0)],                                                # 2 + 3 -> 3
    11: [(1, "tau",), (1, "q", 6, -1.3)],                                                 # 1 + 3 -> 3
    12: [(2, "nan",)],                                                                    # qdes not finite -> 4
    13: [(3, "nan",), (3, "q", 5, 3.2)],                                                  # 4 + 1 -> 1
    17: [(1, "v", 5, 70.0)],                                                              # 16, 18, 19 share its wbc16 wavefront
    22: [(0, "q", 1, -1.5)],                                                              # on the first call
    36: [(5, "q", 11, -3.15)],                                                            # alone in the padded last wavefront, last call
}
# (first call with the flag, the flag)
EXPECT = {1: (3, 1), 2: (2, 1), 3: (4, 1), 4: (3, 1), 5: (2, 2), 6: (1, 2), 7: (2, 3), 8: (4, 3), 9: (2, 2), 10: (3, 3), 11: (1, 3),
          12: (2, 4), 13: (3, 1), 17: (1, 2), 22: (0, 1), 36: (5, 1)}
SECURITY = np.concatenate([np.zeros(12), 0.1 * np.ones(12), np.zeros(36)]).reshape(5, 12)

_cases = {}


def cases(synth_mod, oracle_mod):
    """dict(calls, clean_calls: K lists of input dicts (clean: the torque and NaN robots left as drawn), q_filt, v_secu,
    clean_q_filt, clean_v_secu (K, B, ...), flags (K, B) expected after each call, tau_max (K, B) the oracle's largest |tau_ff| on
    `calls`)."""
    if _cases:
        return _cases
    gens = [synth_mod.RandomWbcInputs(1, seed0=20740000, b0=b) for b in range(B)]
    rng = np.random.default_rng(20740)
    clean_calls, q_filt, v_secu = [], np.zeros((K, B, 19)), np.zeros((K, B, 12))
    for c in range(K):
        ds = [g.step(c) for g in gens]
        clean_calls.append({k: np.concatenate([d[k] for d in ds]) for k in wr.INPUT_KEYS})
        q_filt[c, :, 2] = 0.2229
        q_filt[c, :, 6] = 1.0
        q_filt[c, :, 7:] = Q_INIT + rng.uniform(-0.1, 0.1, (B, 12))
        v_secu[c] = rng.uniform(-20, 20, (B, 12))
    calls = [{k: v.copy() for k, v in d.items()} for d in clean_calls]
    cq, cv = q_filt.copy(), v_secu.copy()
    for b, events in PLAN.items():
        for ev in events:
            c, what = ev[0], ev[1]
            if what == "q":
                q_filt[c, b, 7 + ev[2]] = ev[3]
            elif what == "v":
                v_secu[c, b, ev[2]] = ev[3]
            elif what == "tau":
                swing = calls[c]["contacts"][b] == 0
                assert swing.any(), (b, c)  # (the plan puts torque trips on calls where the robot has a swing foot)
                calls[c]["agoals"][b] = 1500.0 * np.where(rng.random((3, 4)) < 0.5, -1.0, 1.0) * swing[None, :]
            elif what == "nan":
                calls[c]["pgoals"][b, 1, 2] = np.nan
    flags = np.zeros((K, B), np.int32)
    for b, (c0, code) in EXPECT.items():
        flags[c0:, b] = code
    ctl = [oracle_mod.WbcController(0.002) for _ in range(B)]
    tau_max = np.zeros((K, B))
    for c, d in enumerate(calls):
        for b in range(B):
            ctl[b].compute(*[d[k][b] for k in wr.INPUT_KEYS])
            tau_max[c, b] = np.abs(ctl[b].tau_ff).max()  # (NaN for a robot with a NaN goal, on that call and after it)
    _cases.update(calls=calls, clean_calls=clean_calls, q_filt=q_filt, v_secu=v_secu, clean_q_filt=cq, clean_v_secu=cv, flags=flags,
                  tau_max=tau_max)
    return _cases


def glue_result(g, tau_ff, qdes, vdes, q_filt, v_secu):
    """controller_oracle.ControllerGlue.result plus the one thing the library adds to the reference (include/qrw_hip.h,
    glue::result): a non-finite tau_ff, qdes[7:] or vdes[6:] on an iteration that raises none of the reference's three flags
    raises the sticky code 4 (the reference's comparisons are blind to NaN)."""
    was = g.error
    res = g.result(tau_ff, qdes, vdes, q_filt, v_secu)
    if not was and not g.error and not (np.isfinite(tau_ff).all() and np.isfinite(qdes[7:]).all() and np.isfinite(vdes[6:]).all()):
        g.error, g.error_flag = True, 4
        res = tuple(SECURITY)
    return res


def test_fused_result_cases_do_not_hinge_on_rounding(oracle_mod, synth_mod):
    """The table on the CPU: the oracle's largest |tau_ff| of every robot-call is below 7.9 or above 8.1 N m (or NaN, for the two
    robots with a NaN goal), above on exactly the planned calls; ControllerGlue fed with the oracle's own outputs shows the
    planned flag after every call; the threshold values are the limits themselves and their upper neighbours."""
    import controller_oracle as co

    cs = cases(synth_mod, oracle_mod)
    tm = cs["tau_max"]
    nan_from = {b: ev[0] for b, events in PLAN.items() for ev in events if ev[1] == "nan"}
    over = {(ev[0], b) for b, events in PLAN.items() for ev in events if ev[1] == "tau"}
    for c in range(K):
        for b in range(B):
            if b in nan_from and c >= nan_from[b]:
                continue  # (the QP's warm start keeps the NaN: the robot is stopped, its later torques mean nothing)
            assert np.isfinite(tm[c, b]) and not (7.9 <= tm[c, b] <= 8.1), (c, b, tm[c, b])
            assert (tm[c, b] > 8.1) == ((c, b) in over), (c, b, tm[c, b])
    assert len(over) == 4 and sum(1 for b in range(B) if b not in EXPECT) >= 20
    assert np.nextafter(50.0, UP) > 50.0 and all(np.nextafter(x, UP) > x for x in Q_SEC)
    # the flags, from the oracle's WBC through the oracle's glue
    ctl = [oracle_mod.WbcController(0.002) for _ in range(B)]
    glue = [co.ControllerGlue(Q_INIT, 0.2229, 0.002) for _ in range(B)]
    for c, d in enumerate(cs["calls"]):
        for b in range(B):
            ctl[b].compute(*[d[k][b] for k in wr.INPUT_KEYS])
            glue_result(glue[b], ctl[b].tau_ff, ctl[b].qdes, ctl[b].vdes[:, 0], cs["q_filt"][c, b], cs["v_secu"][c, b])
            assert glue[b].error_flag == cs["flags"][c, b], (c, b)
    assert set(cs["flags"][-1]) == {0, 1, 2, 3, 4}


def _t(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _handle(lanes):
    import qrw_hip

    eng = qrw_hip.Batch(B)
    eng.wbc_set_lanes(lanes)
    eng.controller_init(_t(np.tile(Q_INIT, (B, 1))), 0.2229)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 4], ids=["wbc16_kernel", "wbc_kernel_quad"])
def test_fused_result_codes_precedence_thresholds_stickiness_isolation(oracle_mod, synth_mod, lanes):
    """qrw_wbc_compute_result over the table, on three handles: (a) the fused call, (b) qrw_wbc_compute + qrw_controller_result,
    (c) the fused call on the same inputs with nothing tripped.
      * result and error_flag of (a) are bit-identical to (b), the six WBC outputs too;
      * they equal ControllerGlue.result fed with the kernel's own tau_ff, qdes, vdes (exactly: 0.8 tau_ff is one product), and
        the flags are the planned ones after every call -- at the limit no flag, one ulp over it the flag, 1 + 2 -> 2,
        2 + 3 -> 3, 1 + 3 -> 3, 4 alone and 4 + 1 -> 1;
      * a tripped robot keeps its code and the security output (P = 0, D = 0.1, zeros) on every later call, clean or not;
      * every untripped robot is bit-identical to (c) in all eight outputs on every call, the three that share a wbc16 wavefront
        with a tripped one and the fifteen of a quad-kernel wavefront included."""
    import controller_oracle as co
    import torch

    cs = cases(synth_mod, oracle_mod)
    fused, separate, clean = _handle(lanes), _handle(lanes), _handle(lanes)
    glue = [co.ControllerGlue(Q_INIT, 0.2229, 0.002) for _ in range(B)]
    untripped = np.array([b for b in range(B) if b not in EXPECT])
    assert {16, 18, 19} <= set(untripped.tolist()) and 17 in EXPECT and len(untripped) >= 20
    wbc_keys = ("tau_ff", "qdes", "vdes", "f_with_delta", "ddq_res", "feet")
    for c in range(K):
        d, dc = cs["calls"][c], cs["clean_calls"][c]
        args = [_t(d[k]) for k in wr.INPUT_KEYS]
        qf, vs = _t(cs["q_filt"][c]), _t(cs["v_secu"][c])
        a = fused.wbc_compute_result(*args, qf, vs)
        w = separate.wbc_compute(*args)
        r = separate.controller_result(w["tau_ff"], w["qdes"], w["vdes"], qf, vs)
        n = clean.wbc_compute_result(*[_t(dc[k]) for k in wr.INPUT_KEYS], _t(cs["clean_q_filt"][c]), _t(cs["clean_v_secu"][c]))
        torch.cuda.synchronize()
        a, w, r, n = ({k: v.cpu().numpy() for k, v in x.items()} for x in (a, w, r, n))
        for k in wbc_keys:
            assert np.array_equal(a[k], w[k], equal_nan=True), (c, k)
        assert np.array_equal(a["result"], r["result"]) and np.array_equal(a["error_flag"], r["error_flag"]), c
        assert np.array_equal(a["error_flag"], cs["flags"][c]), (c, a["error_flag"], cs["flags"][c])
        assert np.isfinite(a["result"]).all()
        for b in range(B):
            res = glue_result(glue[b], a["tau_ff"][b], a["qdes"][b], a["vdes"][b], cs["q_filt"][c, b], cs["v_secu"][c, b])
            assert glue[b].error_flag == a["error_flag"][b], (c, b)
            assert np.array_equal(a["result"][b], np.stack(res)), (c, b)
            if b in EXPECT and c >= EXPECT[b][0]:
                assert a["error_flag"][b] == EXPECT[b][1] and np.array_equal(a["result"][b], SECURITY), (c, b)
            else:
                assert a["error_flag"][b] == 0 and np.array_equal(a["result"][b, 0], 3.0 * np.ones(12)), (c, b)
        assert (n["error_flag"][untripped] == 0).all()
        for k in wbc_keys + ("result", "error_flag"):
            assert np.array_equal(a[k][untripped], n[k][untripped]), (c, k)
    assert sorted(set(a["error_flag"].tolist())) == [0, 1, 2, 3, 4]
