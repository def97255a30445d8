"""Record-and-audit test of the WHOLE device loop on its own signals: Joystick_batch.step -> Controller_batch.compute_sensors
(estimator, planners, MPC, glue, WBC, result) -> Simulator_batch.step, every inter-stage tensor of every tick kept; then, on the
host, every stage of every robot held to its checker FED WITH THE DEVICE'S OWN RECORDED INPUTS OF THAT STAGE (teacher forcing,
tests/loop_chain.py), so that contact dynamics cannot amplify rounding into a divergence and no robot and no tick is excused.
A wiring error between the stages -- the estimator reading the gait after the planners' roll, a code or a push a tick late, the
latch seeing the flag of the wrong tick -- is a disagreement of one stage with its checker here, where a device-against-device
test shows it identically on both sides.

Scenarios: tests/loop_cases.py (a base that travels and yaws, gait changes through joystick_code, pushes through the dynamics, and
the whole stopped regime: flag, latch, zero joystick outputs, security branch P = 0 D = 0.1, the simulator collapsing under
damping, the estimator at large attitude); tests/test_loop_cpu.py holds them to what they claim on the checkers alone.

Criteria, none derived from the device's output:
  joystick    bit identity of v_ref, code, f_ext on every tick and of k_stop (tests/test_gpu_joystick.py's criterion)
  simulator   every state item and output within 100 x LOOP_TICK_SPREAD[variant]["sim"] relative to max(1, |item|_inf), tick and
              status equal, the checker's smallest |d| above MIN_ABS_D
  estimator   rtol 1e-9 / atol 1e-11 (tests/test_gpu_estimator.py); the Kalman variant's q_filt and v_filt within KALMAN_BOUND
              (tests/test_gpu_estimator_kalman.py)
  controller  error_flag equal on every tick, P and D exact, q_des / v_des / tau_ff within 1e-4 relative (_closed_loop of
              tests/test_gpu_controller.py), the MPC's status equal on solving ticks; iteration counts compared and printed only
  scenario    tests/loop_cases.py's check_scenario on the device's record

Worst deviations as printed on the device (see the docstring of test_the_device_loop_stage_by_stage)."""
import numpy as np
import pytest

import loop_cases as lc
import loop_chain as lch

pytestmark = pytest.mark.gpu

CTL_RTOL = 1e-4  # _closed_loop's


def device_record(variant):
    """The loop on the device for the variant's T ticks.  Returns dict of numpy arrays with a leading tick axis -- v_ref, code, f_ext,
    the estimator's four outputs, result, flag, contacts, every simulator output and state item (index 0 of `out` / `state` is
    the state after sim_init, index k + 1 the one after tick k) --, solves {tick: (iterations, status)} and k_stop."""
    import torch

    from Controller import Controller_batch
    from Joystick import Joystick_batch
    from Simulator import Simulator_batch, reference_rough_ground

    f = lc.fleet(variant)
    B, T, asyn = f["B"], f["T"], f["lag"] is not None
    rec = {n: [] for n in ("v_ref", "code", "f_ext", "result", "flag", "contacts") + lch.EST_KEYS}
    out, state, solves = {n: [] for n in lch.SIM_OUT_KEYS}, {n: [] for n in lch.SIM_STATE_KEYS + ("tick", "status")}, {}
    with torch.cuda.stream(torch.cuda.Stream()):
        ctl = Controller_batch(B, lc.Q_INIT, multiprocessing=asyn, mpc_lag=f["lag"], groups=1,
                               estimator=dict(h_init=lc.H_INIT, kalman=f["kalman"]), **lc.DEFAULT_CFG)
        kw = dict(terrain=reference_rough_ground(), terrain_origin=lc.origins(B)) if f["rough"] else {}
        sim = Simulator_batch(B, lc.Q_INIT, dt=lc.DEFAULT_CFG["dt_wbc"], controller=ctl, **kw)
        joy = Joystick_batch(ctl, profiles=f["profiles"], codes=f["codes"], pushes=f["pushes"])

        def keep_sim():
            torch.cuda.synchronize()
            for n in lch.SIM_OUT_KEYS:
                out[n].append(sim.out[n].cpu().numpy().copy())
            st = sim.state()
            for n in state:
                state[n].append(st[n].copy())

        keep_sim()
        for k in range(T):
            joy.step(k)
            r = ctl.compute_sensors(joy.v_ref, **sim.sensors, joystick_code=joy.code)
            sim.step(r, f_ext=joy.f_ext)
            keep_sim()
            for n, t in (("v_ref", joy.v_ref), ("code", joy.code), ("f_ext", joy.f_ext), ("result", ctl._res["result"]),
                         ("flag", ctl.error_flag), ("contacts", ctl._pre["contacts"]), ("q_filt", ctl.q_filt), ("v_filt", ctl.v_filt),
                         ("rpy", ctl.rpy), ("v_secu", ctl.v_secu)):
                rec[n].append(t.cpu().numpy().copy())
            if k % ctl.k_mpc == 0:
                st = ctl.stats()["mpc"]
                solves[k] = (st["iters"].copy(), st["status"].copy())
        k_stop = joy.k_stop()
        ctl.stop_parallel_loop()
    rec = {n: np.stack(v) for n, v in rec.items()}
    rec["contacts"] = rec["contacts"].reshape(T, B, 4)
    return dict(rec, out={n: np.stack(v) for n, v in out.items()}, state={n: np.stack(v) for n, v in state.items()}, solves=solves,
                k_stop=np.asarray(k_stop))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Audit:
    """Worst deviation per stage, and every violation (the first few are shown): the whole record is compared before anything
    is asserted, so one run says everything."""

    def __init__(self):
        self.worst, self.bad = {}, []

    def hold(self, stage, err, bound, where):
        self.worst[stage] = max(self.worst.get(stage, 0.0), float(err))
        if not err <= bound:
            self.bad.append((stage, where, float(err), bound))

    def same(self, stage, ok, where):
        if not ok:
            self.bad.append((stage, where))


def estimator_errors(kalman, name, got, ref):
    """(error, bound) pairs of one estimator output in the measures of the two estimator test files."""
    import test_gpu_estimator as tge
    import test_gpu_estimator_kalman as tgk

    if kalman and name in ("q_filt", "v_filt"):
        return tgk.kalman_err(got, ref), tgk.KALMAN_BOUND
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got) - ref) / (tge.ATOL + tge.RTOL * np.abs(ref))  # np.allclose's criterion, as a ratio
    return float(np.max(np.where(np.isnan(e), np.inf, e))), 1.0


@pytest.mark.parametrize("variant", list(lc.VARIANTS))
def test_the_device_loop_stage_by_stage(oracle_mod, variant):
    """B = 8 x 320 ticks on the plane, B = 6 x 240 on the reference's rough ground with the Kalman estimator, B = 5 x 120 with the
    asynchronous MPC adopted three iterations late: zero robots and zero ticks left out.
    Worst deviations as printed on the device; every flag rose on the checkers' tick (plane 137 and 111, rough 152 and 137,
    asynchronous 92), k_stop one later, the MPC's iteration counts differed on 0 of 256 / 144 / 60 solves:
                                                   plane      rough_kalman   async_lag3     bound
        controller q_des / v_des / tau_ff          9.6e-11    4.3e-11        4.8e-12        1e-4
        estimator, share of rtol 1e-9 + atol 1e-11 2.1e-3     7.7e-7 (*)     3.8e-4         1
        (*) rpy and v_secu; the Kalman q_filt 1.6e-13 and v_filt 7.6e-14 against KALMAN_BOUND 4.3e-11
        simulator state / outputs                  4.1e-11    1.6e-11        9.5e-12        1.46e-8 / 2.24e-9 / 1.49e-9
        smallest |d| of the forced ticks           5.6e-7     2.7e-7         1.4e-6         > 1e-9
    The estimator's existing tolerances hold on the tumbling robots too, so no bound from LOOP_TICK_SPREAD's `est` is in use."""
    import test_gpu_sim as tgs

    f = lc.fleet(variant)
    B, T = f["B"], f["T"]
    dev = device_record(variant)
    sim_bound = 100.0 * lc.LOOP_TICK_SPREAD[variant]["sim"]
    cs, a = lc.chains(variant), Audit()
    iter_mismatch = n_solves = 0
    for b, c in enumerate(cs):
        for k in range(T):
            w = (f["names"][b], k)
            forced = dict(flag_prev=int(dev["flag"][k - 1, b]) if k else 0, sensors={n: dev["out"][n][k, b] for n in lch.SENSOR_KEYS},
                          v_ref=dev["v_ref"][k, b], code=int(dev["code"][k, b]), f_ext=dev["f_ext"][k, b],
                          est={n: dev[n][k, b] for n in lch.EST_KEYS}, result=dev["result"][k, b],
                          sim_state={n: dev["state"][n][k, b] for n in dev["state"]})
            o = c.tick(k, forced)
            # joystick: the stage's own criterion
            a.same("joystick v_ref", np.array_equal(bits(o["v_ref"]), bits(dev["v_ref"][k, b])), w)
            a.same("joystick code", o["code"] == dev["code"][k, b], w)
            a.same("joystick f_ext", np.array_equal(bits(o["f_ext"]), bits(dev["f_ext"][k, b])), w)
            # estimator
            for n in lch.EST_KEYS:
                e, bound = estimator_errors(f["kalman"], n, dev[n][k, b], o["est"][n])
                a.hold("estimator %s (%s)" % (n, "KALMAN_BOUND" if bound != 1.0 else "of rtol 1e-9 + atol 1e-11"), e, bound, w)
            # controller
            ref = o["ctl"]["result"]
            a.same("error_flag", o["ctl"]["flag"] == dev["flag"][k, b], w + (o["ctl"]["flag"], int(dev["flag"][k, b])))
            for i, (name, tol) in enumerate((("P", 0.0), ("D", 0.0), ("q_des", CTL_RTOL), ("v_des", CTL_RTOL), ("tau_ff", CTL_RTOL))):
                a.hold("controller " + name, lch.rel(dev["result"][k, b, i], ref[i]), tol, w)
            if o["ctl"]["solve"] is not None:
                it, status = dev["solves"][k]
                n_solves += 1
                iter_mismatch += int(it[b] != o["ctl"]["solve"][0])
                a.same("mpc status", status[b] == o["ctl"]["solve"][1], w + (int(status[b]), o["ctl"]["solve"][1]))
            a.same("contacts", np.array_equal(dev["contacts"][k, b], o["ctl"]["gait_row0"]), w)
            # simulator: one forced tick from the device's previous state
            s = o["sim"]
            a.same("simulator tick / status", s.tick == dev["state"]["tick"][k + 1, b] and s.status == dev["state"]["status"][k + 1, b], w)
            for n, x in (("q", s.q), ("v", s.v), ("prev_o_imuVel", s.prev)):
                a.hold("simulator state", lch.rel(dev["state"][n][k + 1, b], x), sim_bound, w + (n,))
            for n in lch.SIM_OUT_KEYS:
                a.hold("simulator outputs", lch.rel(dev["out"][n][k + 1, b], s.out[n]), sim_bound, w + (n,))
        a.same("k_stop", c.k_stop == dev["k_stop"][b], (f["names"][b], c.k_stop, int(dev["k_stop"][b])))
    smallest = min(c.sim.min_abs_d for c in cs)
    print("whole loop %s (B = %d, T = %d): worst deviations %s; simulator bound %.3g; smallest |d| %.3g; MPC iteration counts differ "
          "on %d of %d solves" % (variant, B, T, {n: "%.3g" % e for n, e in sorted(a.worst.items())}, sim_bound, smallest,
                                 iter_mismatch, n_solves))
    assert not a.bad, (len(a.bad), a.bad[:12])
    assert smallest > tgs.MIN_ABS_D, smallest
    # the scenario on the device's own record
    feet = (dev["out"]["contact_forces"][1:, :, :, 2] > 0).sum(axis=2)
    seen = lc.check_scenario(variant, dev["flag"], dev["k_stop"], dev["v_ref"], dev["code"], dev["f_ext"], dev["contacts"], feet,
                             dev["state"]["status"][1:])
    for b in range(B):
        if f["stops"][b] is None:
            assert all(np.all(np.isfinite(dev[n][:, b])) for n in ("result",) + lch.EST_KEYS), f["names"][b]
            assert all(np.all(np.isfinite(x[:, b])) for x in list(dev["out"].values()) + list(dev["state"].values())), f["names"][b]
        else:
            kf = lc.flag_tick(dev["flag"][:, b])
            assert np.array_equal(dev["result"][kf:, b, 0], np.zeros((T - kf, 12))) and np.all(dev["result"][kf:, b, 1] == 0.1)
            assert not dev["result"][kf:, b, 2:].any()  # the security branch: P = 0, D = 0.1, no targets, no torque
    print("whole loop %s: flags rose at %s, k_stop %s, feet in contact seen %s"
          % (variant, [lc.flag_tick(dev["flag"][:, b]) for b in range(B)], dev["k_stop"].tolist(), seen))
