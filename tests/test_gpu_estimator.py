"""GPU parity tests of the batched state estimator (estimator_kernel.hip through the C ABI, the drop-in Estimator.py and
Controller_batch.compute_sensors) against the numpy checker tests/estimator_numpy.py.

Tolerance: rtol 1e-9, atol 1e-11 -- the project's own for the other kernel that chains trigonometry and polynomials in FP64
(tests/test_gpu_planner.py:56); the integer and boolean items (k_since_contact, close_from_contact, k_log) compare exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])  # scripts/main_solo12_control.py:120
H_INIT = 0.22294615
DT = 0.002
RTOL, ATOL = 1e-9, 1e-11
EXACT = ("k_since_contact", "close_from_contact", "k_log")
SENSOR_KEYS = ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")
IDENT = np.array([0.0, 0.0, 0.0, 1.0])


def _t(x, dtype=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def en(oracle_mod):
    import estimator_numpy

    return estimator_numpy


def _close(got, ref, what):
    assert np.allclose(got, ref, rtol=RTOL, atol=ATOL), (what, np.abs(np.asarray(got) - np.asarray(ref)).max(), got, ref)


def _compare(eng, out, refs, tick, items=True, robots=None):
    """The four outputs of every robot and (items) every getter item against the checker objects (robots: the instances of the
    handle they stand for; None: 0, 1, ...)."""
    import qrw_hip

    for b, r in enumerate(refs) if robots is None else zip(robots, refs):
        _close(out["q_filt"][b], r.q_filt, ("q_filt", tick, b))
        _close(out["v_filt"][b], r.v_filt, ("v_filt", tick, b))
        _close(out["rpy"][b], r.RPY, ("rpy", tick, b))
        _close(out["v_secu"][b], r.v_secu, ("v_secu", tick, b))
        if not items:
            continue
        want = r.items()
        assert set(want) == set(qrw_hip.ESTIMATOR_ITEMS)
        for name, ref in want.items():
            got = eng.estimator_get(name, b)
            if name in EXACT:
                assert np.array_equal(got, ref), (name, tick, b, got, ref)
            else:
                _close(got, ref, (name, tick, b))


def _step(eng, refs, tick, sensors, gait, goals, true_pos=None, true_b_vel=None, items=True, planner=False):
    """One tick on the device (explicit gait / goals unless planner=True: NULL, the handle's planner state) and in the checker."""
    import torch

    opt = lambda x: None if x is None else _t(x)
    o = eng.estimator_step(*[_t(sensors[k]) for k in SENSOR_KEYS], gait=None if planner else _t(gait),
                           goals=None if planner else _t(goals), true_pos=opt(true_pos), true_b_vel=opt(true_b_vel))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    for b, r in enumerate(refs):
        r.run_filter(gait[b], goals[b], *[sensors[k][b] for k in SENSOR_KEYS],
                     true_pos=None if true_pos is None else true_pos[b], true_b_vel=None if true_b_vel is None else true_b_vel[b])
    _compare(eng, out, refs, tick, items)
    return out


def test_run_with_explicit_gait_matches_the_checker(oracle_mod, synth_mod, en):
    """B = 17 (two wavefronts, the second holding one quad), 200 ticks (more than one 160-tick trot period: the >= 16 threshold,
    both halves of the alpha ramp and every contact switch occur), gait matrices and foot positions of oracle planners stepped
    alongside, gait codes changing twice (ticks 5 and 35, static among them: a new gait enters at the END of the current one, so
    its rows reach row 0 sixteen MPC steps later -- four-stance rows from tick 161 to 190): all outputs and every state item, every
    tick."""
    import qrw_hip

    B, N_gait = 17, 20
    eng = qrw_hip.Batch(B, 16, N_gait)
    eng.estimator_init(H_INIT)
    refs = [en.Estimator(DT, H_INIT) for _ in range(B)]
    plan = [oracle_mod.Planner() for _ in range(B)]
    sen = synth_mod.SyntheticSensors(B, 7)
    rng = np.random.default_rng(5)
    vref = rng.uniform(-0.4, 0.4, (B, 6)) * np.array([1.5, 0.8, 0, 0, 0, 1.0])
    q7 = np.array([0.0, 0.0, 0.2229, 0.0, 0.0, 0.0, 1.0])
    seen_static = seen_alpha_low = False
    for k in range(200):
        gait = np.stack([p.gaits()[1] for p in plan])
        goals = np.stack([p.feet()[0] for p in plan])
        _step(eng, refs, k, sen.step(k), gait, goals)
        seen_static = seen_static or any(np.all(g[0] == 1) for g in gait)
        seen_alpha_low = seen_alpha_low or any(r.alpha < 0.98 for r in refs)
        for b, p in enumerate(plan):  # (the planners run AFTER the estimator, scripts/Controller.py:213-236)
            code = ((4 if b % 2 == 0 else 1) if k == 5 else 3 if k == 35 else 0)
            p.step(k, q7, vref[b], vref[b], code)
    assert seen_static and seen_alpha_low
    assert all(r.k_log == 200 for r in refs)
    assert eng.state_bytes() >= B * 47 * 8


def test_run_on_the_handles_planner_state(oracle_mod, synth_mod, en):
    """B = 5, d_gait / d_goals NULL: the estimator reads the current gait (64-bit column masks) and the foot positions of the
    handle's planner, with qrw_planner_step after it on every tick as Controller.compute orders them."""
    import torch

    import qrw_hip

    B = 5
    eng = qrw_hip.Batch(B, 16, 20)
    eng.planner_init()
    eng.estimator_init(H_INIT)
    refs = [en.Estimator(DT, H_INIT) for _ in range(B)]
    plan = [oracle_mod.Planner() for _ in range(B)]
    sen = synth_mod.SyntheticSensors(B, 8)
    rng = np.random.default_rng(6)
    vref = rng.uniform(-0.4, 0.4, (B, 6)) * np.array([1.5, 0.8, 0, 0, 0, 1.0])
    q7 = np.tile(np.array([0.0, 0.0, 0.2229, 0.0, 0.0, 0.0, 1.0]), (B, 1))
    pout = None
    for k in range(100):
        gait = np.stack([p.gaits()[1] for p in plan])
        goals = np.stack([p.feet()[0] for p in plan])
        _step(eng, refs, k, sen.step(k), gait, goals, planner=True, items=(k % 10 == 9))
        code = np.array([[1, 2, 3, 4, 5][b] if k == 35 else 0 for b in range(B)], np.int32)
        pout = eng.planner_step(k, _t(q7), _t(vref), _t(vref), _t(code, np.int32), out=pout)
        torch.cuda.synchronize()
        for b, p in enumerate(plan):
            p.step(k, q7[b], vref[b], vref[b], int(code[b]))


# ------------------------------------------------------------------------------------------------ off the default configuration
def test_other_time_step_and_gait_table_length(oracle_mod, synth_mod, en):
    """dt_wbc = 0.001 and gait matrices of 26 rows (tests/test_gpu_controller.py's ALT_CFG), B = 17, 120 ticks, noisy sensors: the
    filters' coefficients and integration step take the handle's dt, the scan for the end of the phase runs over 26 rows (robots
    2 and 9 have no zero row, robots 5 and 16 have 26 equal rows: the scan ends at N_gait).  All outputs and every state item,
    every tick.  And the time step matters: the checker at 0.002 gives another v_filt."""
    import qrw_hip
    import test_gpu_estimator_kalman as K

    seq = K.alt_trot_sequence(synth_mod)
    eng = qrw_hip.Batch(17, **K.ALT_HANDLE)
    eng.estimator_init(H_INIT)
    refs, plain = [en.Estimator(K.ALT_DT, H_INIT) for _ in range(17)], en.Estimator(DT, H_INIT)
    seen = set()
    for k, t in enumerate(seq):
        _step(eng, refs, k, t["sensors"], t["gait"], t["goals"])
        K.checker_step(plain, t, 0)
        seen |= {r.remaining_steps for r in refs}
    assert all(r.k_log == 120 for r in refs) and seen >= {K.ALT_N_GAIT, 8, 1}, seen
    assert any(r.alpha < 0.98 for r in refs)
    assert not np.allclose(plain.v_filt, refs[0].v_filt, rtol=1e3 * RTOL, atol=1e3 * ATOL)


def test_other_configuration_on_the_handles_planner_state(oracle_mod, synth_mod, en):
    """The same configuration with d_gait / d_goals NULL, B = 5, 60 ticks: the handle's planner (k_mpc = 20, T_gait = 0.40, 26-row
    matrices as 64-bit column masks) stepped after the estimator, against oracle planners of that configuration."""
    import torch

    import qrw_hip
    import test_gpu_estimator_kalman as K

    B = 5
    eng = qrw_hip.Batch(B, **K.ALT_HANDLE)
    eng.planner_init(**K.ALT_OPTIONS["planner_init"])
    eng.estimator_init(H_INIT)
    refs = [en.Estimator(K.ALT_DT, H_INIT) for _ in range(B)]
    pout = None
    for k, t in enumerate(K.planner_sequence(oracle_mod, synth_mod, seed=18, **K.ALT_PLANNER)):
        assert t["gait"].shape == (B, K.ALT_N_GAIT, 4)
        _step(eng, refs, k, t["sensors"], t["gait"], t["goals"], planner=True)
        q7, vref, code = t["plan"]
        pout = eng.planner_step(k, _t(q7), _t(vref), _t(vref), _t(code, np.int32), out=pout)
        torch.cuda.synchronize()


def test_block_coverage(oracle_mod, synth_mod, en):
    """test_gpu_estimator_kalman.block_coverage for the complementary filters: B = 83 against B = 17 bit for bit over 20 ticks, the
    first tick of robots 64..82 (the init kernel's second block) against the checker."""
    import test_gpu_estimator_kalman as K

    K.block_coverage(synth_mod, False, lambda: en.Estimator(DT, H_INIT),
                     lambda eng, out, refs, robots: _compare(eng, out, refs, 0, robots=robots))


# ------------------------------------------------------------------------------------------------ hand-made corners
S = np.sqrt(0.5)  # S * S = 0.5000000000000001: 2 S S >= 1.0 exactly as numpy rounds it


def _plain(B, rng):
    d = dict(lin_acc=rng.uniform(-0.5, 0.5, (B, 3)), ang_vel=rng.uniform(-0.3, 0.3, (B, 3)), quat=np.tile(IDENT, (B, 1)),
             q_mes=Q_INIT + rng.uniform(-0.05, 0.05, (B, 12)), v_mes=rng.uniform(-1.0, 1.0, (B, 12)))
    return d


def _table(row0, B, N_gait=20):
    g = np.zeros((B, N_gait, 4))
    g[:, :8] = np.asarray(row0, dtype=np.float64).reshape(-1, 1, 4)
    g[:, 8:16] = [0, 1, 1, 0]
    return g


@pytest.mark.parametrize("corner", ["pitch_clamp", "zero_atan2_arguments", "no_foot_in_contact", "one_foot_in_contact",
                                    "contact_counter_15_to_16", "perfect"])
def test_hand_made_corners(oracle_mod, en, corner):
    import qrw_hip

    B = 4
    rng = np.random.default_rng(21)
    eng = qrw_hip.Batch(B, 16, 20)
    perfect = corner == "perfect"
    eng.estimator_init(H_INIT, perfect)
    refs = [en.Estimator(DT, H_INIT, perfect) for _ in range(B)]
    goals = rng.uniform(-0.2, 0.2, (B, 3, 4))
    stance = _table([1, 1, 1, 1], B)
    true = lambda: (rng.uniform(-1, 1, (B, 3)), rng.uniform(-1, 1, (B, 3))) if perfect else (None, None)
    lead = 15 if corner == "contact_counter_15_to_16" else 20
    if corner == "contact_counter_15_to_16":  # robot b: foot b alone (robot 3: all four) in stance from the first tick
        stance = _table([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]], B)
    for k in range(lead):
        tp, tv = true()
        _step(eng, refs, k, _plain(B, rng), stance, goals, tp, tv, items=(k == lead - 1))
    d = _plain(B, rng)
    gait = stance
    before = {n: np.stack([eng.estimator_get(n, b) for b in range(B)]) for n in ("FK_lin_vel", "FK_xyz", "xyz_mean_feet")}
    if corner == "pitch_clamp":
        # 2 S S = 1.0000000000000002 (clamp), the same negative, exactly 1.0 from a quaternion that is not normalised (>= clamps),
        # and the last double below 1.0 (arcsin)
        d["quat"] = np.array([[0.0, S, 0.0, S], [0.0, -S, 0.0, S], [0.0, 0.5, 0.0, 1.0], [0.0, np.nextafter(S, 0), 0.0, np.nextafter(S, 0)]])
    elif corner == "zero_atan2_arguments":
        # pitch +-pi/2: both arguments of both atan2 are 0; roll pi/2 and yaw pi/2: the second argument alone is 0 and the guard
        # returns 0 where atan2 would give pi/2 (scripts/Estimator.py:696, :711)
        d["quat"] = np.array([[0.0, S, 0.0, S], [S, 0.0, 0.0, S], [0.0, 0.0, S, S], [0.0, 0.0, -S, S]])
    elif corner == "no_foot_in_contact":
        gait = _table([0, 0, 0, 0], B)
    elif corner == "one_foot_in_contact":
        gait = _table([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], B)
    elif corner == "contact_counter_15_to_16":
        assert all(np.array_equal(before["FK_xyz"][b], [0.0, 0.0, H_INIT]) for b in range(B))  # nothing has counted yet
    tp, tv = true()
    out = _step(eng, refs, lead, d, gait, goals, tp, tv)
    after = {n: np.stack([eng.estimator_get(n, b) for b in range(B)]) for n in before}
    if corner == "pitch_clamp":
        assert np.array_equal(out["rpy"][:3, 1], [np.pi / 2, -np.pi / 2, np.pi / 2]) and out["rpy"][3, 1] < np.pi / 2
    elif corner == "zero_atan2_arguments":
        assert np.array_equal(out["rpy"][0], [0.0, np.pi / 2, 0.0]) and out["rpy"][1, 0] == 0.0
    elif corner == "no_foot_in_contact":
        assert all(np.array_equal(before[n], after[n]) for n in before)  # the persisted values are kept
    elif corner == "one_foot_in_contact":
        assert not np.array_equal(before["FK_xyz"], after["FK_xyz"])
        assert np.array_equal(after["xyz_mean_feet"], np.stack([goals[b][:, b] for b in range(B)]))
    elif corner == "contact_counter_15_to_16":
        assert all(eng.estimator_get("k_since_contact", b).max() == 16.0 for b in range(B))
        assert all(after["FK_xyz"][b, 2] != H_INIT for b in range(B))
    else:
        assert np.array_equal(out["q_filt"][:, 2], tp[:, 2] - 0.0155)


def test_reinitialisation_restores_the_first_call(oracle_mod, en):
    import qrw_hip

    B = 4
    rng = np.random.default_rng(22)
    eng = qrw_hip.Batch(B, 16, 20)
    eng.estimator_init(H_INIT)
    refs = [en.Estimator(DT, H_INIT) for _ in range(B)]
    gait, goals = _table([1, 0, 0, 1], B), rng.uniform(-0.2, 0.2, (B, 3, 4))
    yaw = lambda a: np.tile(en.euler_to_quaternion([0.0, 0.0, a]), (B, 1))
    for k in range(6):
        d = _plain(B, rng)
        d["quat"] = yaw(0.4 + 0.1 * k)
        out = _step(eng, refs, k, d, gait, goals, items=False)
    assert abs(out["rpy"][0, 2] - 0.4) < 1e-12  # (offset latched at the second call: 0.5)
    eng.estimator_init(H_INIT)
    refs = [en.Estimator(DT, H_INIT) for _ in range(B)]
    d = _plain(B, rng)
    d["quat"] = yaw(1.3)
    out = _step(eng, refs, 0, d, gait, goals)
    assert np.array_equal(out["rpy"][:, 2], np.zeros(B))  # latched again
    assert all(eng.estimator_get("k_log", b)[0] == 1.0 and eng.estimator_get("k_since_contact", b).max() == 1.0 for b in range(B))


# ------------------------------------------------------------------------------------------------ host entry point, drop-in
class _Device:
    pass


def test_dropin_estimator_matches_the_checker(oracle_mod, synth_mod, en):
    """Estimator.run_filter (qrw_estimator_step_host on a batch-1 handle) over 60 ticks on a dummy device; the first call is the
    one Controller.__init__ makes with its dummy device (scripts/Controller.py:190-198)."""
    import Estimator as dropin

    est = dropin.Estimator(DT, 1000, H_INIT)
    ref = en.Estimator(DT, H_INIT)
    plan = oracle_mod.Planner()
    sen = synth_mod.SyntheticSensors(1, 9)
    dev = _Device()
    dev.q_mes, dev.v_mes = Q_INIT, np.zeros(12)
    dev.baseLinearAcceleration, dev.baseAngularVelocity, dev.baseOrientation = np.zeros(3), np.zeros(3), IDENT
    dev.dummyPos, dev.b_baseVel = np.array([0.0, 0.0, Q_INIT[2]]), np.zeros(3)
    q7, v = np.array([0.0, 0.0, 0.2229, 0.0, 0.0, 0.0, 1.0]), np.array([0.2, 0.0, 0, 0, 0, 0.1])
    for k in range(60):
        gait, goals = plan.gaits()[1], plan.feet()[0]
        if k > 0:
            d = sen.step(k)
            dev.baseLinearAcceleration, dev.baseAngularVelocity, dev.baseOrientation = d["lin_acc"][0], d["ang_vel"][0], d["quat"][0]
            dev.q_mes, dev.v_mes = d["q_mes"][0], d["v_mes"][0]
        assert est.run_filter(k, gait, dev, goals) == 0
        ref.run_filter(gait, goals, dev.baseLinearAcceleration, dev.baseAngularVelocity, dev.baseOrientation, dev.q_mes, dev.v_mes)
        assert est.q_filt.shape == (19, 1) and est.v_filt.shape == (18, 1) and est.RPY.shape == (3, 1)
        _close(est.q_filt[:, 0], ref.q_filt, ("q_filt", k))
        _close(est.v_filt[:, 0], ref.v_filt, ("v_filt", k))
        _close(est.v_secu, ref.v_secu, ("v_secu", k))
        _close(est.RPY[:, 0], ref.RPY, ("RPY", k))
        if k == 0:
            # the reference's state after Controller.__init__: nothing but the position filter's low-pass half has moved
            assert np.array_equal(est.q_filt[3:, 0], np.concatenate([IDENT, Q_INIT]))
            assert np.array_equal(est.v_filt, np.zeros((18, 1))) and np.array_equal(est.v_secu, np.zeros(12))
            assert np.array_equal(est.RPY, np.zeros((3, 1))) and est.alpha == 1.0 and est.close_from_contact is True
            assert np.array_equal(est.k_since_contact, gait[0]) and np.array_equal(est.FK_xyz, [0.0, 0.0, H_INIT])
            mean = goals[:, gait[0] == 1].mean(axis=1)
            _close(est.q_filt[:3, 0], [0.005 * mean[0], 0.005 * mean[1], 0.9 * H_INIT + 0.1 * (H_INIT + mean[2])], "first q_filt")
        if k % 20 == 19:
            for name in ("FK_lin_vel", "FK_xyz", "filt_lin_vel", "xyz_mean_feet"):
                _close(getattr(est, name), getattr(ref, name), (name, k))
            assert est.alpha == pytest.approx(ref.alpha, rel=RTOL) and est.close_from_contact == ref.close_from_contact
            assert np.array_equal(est.k_since_contact, ref.k_since_contact)
        plan.step(k, q7, v, v, 0)
    q, vv = est.get_configurations()
    assert q.shape == (19,) and vv.shape == (18,)


def test_errors_leave_the_handle_usable(oracle_mod, en):
    """Step before qrw_estimator_init, NULL gait before qrw_planner_init, one of the two `perfect` inputs without the other: -1 and
    a text that names the entry point and the reason; the next valid call works."""
    import qrw_hip

    B = 2
    rng = np.random.default_rng(23)
    eng = qrw_hip.Batch(B, 16, 20)
    d, gait, goals = _plain(B, rng), _table([1, 1, 1, 1], B), np.zeros((B, 3, 4))
    args = [_t(d[k]) for k in SENSOR_KEYS]
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_step: estimator not initialised"):
        eng.estimator_step(*args, gait=_t(gait), goals=_t(goals))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_get_host: bad item"):
        qrw_hip._check(eng._lib.qrw_estimator_get_host(eng._handle, 13, 0, 1, qrw_hip._p(np.empty(1))), "qrw_estimator_get_host")
    eng.estimator_init(H_INIT, perfect=True)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_step: planner not initialised"):
        eng.estimator_step(*args, true_pos=_t(np.zeros((B, 3))), true_b_vel=_t(np.zeros((B, 3))))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_step: a perfect estimator needs both"):
        eng.estimator_step(*args, gait=_t(gait), goals=_t(goals), true_pos=_t(np.zeros((B, 3))))
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_step: a perfect estimator needs both"):
        eng.estimator_step(*args, gait=_t(gait), goals=_t(goals), true_b_vel=_t(np.zeros((B, 3))))
    refs = [en.Estimator(DT, H_INIT, True) for _ in range(B)]
    _step(eng, refs, 0, d, gait, goals, np.ones((B, 3)), np.ones((B, 3)))
    eng.estimator_init(H_INIT, perfect=False)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_estimator_step: d_true_pos / d_true_b_vel given"):
        eng.estimator_step(*args, gait=_t(gait), goals=_t(goals), true_pos=_t(np.zeros((B, 3))))
    refs = [en.Estimator(DT, H_INIT) for _ in range(B)]
    _step(eng, refs, 0, d, gait, goals)


# ------------------------------------------------------------------------------------------------ fleet
def _fleet_inputs(synth_mod, B, ticks, seed):
    sen = synth_mod.SyntheticSensors(B, seed)
    rng = np.random.default_rng(seed)
    vref = rng.uniform(-0.4, 0.4, (B, 6)) * np.array([1.5, 0.8, 0, 0, 0, 1.0])
    return vref, [sen.step(k) for k in range(ticks)]


def _run_fleet(ctl, vref, ticks, separate=False):
    """compute_sensors over the ticks (separate: compute() fed with the outputs of a separate estimator_step on ctl's handle);
    returns per tick (result, error flags, q_filt, v_filt, rpy, v_secu) as host arrays."""
    import torch

    vr, rec, o = _t(vref), [], None
    result = ctl._fleet_result if hasattr(ctl, "_fleet_result") else None  # (stream groups: the fleet's tensor)
    if separate:
        ctl._b.estimator_init(H_INIT)
    for d in ticks:
        s = [_t(d[k]) for k in SENSOR_KEYS]
        if separate:
            o = ctl._b.estimator_step(*s, out=o)
            ctl.compute(vr, o["q_filt"], o["v_filt"], o["rpy"], o["v_secu"])
            est = [o[n] for n in ("q_filt", "v_filt", "rpy", "v_secu")]
        else:
            ctl.compute_sensors(vr, *s)
            est = [ctl.q_filt, ctl.v_filt, ctl.rpy, ctl.v_secu]
        torch.cuda.current_stream().synchronize()
        rec.append([x.cpu().numpy().copy() for x in [ctl._res["result"] if result is None else result, ctl.error_flag] + est])
    return rec


def _same(rec_a, rec_b):
    for k, (a, b) in enumerate(zip(rec_a, rec_b)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (k, i, np.abs(x - y).max())


def test_fleet_compute_sensors_is_estimator_step_then_compute(oracle_mod, synth_mod, en):
    """Controller_batch(B=8, estimator=...).compute_sensors over 30 ticks (three solves): bit for bit compute() fed with a separate
    estimator_step on the same sensors, and within the closed loop's tolerances (tests/test_gpu_controller.py, _closed_loop) the
    chained checker + oracles: estimator -> updateState -> planners -> MPC -> WBC -> result."""
    import controller_oracle as co
    from Controller import Controller_batch

    B, T = 8, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 31)
    a = _run_fleet(Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT)), vref, ticks)
    b = _run_fleet(Controller_batch(B, Q_INIT), vref, ticks, separate=True)
    _same(a, b)
    n_steps = 16
    first = np.zeros((24, n_steps))
    first[2, 0] = 0.2229
    first[12:, 0] = [0.0, 0.0, 8.0] * 4
    for r in range(B):
        est, glue, plan = en.Estimator(DT, H_INIT), co.ControllerGlue(Q_INIT, 0.2229, DT), oracle_mod.Planner()
        mpc, wbc = oracle_mod.MPC(0.02, n_steps, 0.32, 20), oracle_mod.WbcController(DT)
        x_f_mpc, latest, not_first = first, None, False
        for k in range(T):
            d = ticks[k]
            est.run_filter(plan.gaits()[1], plan.feet()[0], *[d[n][r] for n in SENSOR_KEYS])
            for i, ref in enumerate((est.q_filt, est.v_filt, est.RPY, est.v_secu)):
                _close(a[k][2 + i][r], ref, ("estimator output", i, k, r))
            oRh, oTh = glue.update_state(vref[r], est.q_filt, est.v_filt, est.RPY)
            plan.step(k, glue.q[:7, 0], glue.h_v[:6, 0], glue.v_ref[:6, 0], 0)
            xref, (fsteps, _, _), cgait = plan.xref(), plan.footsteps(), plan.gaits()[1]
            if k % 10 == 0:
                mpc.run(k, xref, fsteps)
                latest = mpc.get_latest_result().copy()
            if not_first and latest is not None:  # (the first call returns the default, scripts/MPC_Wrapper.py:106-126)
                x_f_mpc = latest
            not_first = True
            pos, vel, acc, _, _ = plan.feet()
            xw, qw, bv = glue.wbc_inputs(x_f_mpc, xref, oRh, oTh, pos, vel, acc)
            wbc.compute(qw, bv, xw[12:], cgait[0, :], glue.feet_p_cmd, glue.feet_v_cmd, glue.feet_a_cmd)
            P, D, q_des, v_des, t8 = glue.result(wbc.tau_ff, wbc.qdes, wbc.vdes[:, 0], est.q_filt, est.v_secu)
            assert a[k][1][r] == glue.error_flag, (k, r)
            for i, (ref, tol) in enumerate(((P, 0), (D, 0), (q_des, 1e-4), (v_des, 1e-4), (t8, 1e-4))):
                err = np.max(np.abs(a[k][0][r, i] - ref)) / max(1.0, np.max(np.abs(ref)))
                assert err <= tol, (k, r, i, err)


def test_fleet_stream_groups_are_bit_identical_to_one_handle(synth_mod):
    from Controller import Controller_batch, Controller_groups

    B, T = 8, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 32)
    one = _run_fleet(Controller_batch(B, Q_INIT, estimator=dict(h_init=H_INIT)), vref, ticks)
    ctl = Controller_batch(B, Q_INIT, groups=2, estimator=dict(h_init=H_INIT))
    assert isinstance(ctl, Controller_groups) and ctl.q_filt.shape == (B, 19)
    _same(one, _run_fleet(ctl, vref, ticks))


def test_fleet_staggered_group_starts_its_estimator_with_its_first_iteration(synth_mod):
    """groups=2, stagger=True: group 1 runs k_mpc / 2 ticks behind and its estimator's first call (the yaw-offset latch, the
    counters) is that group's first iteration -- its robots get, bit for bit, a single handle started that many ticks later on
    the same readings; before that its estimator outputs are untouched."""
    from Controller import Controller_batch

    B, T = 8, 20
    vref, ticks = _fleet_inputs(synth_mod, B, T, 34)
    ctl = Controller_batch(B, Q_INIT, groups=2, stagger=True, estimator=dict(h_init=H_INIT))
    lag = ctl.lag_of(1)
    assert lag == 5 and ctl.lag_of(0) == 0
    rec = _run_fleet(ctl, vref, ticks)
    late = _run_fleet(Controller_batch(B // 2, Q_INIT, estimator=dict(h_init=H_INIT)), vref[B // 2:],
                      [{n: v[B // 2:] for n, v in d.items()} for d in ticks[lag:]])
    for k in range(T - lag):
        for i in range(6):
            assert np.array_equal(rec[k + lag][i][B // 2:], late[k][i]), (k, i)
    assert all(not rec[k][i][B // 2:].any() for k in range(lag) for i in range(2, 6))
    assert all(rec[k][2][:B // 2].any() for k in range(lag))  # (group 0 has started)


def test_fleet_asynchronous_mode_matches_its_synchronous_estimator_counterpart(synth_mod):
    """multiprocessing=True, mpc_lag=3: the estimator enqueued on the loop's stream by compute_sensors against the same controller
    fed by a separate estimator_step on the caller's stream."""
    import torch
    from Controller import Controller_batch

    B, T = 8, 30
    vref, ticks = _fleet_inputs(synth_mod, B, T, 33)
    with torch.cuda.stream(torch.cuda.Stream()):
        ca = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3, estimator=dict(h_init=H_INIT))
        a = _run_fleet(ca, vref, ticks)
        ca.stop_parallel_loop()
        cb = Controller_batch(B, Q_INIT, multiprocessing=True, mpc_lag=3)
        b = _run_fleet(cb, vref, ticks, separate=True)
        cb.stop_parallel_loop()
    _same(a, b)


def test_compute_sensors_needs_the_estimator():
    import qrw_hip
    from Controller import Controller_batch

    ctl = Controller_batch(2, Q_INIT)
    z = _t(np.zeros((2, 3)))
    with pytest.raises(qrw_hip.QrwError, match="estimator"):
        ctl.compute_sensors(_t(np.zeros((2, 6))), z, z, _t(np.tile(IDENT, (2, 1))), _t(np.tile(Q_INIT, (2, 1))), _t(np.zeros((2, 12))))
    assert ctl.q_filt is None
