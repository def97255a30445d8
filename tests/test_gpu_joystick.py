"""The joystick stage on the device (csrc/joystick_kernel.hip through qrw_joystick_*) against tests/joystick_numpy.py, the
stateful restatement of scripts/Joystick.py and scripts/PyBulletSimulator.py:402-431.

The criterion is BIT IDENTITY: the stage is a fixed sequence of + - * / on doubles with contraction off -- the same correctly
rounded IEEE sequence in numpy and on the device -- and the limits of qrw_joystick_init make every integer power exact
(csrc/joystick_profile.h).  B = 17 unless said otherwise; every robot has tables of its own."""
import numpy as np
import pytest

import joystick_cases as jc
import joystick_numpy as jn

pytestmark = pytest.mark.gpu
B17 = 17


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g

    g.build()
    import torch

    import Joystick
    import qrw_hip

    return torch, qrw_hip, Joystick


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def init(mods, eng, profiles=None, ramp=None, k_start=0, gamepad=None, codes=None, pushes=None):
    _, qrw_hip, Joystick = mods
    kw = {}
    if profiles is not None:
        mode = qrw_hip.JOY_PROFILE
        kw["k_switch"], kw["v_switch"] = Joystick.pad_profiles(profiles, eng.B)
    elif ramp is not None:
        mode, kw["ramp_v"], kw["k_start"] = qrw_hip.JOY_RAMP, ramp, k_start
    else:
        mode = qrw_hip.JOY_GAMEPAD
        kw.update({"gp_" + n: v for n, v in (gamepad or {}).items()})
    if codes is not None:
        kw["code_k"], kw["code_v"] = Joystick.pad_codes(codes, eng.B)
    if pushes is not None:
        kw["push_k"], kw["push_w"] = Joystick.pad_pushes(pushes, eng.B)
    eng.joystick_init(mode, **kw)


def device_run(mods, eng, ticks, v_gp=None, stops=None, with_f_ext=True):
    """The stage at every tick of `ticks`; v_ref (T,B,6), code (T,B), f_ext (T,B,6) as numpy.  v_gp (T,B,6) numpy; stops: a list
    of (B,) int arrays, one per tick."""
    torch = mods[0]
    dev = torch.device("cuda", eng.device)
    B, T = eng.B, len(ticks)
    v = torch.full((T, B, 6), np.nan, dtype=torch.float64, device=dev)
    f = torch.full((T, B, 6), np.nan, dtype=torch.float64, device=dev)
    c = torch.full((T, B), -7, dtype=torch.int32, device=dev)
    gp = None if v_gp is None else torch.from_numpy(np.ascontiguousarray(v_gp)).to(dev)
    st = None if stops is None else torch.from_numpy(np.ascontiguousarray(np.asarray(stops, dtype=np.int32))).to(dev)
    for i, k in enumerate(ticks):
        eng.joystick_step(int(k), v[i], code=c[i], f_ext=f[i] if with_f_ext else None, v_gp=None if gp is None else gp[i],
                          stop=None if st is None else st[i])
    torch.cuda.synchronize()
    return v.cpu().numpy(), c.cpu().numpy().astype(np.int64), f.cpu().numpy()


# ------------------------------------------------------------------------------------------------ profile mode
@pytest.mark.parametrize("n_cols", [2, 5, 32])
def test_profiles_equal_the_stateful_checker_bit_for_bit(mods, n_cols):
    """Tables of 2, 5 and 32 columns, padded ones among them, all six components nonzero, at every k_switch[i] - 1, k_switch[i],
    k_switch[i] + 1, the middle of every segment, 0 and 1000 ticks past the end.  The checker is stepped through every tick."""
    qrw_hip = mods[1]
    prof = jc.profile_tables(B17, n_cols, 20 + n_cols)
    ticks = jc.profile_ticks(prof)
    want = jc.expected(jc.robots(B17, profiles=prof), ticks)
    eng = qrw_hip.Batch(B17)
    init(mods, eng, profiles=prof)
    v, c, _ = device_run(mods, eng, ticks, with_f_ext=False)  # (d_f_ext NULL is accepted without pushes)
    assert (np.abs(want[0]).max(axis=(0, 1)) > 0).all() and len({len(p[0]) for p in prof}) > (1 if n_cols > 2 else 0)
    assert same_bits(v, want[0]), np.argwhere(bits(v) != bits(want[0]))[:5]
    assert not c.any()
    eng.close()


# ------------------------------------------------------------------------------------------------ ramp mode
def test_ramps_equal_the_checker_bit_for_bit(mods):
    """Speeds whose beta sits on the floor of 100, speeds above it, negative ones; ticks before k_start, inside and after."""
    qrw_hip = mods[1]
    k_start = 480
    V = jc.ramp_speeds(B17, 7)
    ticks = jc.ramp_ticks(V, k_start)
    want = jc.expected(jc.robots(B17, ramp=V, k_start=k_start), ticks, every_tick=False)  # (the ramp overwrites v_ref from k alone)
    eng = qrw_hip.Batch(B17)
    init(mods, eng, ramp=V, k_start=k_start)
    v, _, _ = device_run(mods, eng, ticks)
    assert same_bits(v, want[0]), np.argwhere(bits(v) != bits(want[0]))[:5]
    assert not want[0][0].any() and (want[0][-1][:, [0, 1, 5]] == V).all() and (V < 0).any()
    eng.close()


# ------------------------------------------------------------------------------------------------ gamepad mode
def test_the_gamepad_filter_equals_the_checker_on_every_tick(mods):
    """300 ticks of step and sign-changing commands: output and filter state bit-identical on every tick; the four dead-band
    neighbours (0.005 and -0.005 survive, one ulp inside is zeroed); a NaN command for one robot stays in that robot."""
    qrw_hip = mods[1]
    T = 300
    g = jc.gamepad_commands(B17, T, 8)
    fleet = jc.robots(B17, gamepad={})
    want = jn.run(fleet, range(T), g)[0]
    eng = qrw_hip.Batch(B17)
    init(mods, eng)
    v, _, _ = device_run(mods, eng, range(T), v_gp=g)
    assert same_bits(v, want), np.argwhere(bits(v) != bits(want))[:5]
    assert [v[0, b, 0] for b in range(4)] == [0.005, -0.005, 0.0, 0.0]
    assert (v == 0.0).any() and (np.abs(v) > 0.5).any()
    for b in (0, 5, 16):  # the state is what the last tick returned
        assert same_bits(eng.joystick_get("v_ref", b), want[-1, b])
    # a state read in the middle of the run, on every tick of a short one
    init(mods, eng)
    for k in range(5):
        vk, _, _ = device_run(mods, eng, [k], v_gp=g[k:k + 1])
        assert same_bits(vk[0], want[k]) and same_bits(eng.joystick_get("v_ref", 9), want[k, 9])
    # NaN for robot 6 from tick 3 on
    bad = g.copy()
    bad[3:, 6, 2] = np.nan
    init(mods, eng)
    vn, _, _ = device_run(mods, eng, range(T), v_gp=bad)
    others = np.arange(B17) != 6
    assert same_bits(vn[:, others], v[:, others]) and np.isnan(vn[3:, 6, 2]).all() and same_bits(vn[:, 6, :2], v[:, 6, :2])
    eng.close()


# ------------------------------------------------------------------------------------------------ codes
def test_codes_fire_on_their_tick_only_and_the_later_pair_wins(mods):
    qrw_hip = mods[1]
    codes = jc.code_tables(B17, 16, 9)
    ticks = jc.code_ticks(codes)
    prof = jc.profile_tables(B17, 2, 1)
    want = jc.expected(jc.robots(B17, profiles=prof, codes=codes), ticks)
    eng = qrw_hip.Batch(B17)
    init(mods, eng, profiles=prof, codes=codes)
    _, c, _ = device_run(mods, eng, ticks)
    assert np.array_equal(c, want[1])
    at = {k: i for i, k in enumerate(ticks)}
    assert c[at[20], 0] == 4 and c[at[19], 0] == 0 and c[at[21], 0] == 0  # (20, 2) then (20, 4): the later pair
    for b, pairs in enumerate(codes):
        fire = {k for k, _ in pairs}
        for k, _ in pairs:
            assert c[at[k], b] != 0
            for n in (k - 1, k + 1):
                if n >= 0 and n not in fire:
                    assert c[at[n], b] == 0
    assert not c[:, 2].any()
    eng.close()


# ------------------------------------------------------------------------------------------------ pushes
def test_pushes_equal_the_checker_bit_for_bit(mods):
    """start - 1, start, the middle, start + duration, start + duration + 1 of every push; two overlapping pushes sum in table
    order; d_f_ext NULL is refused once the handle has pushes."""
    qrw_hip = mods[1]
    pushes = jc.push_tables(B17, 8, 11)
    ticks = jc.push_ticks(pushes)
    V = jc.ramp_speeds(B17, 3)
    want = jc.expected(jc.robots(B17, ramp=V, pushes=pushes), ticks, every_tick=False)
    eng = qrw_hip.Batch(B17)
    init(mods, eng, ramp=V, pushes=pushes)
    _, _, f = device_run(mods, eng, ticks)
    assert same_bits(f, want[2]), np.argwhere(bits(f) != bits(want[2]))[:5]
    at = {k: i for i, k in enumerate(ticks)}
    both = f[at[25], 1]  # robot 1: (10, 20) and (18, 31) overlap at tick 25
    one = jn.JoystickNumpy(gamepad=True, pushes=pushes[1][:1]).apply_external_forces(25)
    two = jn.JoystickNumpy(gamepad=True, pushes=pushes[1][1:2]).apply_external_forces(25)
    assert same_bits(both, (np.zeros(6) + one) + two) and one.any() and two.any()
    assert not f[:, 2].any() and not f[at[9], 1].any() and not f[at[50], 1].any()
    with pytest.raises(qrw_hip.QrwError, match="qrw_joystick_step: the handle has pushes"):
        device_run(mods, eng, [0], with_f_ext=False)
    eng.close()


# ------------------------------------------------------------------------------------------------ stop latch
def test_the_stop_latch_is_sticky_and_stays_in_its_robot(mods):
    """A flag raised for robots 3 and 11 at ticks 5 and 9 and cleared at tick 12: k_stop is 5 and 9, their outputs are zero from
    then on, their filter state is frozen at the tick before, every other robot is bit-identical to the run with no flag;
    re-initialising resets k_stop to -1."""
    qrw_hip = mods[1]
    T = 30
    g = jc.gamepad_commands(B17, T, 12) + 0.25
    codes = [[(k, 1 + (k + b) % 4) for k in range(0, T, 3)][:16] for b in range(B17)]
    pushes = [[(0, T + b, np.array([1.0, 2.0, 3.0]), np.array([0.1, 0.2, 0.3]))] for b in range(B17)]
    stops = np.zeros((T, B17), np.int32)
    stops[5:12, 3], stops[9:12, 11] = 1, 4
    eng = qrw_hip.Batch(B17)
    init(mods, eng, codes=codes, pushes=pushes)
    clean = device_run(mods, eng, range(T), v_gp=g, stops=np.zeros_like(stops))
    assert np.array_equal(eng.joystick_get("k_stop"), np.full(B17, -1))
    init(mods, eng, codes=codes, pushes=pushes)
    got = device_run(mods, eng, range(T), v_gp=g, stops=stops)
    k_stop = eng.joystick_get("k_stop")
    assert k_stop[3] == 5 and k_stop[11] == 9 and np.array_equal(np.delete(k_stop, [3, 11]), np.full(B17 - 2, -1))
    others = np.ones(B17, bool)
    others[[3, 11]] = False
    for x, y in zip(got, clean):
        assert same_bits(x[:, others], y[:, others]) if x.dtype == np.float64 else np.array_equal(x[:, others], y[:, others])
        for b, k in ((3, 5), (11, 9)):
            assert np.array_equal(x[:k, b], y[:k, b]) and not x[k:, b].any() and y[k:, b].any()
    assert same_bits(eng.joystick_get("v_ref", 3), clean[0][4, 3]) and same_bits(eng.joystick_get("v_ref", 11), clean[0][8, 11])
    init(mods, eng, codes=codes, pushes=pushes)
    assert np.array_equal(eng.joystick_get("k_stop"), np.full(B17, -1)) and not eng.joystick_get("v_ref", 3).any()
    again = device_run(mods, eng, range(T), v_gp=g)
    assert all(np.array_equal(bits(x) if x.dtype == np.float64 else x, bits(y) if y.dtype == np.float64 else y) for x, y in zip(again, clean))
    eng.close()


# ------------------------------------------------------------------------------------------------ position in the batch
def test_outputs_do_not_depend_on_the_position_in_the_batch(mods):
    """B = 83 (two wavefronts, the second partial) against B = 17 and B = 1, bit for bit; one robot's tables at positions 0, 63,
    64 and 82 of 83 give identical outputs."""
    qrw_hip = mods[1]
    B = 83
    prof, codes, pushes = jc.profile_tables(B, 5, 31), jc.code_tables(B, 4, 32), jc.push_tables(B, 3, 33)
    for tab in (prof, codes, pushes):
        for b in (63, 64, 82):
            tab[b] = tab[0]
    ticks = sorted(set(jc.profile_ticks(prof[:B17], past=50)) | set(jc.push_ticks(pushes[:B17])) | set(jc.code_ticks(codes[:B17])))
    runs = {}
    for n in (83, 17, 1):
        eng = qrw_hip.Batch(n)
        init(mods, eng, profiles=prof[:n], codes=codes[:n], pushes=pushes[:n])
        runs[n] = device_run(mods, eng, ticks)
        eng.close()
    for x83, x17, x1 in zip(runs[83], runs[17], runs[1]):
        eq = same_bits if x83.dtype == np.float64 else np.array_equal
        assert eq(x83[:, :17], x17) and eq(x17[:, :1], x1)
        for b in (63, 64, 82):
            assert eq(x83[:, b], x83[:, 0])
    want = jc.expected(jc.robots(83, profiles=prof, codes=codes, pushes=pushes), ticks)
    assert same_bits(runs[83][0], want[0]) and np.array_equal(runs[83][1], want[1]) and same_bits(runs[83][2], want[2])
    assert runs[83][0].any() and runs[83][1].any() and runs[83][2].any()


# ------------------------------------------------------------------------------------------------ host entry point, state bytes
def test_the_host_entry_point_equals_the_device_one_and_the_state_is_counted_once(mods):
    qrw_hip = mods[1]
    eng = qrw_hip.Batch(B17)
    before = eng.state_bytes()
    T = 12
    g = jc.gamepad_commands(B17, T, 13)
    codes, pushes = jc.code_tables(B17, 3, 14), jc.push_tables(B17, 2, 15)
    init(mods, eng, codes=codes, pushes=pushes)
    first = eng.state_bytes()
    assert first == before + 7 * 8 * B17
    dev = device_run(mods, eng, range(T), v_gp=g)
    init(mods, eng, codes=codes, pushes=pushes)
    assert eng.state_bytes() == first
    stop = np.zeros(B17, np.int32)
    for k in range(T):
        stop[2] = int(k >= 7)
        o = eng.joystick_step_host(k, v_gp=g[k], stop=stop)
        live = np.arange(B17) != 2 if k >= 7 else np.ones(B17, bool)
        assert same_bits(o["v_ref"][live], dev[0][k][live]) and np.array_equal(o["code"][live], dev[1][k][live])
        assert same_bits(o["f_ext"][live], dev[2][k][live])
        assert k < 7 or not (o["v_ref"][2].any() or o["code"][2] or o["f_ext"][2].any())
    assert eng.joystick_get("k_stop")[2] == 7
    init(mods, eng, profiles=jc.profile_tables(B17, 32, 1), codes=jc.code_tables(B17, 16, 2), pushes=jc.push_tables(B17, 8, 3))
    assert eng.state_bytes() == first  # (larger tables: the state does not grow)
    eng.close()


# ------------------------------------------------------------------------------------------------ errors
def test_bad_tables_and_bad_calls_are_refused_with_the_robot_and_the_entry(mods):
    torch, qrw_hip, Joystick = mods
    eng = qrw_hip.Batch(B17)
    dev = torch.device("cuda", 0)
    v, gp = torch.zeros((B17, 6), dtype=torch.float64, device=dev), torch.zeros((B17, 6), dtype=torch.float64, device=dev)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_joystick_step: joystick not initialised"):
        eng.joystick_step(0, v)
    good = jc.profile_tables(B17, 5, 4)
    K, V = Joystick.pad_profiles(good, B17)

    def refused(text, **kw):
        with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_joystick_init: " + text):
            eng.joystick_init(kw.pop("mode", qrw_hip.JOY_PROFILE), **kw)

    bad = K.copy()
    bad[4, 2] = bad[4, 1] - 1
    refused("robot 4, k_switch entry 2: decreasing", k_switch=bad, v_switch=V)
    bad = K.copy()
    bad[9, 3:] += (1 << 17) + 1 - (bad[9, 3] - bad[9, 2])
    refused("robot 9, k_switch entry 3: more than 2\\^17 ticks", k_switch=bad, v_switch=V)
    bad[9, 3:] -= 1
    eng.joystick_init(qrw_hip.JOY_PROFILE, k_switch=bad, v_switch=V)  # (exactly 2^17 is legal)
    PK, PW = Joystick.pad_pushes(jc.push_tables(B17, 3, 5), B17)
    for duration, robot, entry in ((0, 7, 0), ((1 << 13) + 1, 16, 2)):
        bad = PK.copy()
        bad[robot, entry, 1] = duration
        refused("robot %d, push entry %d: duration %d" % (robot, entry, duration), k_switch=K, v_switch=V, push_k=bad, push_w=PW)
    bad = PK.copy()
    bad[0, 0, 1] = 1 << 13
    eng.joystick_init(qrw_hip.JOY_PROFILE, k_switch=K, v_switch=V, push_k=bad, push_w=PW)
    refused("n_switch must be in 1..32", k_switch=np.zeros((B17, 0), np.int32), v_switch=np.zeros((B17, 6, 0)))
    refused("n_switch must be in 1..32", k_switch=np.zeros((B17, 33), np.int32), v_switch=np.zeros((B17, 6, 33)))
    # the refusals left the handle with the last good tables
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_joystick_step: d_v_gp given to a joystick that is not in gamepad mode"):
        eng.joystick_step(0, v, f_ext=gp.clone(), v_gp=gp)
    eng.joystick_init(qrw_hip.JOY_GAMEPAD)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_joystick_step: gamepad mode needs d_v_gp"):
        eng.joystick_step(0, v)
    with pytest.raises(qrw_hip.QrwError, match=r"\(-1\): qrw_joystick_step: k must be >= 0"):
        eng.joystick_step(-1, v, v_gp=gp)
    eng.close()


# ------------------------------------------------------------------------------------------------ wiring
def test_the_stage_feeds_the_closed_loop_and_the_bound_iteration_stays_bound(mods):
    """Closed loop at B = 8 for 40 ticks (four solves): Joystick_batch.step -> compute_sensors(joy.v_ref, **sim.sensors,
    joystick_code=joy.code) -> sim.step(r, f_ext=joy.f_ext), the profile ramping 0 -> 0.2 m/s, a code at tick 20, a push over ticks
    10..30.  Every tick's Result, error flags and simulator outputs -- and the simulator's final state -- are bit-identical to a
    second run in which the three tensors are filled from the first run's record and the stage is not called; every
    non-solving tick of the first run went through the bound iteration, bound once, and the three tensors never moved."""
    torch, qrw_hip, Joystick = mods
    from Controller import Controller_batch
    from Simulator import Simulator_batch

    B, T = 8, 40
    q_init = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])
    speed = np.zeros((B, 6, 2))
    speed[:, 0, 1], speed[:, 5, 1] = 0.2, np.linspace(-0.1, 0.1, B)
    profiles = [([0, 30 + 2 * b], speed[b]) for b in range(B)]
    codes = [[(20, 1 + b % 3)] for b in range(B)]
    pushes = [[(10, 20, np.array([0.0, 2.0 + 0.25 * b, 0.0]), np.array([0.0, 0.0, 0.05]))] for b in range(B)]
    names = ("q_mes", "v_mes", "quat", "ang_vel", "lin_acc", "true_pos", "contact_forces", "joint_torques")

    def loop(feed):
        ctl = Controller_batch(B, q_init, estimator=dict(h_init=0.22294615))
        sim = Simulator_batch(B, q_init, controller=ctl)
        calls = dict(pre=0, bind=0)
        pre, bind = ctl._b.control_pre, ctl._b.bind_iteration
        ctl._b.control_pre = lambda *a, **k: (calls.__setitem__("pre", calls["pre"] + 1), pre(*a, **k))[1]
        ctl._b.bind_iteration = lambda *a, **k: (calls.__setitem__("bind", calls["bind"] + 1), bind(*a, **k))[1]
        if feed is None:
            joy = Joystick.Joystick_batch(ctl, profiles=profiles, codes=codes, pushes=pushes)
            v_ref, code, f_ext = joy.v_ref, joy.code, joy.f_ext
        else:
            v_ref, code, f_ext = feed[0][0].clone(), feed[1][0].clone(), feed[2][0].clone()
        ptrs = (v_ref.data_ptr(), code.data_ptr(), f_ext.data_ptr())
        rec, ins = [], ([], [], [])
        for k in range(T):
            if feed is None:
                joy.step(k)
            else:
                for dst, src in zip((v_ref, code, f_ext), feed):
                    dst.copy_(src[k])
            for lst, t in zip(ins, (v_ref, code, f_ext)):
                lst.append(t.clone())
            r = ctl.compute_sensors(v_ref, **sim.sensors, joystick_code=code)
            sim.step(r, f_ext=f_ext)
            rec.append([ctl._res["result"].clone(), ctl.error_flag.clone()] + [sim.out[n].clone() for n in names])
        torch.cuda.synchronize()
        assert ptrs == (v_ref.data_ptr(), code.data_ptr(), f_ext.data_ptr())
        # control_pre ran on the four solving ticks only: the 36 others took the bound iteration, which was bound once
        assert calls == dict(pre=4, bind=1) and ctl._fast is not None and ctl._fast[4] is v_ref and ctl._fast[9] is code
        state = sim.state()
        out = [[x.cpu().numpy() for x in row] for row in rec], state, [torch.stack(x) for x in ins]
        k_stop = joy.k_stop() if feed is None else None
        return out + (k_stop,)

    rec_a, state_a, feed, k_stop = loop(None)
    rec_b, state_b, _, _ = loop(feed)
    for k, (ra, rb) in enumerate(zip(rec_a, rec_b)):
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y, equal_nan=True) and (x.dtype != np.float64 or same_bits(x, y)), k
    for n in state_a:
        assert np.array_equal(state_a[n], state_b[n]), n
    v, c, f = (x.cpu().numpy() for x in feed)
    assert v[0].max() == 0.0 and 0.19 < v[-1, 0, 0] <= 0.2 and (c[20] == [1 + b % 3 for b in range(B)]).all() and not c[:20].any()
    assert not c[21:].any() and not f[:10].any() and not f[31:].any() and f[20, :, 1].min() >= 2.0
    assert not state_a["status"].any() and np.array_equal(k_stop, np.full(B, -1)) and not rec_a[-1][1].any()
    assert np.all(np.isfinite(rec_a[-1][0]))
