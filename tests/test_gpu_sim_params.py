"""GPU tests of the simulator away from its defaults: every field of qrw_sim_params changed (on the plane and on the rough field),
each of them changed alone, the command stride of the fleet path, the position of a robot in the batch and the batch's size,
every way into the frozen state and both ways out, and the momentum of a robot in flight.  The checkers are
tests/sim_numpy.py and tests/sim_terrain_numpy.py; the helpers are those of tests/test_gpu_sim.py and
tests/test_gpu_sim_terrain.py, which take the parameters as arguments.

Tolerances, by the method of tests/test_gpu_sim.py: the checker against itself with every input moved by one ulp, on the cases
of THIS file (plane_spreads / terrain_spreads below; scripts/sim_tolerance.py and scripts/sim_terrain_tolerance.py print them),
relative to max(1, |item|_inf); every bound is 100 x the largest spread of the cases it is used on.
  plane, forward dynamics, the 17 states of test_gpu_sim._fd_states with and without the wrench:
      TUNED 2.13e-13, kn alone 1.36e-13, dn alone 1.34e-13, mu alone 2.05e-13, vs alone 1.33e-13, foot_radius alone 1.35e-13
                                                                                 -> FD_SPREAD 2.13e-13, FD_BOUND 2.13e-11
      (the largest relative change in a over the 17 states: vs alone 0.0632, dn 0.193, kn 0.384, foot_radius 0.521, mu 0.692)
  plane, one tick of the checker's free run of test_gpu_sim._tick_case under TUNED, 60 ticks: 1.05e-12 (smallest |d| 2.53e-08,
      0, 1, 2, 3 and 4 feet in contact)                                          -> TICK_SPREAD 1.05e-12, TICK_BOUND 1.05e-10
  plane, the first five ticks of that case with substeps = 1: 4.23e-12, 3: 5.63e-12, 8 (the defaults): 9.31e-12, dt = 0.001:
      1.46e-12 (smallest |d| 6.31e-07)                                           -> V_TICK_SPREAD 9.31e-12, V_TICK_BOUND 9.31e-10
  rough field, forward dynamics, the 17 states of test_gpu_sim_terrain._fd_states settled under TUNED: 5.16e-14
                                                                                 -> T_FD_SPREAD 5.16e-14, T_FD_BOUND 5.16e-12
  rough field, one tick, 60 ticks of test_gpu_sim_terrain._tick_case(seed=ROUGH_SEED) settled under TUNED: 1.22e-12 (smallest
      |d| 2.08e-06, |fu - fv| 3.93e-05, edge distance 3.34e-06; 0, 1, 2, 3 and 4 feet in contact, both triangle kinds)
                                                                                 -> T_TICK_SPREAD 1.22e-12, T_TICK_BOUND 1.22e-10
The runs at the defaults (command stride) are the first 20 ticks of the run test_gpu_sim's TICK_BOUND was measured on and keep it.
No state of a parity test may come nearer to a switch of the contact law than MIN_ABS_D / MIN_SWITCH; no robot is excused."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_sim as tg
import test_gpu_sim_terrain as tt
from test_gpu_sim import B17, MIN_ABS_D, OUT_KEYS, RESIDUAL_EPS, _rel, _run, _same, _t
from test_gpu_sim_terrain import MIN_SWITCH, set_terrain

pytestmark = pytest.mark.gpu

TUNED = dict(dt=0.001, substeps=3, kn=6.5e3, dn=35.0, mu=0.55, vs=0.03, foot_radius=0.021)  # all seven away from the defaults
SINGLE = {n: TUNED[n] for n in ("kn", "dn", "mu", "vs", "foot_radius")}                      # ... and each contact parameter alone
TICK_VARIANTS = (dict(substeps=1), dict(substeps=3), dict(substeps=8), dict(dt=0.001))       # five ticks each
FD_SPREAD, FD_BOUND = 2.13e-13, 2.13e-11
TICK_SPREAD, TICK_BOUND = 1.05e-12, 1.05e-10
V_TICK_SPREAD, V_TICK_BOUND = 9.31e-12, 9.31e-10
T_FD_SPREAD, T_FD_BOUND = 5.16e-14, 5.16e-12
T_TICK_SPREAD, T_TICK_BOUND = 1.22e-12, 1.22e-10
# the rough field's teacher-forced case under TUNED: with test_gpu_sim_terrain's own seed (7) the checker's free run passes a foot
# within 1.3e-9 of d = 0, next to the guard; these initial states and commands keep 2e-6 from every switch
ROUGH_SEED = 9
B83 = 83  # six blocks of 16 quads, the last holding three


@pytest.fixture(scope="module")
def sn(oracle_mod):
    import sim_numpy

    return sim_numpy


@pytest.fixture(scope="module")
def stn(oracle_mod):
    import sim_terrain_numpy

    return sim_terrain_numpy


# ------------------------------------------------------------------------------------------------ the checker against itself
def plane_spreads(sn):
    """(forward-dynamics one-ulp spreads by case, per-tick (spread, smallest |d|, feet seen) by case) on the plane; no GPU."""
    states = tg._fd_states(sn)
    fd = {"TUNED": tg.fd_spread(sn, states, TUNED)[1]}
    fd.update({name: tg.fd_spread(sn, states, {name: value})[1] for name, value in SINGLE.items()})
    tick = {"TUNED": tg.tick_spread(sn, B17, 60, **TUNED)}
    tick.update({"%s=%s" % next(iter(var.items())): tg.tick_spread(sn, B17, 5, **var) for var in TICK_VARIANTS})
    return fd, tick


def terrain_spreads(stn):
    """(forward-dynamics one-ulp spread, tick_spread's tuple) on the rough field under TUNED; no GPU."""
    return tt.fd_spread(stn, fields=("rough",), prm=TUNED)[1], tt.tick_spread(stn, B17, 60, seed=ROUGH_SEED, **TUNED)


# ------------------------------------------------------------------------------------------------ helpers
def _stack(states, i):
    return np.stack([s[i] for s in states])


def _compare_fd(oracle_mod, sn, eng, states, with_f_ext, bound, **params):
    """test_gpu_sim's forward-dynamics comparison on the plane with the parameters given to the device and the checker alike:
    accelerations and forces within `bound`, the row-by-row residual, no foot near the switch.  Returns the contact counts."""
    prm = dict(sn.DEFAULTS, **params)
    a_dev, f_dev = eng.test_sim_forward_dynamics(_stack(states, 0), _stack(states, 1), _stack(states, 2),
                                                 f_ext=_stack(states, 3) if with_f_ext else None, **params)
    worst, contacts = 0.0, []
    assert len(states) == B17 == len(a_dev) == len(f_dev)  # (no state left out)
    for i, (q, v, tau, fx, want) in enumerate(states):
        f_ext = fx if with_f_ext else None
        a, f, d = sn.forward_dynamics(q, v, tau, prm, f_ext=f_ext)
        assert np.abs(d).min() > MIN_ABS_D, (i, d)
        contacts.append(int((d > 0).sum()))
        if want is not None:
            assert contacts[-1] == want, (i, d)
        ea, ef = _rel(a_dev[i], a), _rel(f_dev[i], f)
        worst = max(worst, ea, ef)
        assert ea <= bound and ef <= bound, (i, ea, ef)
        J, M, h = oracle_mod.feet_jacobians(q), oracle_mod.crba(q), oracle_mod.rnea(q, v, np.zeros(18))
        res = oracle_mod.rnea(q, v, a_dev[i]) - (sn.rhs_of(q, v, tau, f_dev[i], J, f_ext) + h)
        scale = np.abs(M) @ np.abs(a_dev[i]) + np.abs(h) + np.abs(J.T) @ np.abs(f_dev[i].ravel())
        assert np.all(np.abs(res) <= RESIDUAL_EPS * 2.0 ** -52 * scale), (i, np.abs(res / scale).max() / 2.0 ** -52)
    print("  worst relative error %.3g (bound %.3g), feet in contact %s" % (worst, bound, contacts))
    return contacts


def _plain(eng, out, cmd, f_ext):
    eng.sim_step(*[_t(x) for x in cmd], out, f_ext=None if f_ext is None else _t(f_ext))


def _planes(eng, out, cmd, f_ext):
    """The five commands as the planes of one contiguous (B,5,12) tensor: Batch.sim_step's cmd_ld = 60 branch."""
    import torch

    res = torch.full((len(cmd[0]), 5, 12), float("nan"), dtype=torch.float64, device="cuda")
    for i, x in enumerate(cmd):
        res[:, i] = _t(x)
    planes = [res[:, i] for i in range(5)]
    assert not any(p.is_contiguous() for p in planes) and all(p.stride() == (60, 1) for p in planes)
    eng.sim_step(*planes, out, f_ext=None if f_ext is None else _t(f_ext))


def _record(eng, out):
    st = eng.sim_state()
    return [st[n].copy() for n in tg.STATE_KEYS + ("tick", "status")] + [out[n].cpu().numpy() for n in OUT_KEYS]


def _teacher_forced(eng, out, refs, command, ticks, bound, deliver=_plain):
    """test_gpu_sim's teacher-forced loop for either checker: each tick every checker object starts from the device's state;
    every state item and output of every robot compared after the tick.  Returns the device's record per tick (_run's layout)
    and the numbers of feet in contact the checkers saw."""
    import torch

    st = eng.sim_state()
    worst = tg._compare_tick(st, {n: out[n].cpu().numpy() for n in OUT_KEYS}, refs, -1, bound)
    rec, in_contact, compared = [], set(), 0
    for k in range(ticks):
        *cmd, f_ext = command(k)
        for b, r in enumerate(refs):
            r.set_state(st["q"][b], st["v"][b], st["prev_o_imuVel"][b], st["tick"][b])
            r.step(*[x[b] for x in cmd], None if f_ext is None else f_ext[b])
            in_contact.add(int((np.abs(r.out["contact_forces"]).sum(axis=1) > 0).sum()))
        deliver(eng, out, cmd, f_ext)
        torch.cuda.synchronize()
        st = eng.sim_state()
        worst = max(worst, tg._compare_tick(st, {n: out[n].cpu().numpy() for n in OUT_KEYS}, refs, k, bound))
        compared += len(refs)
        rec.append(_record(eng, out))
    assert compared == ticks * len(refs) == ticks * eng.B  # (no comparison left out)
    print("  %d ticks x %d robots: worst relative error %.3g (bound %.3g), feet in contact seen %s"
          % (ticks, len(refs), worst, bound, sorted(in_contact)))
    return rec, in_contact


# ------------------------------------------------------------------------------------------------ 1. every parameter changed
@pytest.mark.parametrize("with_f_ext", [False, True])
def test_forward_dynamics_with_every_parameter_changed(oracle_mod, sn, with_f_ext):
    """The 17 states of test_gpu_sim._fd_states under TUNED on the device and in the checker."""
    import qrw_hip

    contacts = _compare_fd(oracle_mod, sn, qrw_hip.Batch(2), tg._fd_states(sn), with_f_ext, FD_BOUND, **TUNED)
    assert {0, 1, 4} <= set(contacts), contacts


@pytest.mark.parametrize("with_f_ext", [False, True])
def test_forward_dynamics_on_the_rough_field_with_every_parameter_changed(oracle_mod, stn, with_f_ext):
    """The rough field's 17 states, settled again under TUNED's foot_radius, with per-robot origins."""
    import qrw_hip

    T, states = tt._fd_states(stn, "rough", prm=dict(stn.DEFAULTS, **TUNED))
    eng = qrw_hip.Batch(B17)
    set_terrain(eng, T, origin=_stack(states, 4))
    worst, contacts, kinds = tt._compare_fd(oracle_mod, stn, eng, T, states, with_f_ext, bound=T_FD_BOUND, **TUNED)
    print("forward dynamics on the rough field under TUNED, f_ext=%s: worst relative error %.3g (bound %.3g)" % (with_f_ext, worst, T_FD_BOUND))
    assert {0, 1, 4} <= set(contacts), contacts
    assert kinds == {"lower", "upper"}, kinds
    tt.check_identical_robots(stn, T, states)


def test_teacher_forced_ticks_with_every_parameter_changed(oracle_mod, sn):
    """60 ticks at B = 17 of test_gpu_sim._tick_case under TUNED (dt, the sub-steps and the five contact parameters)."""
    import qrw_hip

    q0, command = tg._tick_case(sn)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    eng.sim_init(_t(q0), out, **TUNED)
    refs = [sn.SimNumpy(q0[b], **TUNED) for b in range(B17)]
    _, in_contact = _teacher_forced(eng, out, refs, command, 60, TICK_BOUND)
    smallest = min(r.min_abs_d for r in refs)
    print("  smallest |d| %.3g" % smallest)
    assert smallest > MIN_ABS_D, smallest
    assert {0, 4} <= in_contact, in_contact


def test_teacher_forced_ticks_on_the_rough_field_with_every_parameter_changed(oracle_mod, stn):
    """60 ticks at B = 17 of test_gpu_sim_terrain._tick_case, settled and run under TUNED, with per-robot origins."""
    import qrw_hip

    T, origin, q0, command = tt._tick_case(stn, seed=ROUGH_SEED, prm=dict(stn.DEFAULTS, **TUNED))
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    set_terrain(eng, T, origin=origin)
    eng.sim_init(_t(q0), out, **TUNED)
    refs = [stn.SimTerrainNumpy(q0[b], T, origin[b], **TUNED) for b in range(B17)]
    _, in_contact = _teacher_forced(eng, out, refs, command, 60, T_TICK_BOUND)
    d_min, diag_min, edge_min = (min(getattr(r, n) for r in refs) for n in ("min_abs_d", "min_diag", "min_edge"))
    kinds = set().union(*[r.kinds for r in refs])
    print("  smallest |d| %.3g, |fu - fv| %.3g, edge distance %.3g; triangles %s" % (d_min, diag_min, edge_min, sorted(kinds)))
    assert min(d_min, diag_min, edge_min) > MIN_SWITCH, (d_min, diag_min, edge_min)
    assert in_contact == {0, 1, 2, 3, 4}, in_contact
    assert kinds == {"lower", "upper"}, kinds


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_each_contact_parameter_matters(oracle_mod, sn, name):
    """One contact parameter changed alone: the device follows the checker with that one change within FD_BOUND, and over the 17
    states its accelerations differ from its own at the defaults by more than 1000 x FD_BOUND -- two parameters swapped anywhere
    between the binding and the contact law cannot pass this for both."""
    import qrw_hip

    states = tg._fd_states(sn)
    eng = qrw_hip.Batch(2)
    _compare_fd(oracle_mod, sn, eng, states, True, FD_BOUND, **{name: SINGLE[name]})
    a_one, _ = eng.test_sim_forward_dynamics(_stack(states, 0), _stack(states, 1), _stack(states, 2), **{name: SINGLE[name]})
    a_def, _ = eng.test_sim_forward_dynamics(_stack(states, 0), _stack(states, 1), _stack(states, 2))
    change = max(_rel(a_one[i], a_def[i]) for i in range(B17))
    print("  %s alone: largest relative change in a %.3g" % (name, change))
    assert change > 1e3 * FD_BOUND, (name, change)


def test_substeps_and_dt_matter(oracle_mod, sn):
    """substeps 1, 3 and 8 and dt 0.001 against 0.002, five teacher-forced ticks each: within V_TICK_BOUND of the checker with the
    same setting, and the four runs' final velocities differ pairwise by more than 1000 x V_TICK_BOUND."""
    import qrw_hip

    q0, command = tg._tick_case(sn)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    last = []
    for var in TICK_VARIANTS:
        eng.sim_init(_t(q0), out, **var)
        refs = [sn.SimNumpy(q0[b], **var) for b in range(B17)]
        rec, _ = _teacher_forced(eng, out, refs, command, 5, V_TICK_BOUND)
        assert min(r.min_abs_d for r in refs) > MIN_ABS_D
        last.append(rec[-1][1])
    for i in range(len(last)):
        for j in range(i):
            assert _rel(last[i], last[j]) > 1e3 * V_TICK_BOUND, (TICK_VARIANTS[i], TICK_VARIANTS[j], _rel(last[i], last[j]))


def test_twelve_joint_init_with_every_parameter_changed(oracle_mod, stn):
    """sim_init(q12, base_height=0.31, **TUNED): the base level at exactly (0, 0, 0.31) on the plane; on the rough field 0.31 above
    the checker's highest ground under the four feet, to 4 ulp, per robot."""
    import qrw_hip

    T, origin, q0, _ = tt._tick_case(stn)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    eng.sim_init(_t(q0[:, 7:]), out, base_height=0.31, **TUNED)
    st = eng.sim_state()
    assert np.array_equal(st["q"][:, :7], np.tile([0.0, 0.0, 0.31, 0.0, 0.0, 0.0, 1.0], (B17, 1)))
    assert np.array_equal(st["q"][:, 7:], q0[:, 7:]) and np.array_equal(out["true_pos"].cpu().numpy(), st["q"][:, :3])
    set_terrain(eng, T, origin=origin)
    eng.sim_init(_t(q0[:, 7:]), out, base_height=0.31, **TUNED)
    st = eng.sim_state()
    want = np.array([stn.init_height(q0[b, 7:], T, origin[b], 0.31) for b in range(B17)])
    assert len(set(want)) == B17 and (want - 0.31).min() > 0.0
    assert np.abs(st["q"][:, 2] - want).max() <= 4 * 2.0 ** -52, np.abs(st["q"][:, 2] - want).max()
    assert np.array_equal(st["q"][:, :2], np.zeros((B17, 2))) and np.array_equal(st["q"][:, 3:7], np.tile(tt.LEVEL, (B17, 1)))
    ref = stn.SimTerrainNumpy(q0[3, 7:], T, origin[3], base_height=0.31, **TUNED)
    assert abs(ref.q[2] - st["q"][3, 2]) <= 4 * 2.0 ** -52


# ------------------------------------------------------------------------------------------------ 2. command stride
def test_result_planes_match_the_checker(oracle_mod, sn):
    """The five commands as the planes of one (B,5,12) tensor (cmd_ld = 60, what the fleet path uses), 20 teacher-forced ticks at
    B = 17 against the checker, and bit for bit the run with five contiguous (B,12) tensors."""
    import qrw_hip

    q0, command = tg._tick_case(sn)
    eng, plain = qrw_hip.Batch(B17), qrw_hip.Batch(B17)
    out, out_p = eng.sim_outputs(), plain.sim_outputs()
    eng.sim_init(_t(q0), out)
    plain.sim_init(_t(q0), out_p)
    refs = [sn.SimNumpy(q0[b]) for b in range(B17)]
    rec, _ = _teacher_forced(eng, out, refs, command, 20, tg.TICK_BOUND, deliver=_planes)
    assert min(r.min_abs_d for r in refs) > MIN_ABS_D
    _same(rec, _run(plain, out_p, command, 20))


def test_padded_command_rows_and_a_stride_too_short(oracle_mod, sn):
    """qrw_sim_step with cmd_ld = 16, five (B,16) buffers whose last four columns hold NaN: bit for bit cmd_ld = 12, no status
    set.  cmd_ld = 11 is refused with a text that says so, and the next valid step works."""
    import torch

    import qrw_hip

    q0, command = tg._tick_case(sn)
    eng, plain = qrw_hip.Batch(B17), qrw_hip.Batch(B17)
    out, out_p = eng.sim_outputs(), plain.sim_outputs()
    eng.sim_init(_t(q0), out)
    plain.sim_init(_t(q0), out_p)
    want = _run(plain, out_p, command, 6)

    def step(k, ld):
        *cmd, f_ext = command(k)
        wide = [np.full((B17, 16), np.nan) for _ in cmd]
        for w, x in zip(wide, cmd):
            w[:, :12] = x
        bufs = [_t(w) for w in wide]
        fe = None if f_ext is None else _t(f_ext)
        rc = eng._lib.qrw_sim_step(eng._handle, *[b.data_ptr() for b in bufs], ld, None if fe is None else fe.data_ptr(),
                                   C.byref(eng._sim_buffers(out)), eng._stream())
        torch.cuda.synchronize()
        return rc

    got = []
    for k in range(5):
        assert step(k, 16) == 0
        got.append(_record(eng, out))
    _same(got, want[:5])
    assert not got[-1][4].any()
    assert step(5, 11) == -1 and eng._lib.qrw_last_error().decode() == "qrw_sim_step: cmd_ld must be >= 12"
    _same([_record(eng, out)], want[4:5])  # (the refused call changed nothing)
    assert step(5, 16) == 0
    _same([_record(eng, out)], want[5:])


# ------------------------------------------------------------------------------------------------ 3. batch position and size
def _spread_over(B, n=B17, seed=83):
    """src (B,): robot i of the large batch is robot src[i] of the n-robot case; a fixed permutation, so that equal robots do
    not sit n apart."""
    return np.random.default_rng(seed).permutation(B) % n


def _rows(command, rows):
    return lambda k: tuple(None if x is None else x[rows] for x in command(k))


@pytest.mark.parametrize("terrain", [False, True])
def test_batch_position_and_size_invariance(oracle_mod, sn, stn, terrain):
    """B = 83 (six blocks, the last holding three quads), robot i given the initial state, commands, wrench and origin of robot
    src[i] of the 17-robot case: over 10 ticks every state item and output of robot i is bit for bit that of robot src[i] in a
    B = 17 handle, and robots 0 and 82 are bit for bit a B = 1 handle."""
    import qrw_hip

    if terrain:
        T, origin, q0, command = tt._tick_case(stn)
    else:
        (q0, command), T, origin = tg._tick_case(sn), None, None
    src = _spread_over(B83)
    assert set(src) == set(range(B17)) and not np.array_equal(src[:B17], src[B17:2 * B17])

    def run(rows):
        eng = qrw_hip.Batch(len(rows))
        out = eng.sim_outputs()
        if terrain:
            set_terrain(eng, T, origin=origin[rows])
        eng.sim_init(_t(q0[rows]), out)
        return _run(eng, out, _rows(command, rows), 10)

    small, large = run(np.arange(B17)), run(src)
    assert not small[-1][4].any() and np.array_equal(large[-1][3], np.full(B83, 10))
    for k, (a, b) in enumerate(zip(large, small)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y[src]), (k, i, np.nonzero(np.any((x != y[src]).reshape(B83, -1), axis=1))[0])
    assert np.abs(small[-1][5 + 8]).sum() > 0  # (robots in contact among them)
    for r in (0, B83 - 1):
        _same([[x[r:r + 1] for x in row] for row in large], run(src[r:r + 1]))


@pytest.mark.parametrize("terrain", [False, True])
def test_forward_dynamics_batch_invariance(oracle_mod, sn, stn, terrain):
    """qrw_test_sim_forward_dynamics with n = 83 on an 83-robot handle against the n = 17 result, bit for bit."""
    import qrw_hip

    src = _spread_over(B83)
    if terrain:
        T, states = tt._fd_states(stn, "rough")
    else:
        states = tg._fd_states(sn)
    q, v, tau, fe = (_stack(states, i) for i in range(4))
    small, large = qrw_hip.Batch(B17), qrw_hip.Batch(B83)
    if terrain:
        set_terrain(small, T, origin=_stack(states, 4))
        set_terrain(large, T, origin=_stack(states, 4)[src])
    a17, f17 = small.test_sim_forward_dynamics(q, v, tau, f_ext=fe)
    a83, f83 = large.test_sim_forward_dynamics(q[src], v[src], tau[src], f_ext=fe[src])
    assert np.array_equal(a83, a17[src]) and np.array_equal(f83, f17[src])
    assert np.all(np.isfinite(a17)) and np.abs(f17).sum() > 0


# ------------------------------------------------------------------------------------------------ 5. freeze and recovery
BY_WRENCH, BY_GAIN, BY_STATE = 3, 8, 12  # the robots poisoned by a NaN in f_ext, +inf in P, a NaN velocity written with set


def _with_wrench(command):
    """_tick_case's commands with a wrench on every tick (the even ticks take the next tick's)."""
    def cmd(k):
        c = list(command(k))
        if c[5] is None:
            c[5] = command(k + 1)[5]
        return tuple(c)

    return cmd


def _poisoned(command):
    def cmd(k):
        c = [x.copy() for x in command(k)]
        if k == 2:
            c[5][BY_WRENCH, 4] = np.nan
            c[0][BY_GAIN, 7] = np.inf
        return tuple(c)

    return cmd


def _run_ticks(eng, out, command, ticks, before=None):
    rec = []
    for k in range(ticks):
        if before is not None:
            before(k)
        rec += _run(eng, out, command, 1, k0=k)
    return rec


def test_every_way_into_the_frozen_state_and_both_ways_out(oracle_mod, sn):
    """Tick 2 of 5 at B = 17: a NaN in robot 3's f_ext, +inf in robot 8's P, a NaN velocity written into robot 12 with
    sim_set_state before the tick.  Each gets status 1 and keeps its state, tick counter and outputs (robot 12: the state as
    written, the outputs of the tick before) through the later clean ticks; the other 14 are bit for bit the clean run.  Out of it:
    sim_set_state(status=0) with the clean twin's state continues bit for bit with the twin; sim_init clears every status and
    the ticks after it are those of a fresh handle."""
    import qrw_hip

    q0, command = tg._tick_case(sn, seed=5)
    command = _with_wrench(command)
    twin, eng = qrw_hip.Batch(B17), qrw_hip.Batch(B17)
    out_t, out = twin.sim_outputs(), eng.sim_outputs()
    twin.sim_init(_t(q0), out_t)
    eng.sim_init(_t(q0), out)
    clean = _run_ticks(twin, out_t, command, 5)
    written = {}

    def write_nan(k):
        if k == 2:
            st = eng.sim_state()
            st["v"][BY_STATE, 4] = np.nan
            eng.sim_set_state(st["q"], st["v"], st["prev_o_imuVel"], tick=st["tick"], status=st["status"])
            written.update(st)

    bad = _run_ticks(eng, out, _poisoned(command), 5, before=write_nan)
    frozen = [BY_WRENCH, BY_GAIN, BY_STATE]
    others = np.setdiff1d(np.arange(B17), frozen)
    _same(clean, bad, rows=others)
    _same(clean[:2], bad[:2])
    assert not clean[-1][4].any()
    for k in range(2, 5):
        status = bad[k][4]
        assert np.array_equal(np.nonzero(status)[0], frozen) and np.all(status[frozen] == 1), (k, status)
        for r in frozen:
            for i, (x, y) in enumerate(zip(bad[k], bad[1])):
                if i == 4:
                    continue
                if r == BY_STATE and i < 3:  # q, v, prev_o_imuVel: as written, the NaN included
                    y = [written[n] for n in tg.STATE_KEYS]
                    assert np.array_equal(x[r], y[i][r], equal_nan=True), (k, r, i)
                    continue
                assert np.array_equal(x[r], y[r]) and np.all(np.isfinite(x[r])), (k, r, i)
    assert np.isnan(bad[4][1][BY_STATE, 4]) and np.array_equal(bad[4][3][frozen], [2, 2, 2])
    # out, one: the twin's state with status 0 -- all 17 continue with the twin
    st = twin.sim_state()
    eng.sim_set_state(st["q"], st["v"], st["prev_o_imuVel"], tick=st["tick"], status=0)
    revived = _run(eng, out, command, 3, k0=5)
    _same(revived, _run(twin, out_t, command, 3, k0=5))
    assert not revived[-1][4].any() and np.array_equal(revived[-1][3], np.full(B17, 8))
    assert not np.array_equal(revived[0][0][frozen], revived[-1][0][frozen])  # (they move again)
    # out, two: poisoned again, then sim_init
    _run(eng, out, _poisoned(command), 1, k0=2)
    assert np.array_equal(np.nonzero(eng.sim_state()["status"])[0], [BY_WRENCH, BY_GAIN])
    eng.sim_init(_t(q0), out)
    assert not eng.sim_state()["status"].any()
    fresh = qrw_hip.Batch(B17)
    out_f = fresh.sim_outputs()
    fresh.sim_init(_t(q0), out_f)
    _same(_run(eng, out, command, 5), _run(fresh, out_f, command, 5))


def test_nan_in_q_init_freezes_that_robot_at_init(oracle_mod, sn):
    """A NaN in robot 7's q_init: status 1 from the initialisation on and nothing else of it stored -- its state rows and its rows of
    the output buffers keep what they held (zero in a handle never initialised before, the last tick's after a run), as
    include/qrw_hip.h says; the others' first measurement and their ticks are bit for bit those of the clean initialisation."""
    import qrw_hip

    q0, command = tg._tick_case(sn, seed=6)
    bad_q = q0.copy()
    bad_q[7, 9] = np.nan
    others = np.arange(B17) != 7
    clean, eng = qrw_hip.Batch(B17), qrw_hip.Batch(B17)
    out_c, out = clean.sim_outputs(), eng.sim_outputs()
    clean.sim_init(_t(q0), out_c)
    eng.sim_init(_t(bad_q), out)
    first_c, first = _record(clean, out_c), _record(eng, out)
    _same([first_c], [first], rows=others)
    assert first[4][7] == 1 and not first[4][others].any()
    assert all(not x[7].any() for i, x in enumerate(first) if i != 4)  # (a new handle: zero state, zeroed outputs)
    run_c, run = _run(clean, out_c, command, 3), _run(eng, out, command, 3)
    _same(run_c, run, rows=others)
    assert all(np.array_equal(x[7], y[7]) for x, y in zip(run[-1], first))  # (frozen for good)
    # after a run: a clean re-initialisation revives it; a second poisoned one leaves its rows at the last tick's values
    eng.sim_init(_t(q0), out)
    _same([_record(eng, out)], [first_c])
    last = _run(eng, out, command, 3)[-1]
    eng.sim_init(_t(bad_q), out)
    again = _record(eng, out)
    _same([first_c], [again], rows=others)
    assert again[4][7] == 1 and all(np.array_equal(x[7], y[7]) for i, (x, y) in enumerate(zip(again, last)) if i != 4)
    assert again[3][7] == 3 and again[0][7].any()


# ------------------------------------------------------------------------------------------------ 6. momentum in flight
def test_momentum_in_flight_on_the_device(oracle_mod, sn):
    """tests/test_sim_cpu.py's momentum check on the device, 17 tumbling robots in flight (seeds 100..116), zero gains and torques,
    25 ticks at 8 and at 16 sub-steps: the drift of the horizontal linear momentum and of the vertical angular momentum halves
    (factor in [1.9, 2.1]) for every robot.  Only oracle.crba enters the yardstick: this does not rest on the checker's h."""
    import torch

    import qrw_hip
    from test_sim_cpu import momentum_drift

    states = [sn.tumbling_state(np.random.default_rng(100 + b)) for b in range(B17)]
    q, v = _stack(states, 0), _stack(states, 1)
    eng = qrw_hip.Batch(B17)
    out = eng.sim_outputs()
    zero = _t(np.zeros((B17, 12)))
    final = {}
    for substeps in (8, 16):
        eng.sim_init(_t(q), out, substeps=substeps)
        eng.sim_set_state(q, v, np.zeros((B17, 3)))
        for _ in range(25):
            eng.sim_step(zero, zero, zero, zero, zero, out)
        torch.cuda.synchronize()
        st = eng.sim_state()
        assert not st["status"].any() and np.array_equal(st["tick"], np.full(B17, 25)) and st["q"][:, 2].min() > 0.9
        assert not out["contact_forces"].cpu().numpy().any()
        final[substeps] = st
    for b in range(B17):
        lin8, ang8, mass8 = momentum_drift(sn, q[b], v[b], 8, step=lambda *_: (final[8]["q"][b], final[8]["v"][b]))
        lin16, ang16, mass16 = momentum_drift(sn, q[b], v[b], 16, step=lambda *_: (final[16]["q"][b], final[16]["v"][b]))
        print("  robot %2d: linear drift %.3g / %.3g = %.4f, angular-z drift %.3g / %.3g = %.4f, mass %.5f %.5f"
              % (b, lin8, lin16, lin8 / lin16, ang8, ang16, ang8 / ang16, mass8, mass16))
        assert 1.9 <= lin8 / lin16 <= 2.1 and 1.9 <= ang8 / ang16 <= 2.1, (b, lin8 / lin16, ang8 / ang16)
