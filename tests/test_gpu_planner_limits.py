"""GPU tests of the batched planners at the limits of the gait table (planner_kernel.hip, control_pre_quad_kernel, the estimator's
read of the gait masks) against the oracle: a period that fills the table, a walk that fills it, an odd number of rows per
period, the widest table (N_gait 63, a 62-row trot), the tightest one (n_steps + 1 = N_gait); the refusals of the size rule;
and a second block of robots.  Cases, sequences, the oracle's runs and the bounds come from tests/planner_cases.py.

The refusals are safe to ask for on a GPU only because qrw_planner_init refuses BEFORE it launches anything: that is what
tests/test_gait_masks_cpu.py establishes on the CPU, and what test_refusals_leave_the_handle_uninitialised relies on."""
import numpy as np
import pytest

import planner_cases as pc

pytestmark = pytest.mark.gpu

Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])


def _t(x, dtype=np.float64):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _where(got, ref):
    """(robot, row, column) of the largest difference, with the two values: for the message of a failed comparison."""
    i = np.unravel_index(np.abs(got - ref).argmax(), ref.shape)
    return tuple(int(x) for x in i), float(got[i]), float(ref[i])


def compare_state(eng, ref, case, k, worst):
    """Items 0-6 of qrw_planner_get_host (past / current / desired gait, newPhase, is_static, remainingTime, number of swing feet)
    exactly, and item 17 (the trajectory generator's target) within the bound of `target`, for every robot."""
    Ng = pc.CASES[case]["N_gait"]
    for b, (past, des, ft_target) in enumerate(ref["state"][k]):
        assert np.array_equal(eng.planner_get(0, Ng * 4, b).reshape(Ng, 4), past), (case, k, b)
        assert np.array_equal(eng.planner_get(1, Ng * 4, b).reshape(Ng, 4), ref["gait"][k, b]), (case, k, b)
        assert np.array_equal(eng.planner_get(2, Ng * 4, b).reshape(Ng, 4), des), (case, k, b)
        flags = [eng.planner_get(item, 1, b)[0] for item in (3, 4, 5, 6)]
        assert np.array_equal(flags, ref["flags"][k, b]), (case, k, b, flags, ref["flags"][k, b])
        e = pc.err(eng.planner_get(17, 12, b).reshape(3, 4), ft_target)
        worst["ft_target"] = max(worst.get("ft_target", 0.0), e)
        assert e <= pc.bound(case, "ft_target"), (case, k, b, "ft_target", e)


def run_against_the_oracle(oracle_mod, case, floats=pc.FLOAT_OUTPUTS, extra=None):
    """The case's whole sequence through qrw_planner_step with per-robot code tensors: gait and contacts exactly, every
    floating-point output of every iteration within its bound, the state items every STATE_EVERY iterations.  Returns the
    device's worst err per output.  extra(k, out, ref): further checks on the raw outputs of iteration k."""
    import torch

    import qrw_hip

    seq, ref = pc.sequence(case), pc.oracle_run(oracle_mod, case)
    K, B = seq["code"].shape
    eng = qrw_hip.Batch(B, **pc.handle_kwargs(case))
    eng.planner_init(**pc.planner_init_kwargs(case))
    dev = {n: torch.from_numpy(v).cuda() for n, v in seq.items()}
    worst, out = dict.fromkeys(floats, 0.0), None
    for k in range(K):
        out = eng.planner_step(k, dev["q7"][k], dev["hv"][k], dev["vref"][k], dev["code"][k], out=out)
        o = {n: v.cpu().numpy() for n, v in out.items()}
        assert np.array_equal(o["gait"], ref["gait"][k]), (case, k)
        assert np.array_equal(o["contacts"], ref["gait"][k][:, 0]), (case, k)
        got = dict(xref=o["xref"], fsteps=o["fsteps"], target=o["target"], pos=o["feet_pva"][:, 0], vel=o["feet_pva"][:, 1], acc=o["feet_pva"][:, 2])
        for name in floats:
            e = pc.err(got[name], ref[name][k])
            worst[name] = max(worst[name], e)
            assert e <= pc.bound(case, name), (case, k, name, e, pc.bound(case, name), _where(got[name], ref[name][k]))
        if extra is not None:
            extra(k, got, ref)
        if k in ref["state"]:
            compare_state(eng, ref, case, k, worst)
    eng.close()
    print("%s: %d iterations; device err / bound: %s" % (case, K, "  ".join("%s %.2e / %.2e" % (n, w, pc.bound(case, n)) for n, w in worst.items())))
    return worst


@pytest.mark.parametrize("case", pc.LIMITS)
def test_planner_at_the_table_limits_matches_oracle(oracle_mod, case):
    """B = 9, every robot with its own gait changes (codes 1..5, static and away again, on rolling and non-rolling iterations), at
    least two of the longest periods past the last change.  Measured on the device (err, see planner_cases; the bound is 100 x the
    oracle's spread, planner_cases.SPREAD), worst over the run:
        full20        xref 2.2e-16  fsteps 8.9e-16  target 8.9e-16  pos 5.8e-10  vel 1.8e-09  acc 2.1e-08
        walk_fills    xref 1.7e-16  fsteps 2.1e-15  target 2.2e-15  pos 1.7e-10  vel 3.5e-10  acc 1.9e-09
        odd           xref 2.2e-16  fsteps 7.8e-16  target 1.0e-15  pos 1.5e-10  vel 4.5e-10  acc 8.8e-09
        wide          xref 1.7e-16  fsteps 1.3e-15  target 1.3e-15  pos 1.7e-07  vel 4.4e-07  acc 8.9e-07
        tight         xref 1.1e-16  fsteps 1.0e-15  target 1.0e-15  pos 2.0e-12  vel 2.7e-11  acc 3.7e-10"""
    c = pc.CASES[case]
    assert pc.rows_needed(case) <= c["N_gait"] and c["N"] + 1 <= c["N_gait"]
    ref = pc.oracle_run(oracle_mod, case)
    live = ref["gait"].any(-1).sum(-1)
    assert (live == c["N"]).all()  # the current gait keeps n_steps live rows through every change
    if case in ("full20", "walk_fills"):  # ... and the desired one does fill the table at some point
        assert any(des.any(-1).sum() == c["N_gait"] for st in ref["state"].values() for _, des, _ in st)
    if case == "wide":
        assert any(des.any(-1).sum() == 62 for st in ref["state"].values() for _, des, _ in st)
        assert any(past.any(-1).sum() == 33 for st in ref["state"].values() for past, _, _ in st)
    run_against_the_oracle(oracle_mod, case)


def test_estimator_reads_the_widest_gait_masks(oracle_mod, synth_mod):
    """qrw_estimator_step with d_gait = d_goals = NULL on the `wide` handle (63 rows, masks up to bit 62) against the same step
    given the planner's gait and foot positions explicitly, on a second handle stepped alike: bit for bit, 560 ticks.  The first
    row that differs from row 0 runs from 1 to 31 (a 62-row trot), and while a robot stands (code 4: 32 equal rows, zero rows
    after them) it is the first zero row, 32."""
    import torch

    import qrw_hip

    case = "wide"
    seq = pc.sequence(case)
    K, B = 560, seq["code"].shape[1]
    engs = [qrw_hip.Batch(B, **pc.handle_kwargs(case)) for _ in range(2)]
    for e in engs:
        e.planner_init(**pc.planner_init_kwargs(case))
        e.estimator_init(0.22294615)
    sen = synth_mod.SyntheticSensors(B, 11, dt=pc.CASES[case]["dt_wbc"])
    dev = {n: torch.from_numpy(v).cuda() for n, v in seq.items()}
    # before the first planner step: the gait and foot positions of qrw_planner_init
    gait = _t(np.stack([pc.oracle_planner(oracle_mod, case).gaits()[1]] * B))
    goals = _t(np.stack([pc.DEFAULT_SHOULDERS] * B))
    pout, firsts = [None, None], set()
    for k in range(K):
        s = [_t(v) for v in (sen.step(k)[n] for n in ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes"))]
        a = engs[0].estimator_step(*s)
        b = engs[1].estimator_step(*s, gait=gait, goals=goals)
        for n in a:
            assert torch.equal(a[n], b[n]), (k, n)
        for i, e in enumerate(engs):
            pout[i] = e.planner_step(k, dev["q7"][k], dev["hv"][k], dev["vref"][k], dev["code"][k], out=pout[i])
        gait, goals = pout[1]["gait"], pout[1]["feet_pva"][:, 0].contiguous()
        g = gait.cpu().numpy()
        for r in range(B):
            differ = np.nonzero((g[r] != g[r, 0]).any(1))[0]
            firsts.add(int(differ[0]) if len(differ) else 63)
    assert {1, 31, 32} <= firsts, sorted(firsts)
    for e in engs:
        e.close()


REFUSED = [dict(n_steps=16, N_gait=63, T_gait=1.24), dict(n_steps=16, N_gait=63, T_gait=1.26), dict(n_steps=12, N_gait=15, T_gait=0.30),
           dict(n_steps=16, N_gait=18, T_gait=0.36)]


def test_refusals_leave_the_handle_uninitialised(oracle_mod):
    """Tables the size rule refuses (a 64-row walk or trot in 63 rows, a 16-row trot in 15, a 20-row walk in 18): planner_init
    raises ValueError, a planner_step on the refused handle answers "not initialised", and a fresh default handle created
    afterwards still matches the oracle for 20 iterations.  Nothing is launched for a refused table (tests/test_gait_masks_cpu.py
    shows the refusal on the CPU; qrw_planner_init tests the rule ahead of its launch)."""
    import torch

    import libquadruped_reactive_walking as lqrw
    import qrw_hip

    rng = np.random.default_rng(31)
    for kw in REFUSED:
        eng = qrw_hip.Batch(2, **kw)
        assert not eng.gait_table_fits()  # (the library's rule, asked without a launch: planner_init below is never reached otherwise)
        with pytest.raises(ValueError, match="Sizes of matrices are too small"):
            eng.planner_init()
        with pytest.raises(qrw_hip.QrwError, match="not initialised"):
            eng.planner_step(0, _t(np.zeros((2, 7))), _t(np.zeros((2, 6))), _t(np.zeros((2, 6))), 0)
        eng.close()
        with pytest.raises(ValueError, match="Sizes of matrices are too small"):  # the drop-in class: the same -3 through its own handle
            lqrw.Gait().initialize(0.02, kw["T_gait"], kw["n_steps"] * 0.02, kw["N_gait"])
    assert qrw_hip.Batch(2, 16).gait_table_fits() and qrw_hip.Batch(2, 16, N_gait=20, T_gait=0.40).gait_table_fits()
    B = 3
    eng = qrw_hip.Batch(B, 16)
    eng.planner_init()
    refs = [oracle_mod.Planner() for _ in range(B)]
    vref = rng.uniform(-0.5, 0.5, (B, 6)) * np.array([2, 1, 0, 0, 0, 1.4])
    for k in range(20):
        q7 = np.tile([0.0, 0.0, 0.2229, 0.0, 0.0, 0.0, 1.0], (B, 1))
        q7[:, :2] = rng.uniform(-1, 1, (B, 2))
        hv = vref + rng.uniform(-0.1, 0.1, (B, 6))
        o = {n: v.cpu().numpy() for n, v in eng.planner_step(k, _t(q7), _t(hv), _t(vref), 3 if k == 7 else 0).items()}
        for b, r in enumerate(refs):
            r.step(k, q7[b], hv[b], vref[b], 3 if k == 7 else 0)
            f, _, otg = r.footsteps()
            pos, vel, acc, _, _ = r.feet()
            assert np.array_equal(o["gait"][b], r.gaits()[1]), (k, b)
            assert np.allclose(o["xref"][b], r.xref(), rtol=1e-12, atol=1e-13) and np.allclose(o["fsteps"][b], f, rtol=1e-11, atol=1e-13), (k, b)
            assert np.allclose(o["target"][b], otg, rtol=1e-11, atol=1e-13), (k, b)
            assert np.allclose(o["feet_pva"][b], [pos, vel, acc], rtol=1e-9, atol=1e-8), (k, b)
    eng.close()


def _block_inputs(rng, B, K):
    vref = rng.uniform(-0.5, 0.5, (B, 6)) * np.array([2, 1, 0, 0, 0, 1.4])
    vref[::7, 5] = 0.0
    q7 = np.zeros((K, B, 7))
    q7[..., :2], q7[..., 2] = rng.uniform(-1, 1, (K, B, 2)), 0.2229 + rng.uniform(-0.01, 0.01, (K, B))
    quat = np.concatenate([rng.uniform(-0.03, 0.03, (K, B, 2)), rng.uniform(-0.2, 0.2, (K, B, 1)), np.ones((K, B, 1))], -1)
    q7[..., 3:] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    hv = vref + rng.uniform(-0.1, 0.1, (K, B, 6))
    code = np.zeros((K, B), np.int32)
    code[23] = 1 + np.arange(B) % 5
    return q7, hv, vref, code


STATE_ITEMS = ((0, 80), (1, 80), (2, 80), (3, 1), (4, 1), (5, 1), (6, 1), (7, 12), (8, 12), (9, 12), (10, 12), (11, 12), (12, 4), (13, 4),
               (14, 240), (15, 12), (16, 7), (17, 12), (18, 2))


def _same_state(big, small, pairs):
    for bb, sb in pairs:
        for item, n in STATE_ITEMS:
            assert np.array_equal(big.planner_get(item, n, bb), small.planner_get(item, n, sb)), (bb, sb, item)


def test_second_block_through_planner_step():
    """planner_kernel runs 64 robots per block: B = 83 against B = 17 and B = 1, bit for bit over 60 iterations with one
    per-robot code change -- robots 0..16 of the large handle equal the small one's, robot 82 (the second block's last lane)
    equals a one-robot handle fed its inputs -- every output of every iteration and every state item at the end."""
    import torch

    import qrw_hip

    K, rng = 60, np.random.default_rng(83)
    q7, hv, vref, code = _block_inputs(rng, 83, K)
    sel = {83: slice(0, 83), 17: slice(0, 17), 1: slice(82, 83)}
    engs = {B: qrw_hip.Batch(B, 16) for B in sel}
    for e in engs.values():
        e.planner_init()
    for k in range(K):
        o = {B: e.planner_step(k, _t(q7[k, sel[B]]), _t(hv[k, sel[B]]), _t(vref[sel[B]]), _t(code[k, sel[B]], np.int32)) for B, e in engs.items()}
        for n in o[83]:
            assert torch.equal(o[83][n][:17], o[17][n]), (k, n)
            assert torch.equal(o[83][n][82:], o[1][n]), (k, n)
    _same_state(engs[83], engs[17], [(0, 0), (16, 16)])
    _same_state(engs[83], engs[1], [(82, 0)])
    assert engs[83].planner_get(1, 80, 82).any() and not np.array_equal(engs[83].planner_get(1, 80, 82), engs[83].planner_get(1, 80, 81))
    for e in engs.values():
        e.close()


def test_second_block_through_control_pre():
    """The same through qrw_control_pre (control_pre_quad_kernel: 16 robots per block, B = 83 is six blocks, the last one partly
    filled), on solving and non-solving iterations."""
    import torch

    import qrw_hip

    K, N, rng = 60, 16, np.random.default_rng(84)
    _, hv, vref, code = _block_inputs(rng, 83, K)
    sel = {83: slice(0, 83), 17: slice(0, 17), 1: slice(82, 83)}
    engs = {B: qrw_hip.Batch(B, N) for B in sel}
    for B, e in engs.items():
        e.planner_init()
        e.controller_init(_t(np.tile(Q_INIT, (B, 1))))
    qf = np.zeros((83, 19))
    qf[:, 2], qf[:, 6], qf[:, 7:] = 0.2229, 1.0, Q_INIT
    x_f = np.zeros((83, 24, N))
    x_f[:, 2, :], x_f[:, 14::3, :] = 0.2229, 6.0
    x_f += rng.uniform(0, 0.1, x_f.shape)
    outs = dict.fromkeys(sel)
    for k in range(K):
        vf = np.zeros((83, 18))
        vf[:, :6] = hv[k]
        vf[:, 6:] = rng.uniform(-0.3, 0.3, (83, 12))
        rpy = rng.uniform(-0.02, 0.02, (83, 3))
        qf[:, 0:2] += 0.002 * vref[:, 0:2]
        solve = k % 10 == 0
        for B, e in engs.items():
            s = sel[B]
            outs[B] = e.control_pre(k, _t(vref[s]), _t(qf[s]), _t(vf[s]), _t(rpy[s]), _t(code[k, s], np.int32),
                                    x_f_mpc=(None if solve else _t(x_f[s])), out=outs[B], mpc_inputs=solve)
        for n in outs[83]:
            if (not solve and n in ("fsteps", "gait")) or (solve and n in ("x_f_wbc", "q_wbc", "b_v", "f_cmd", "feet_cmd")):
                continue

            def cut(t, robots):
                t = t[:, robots] if n == "feet_cmd" else t[robots]  # (feet_cmd is (3, B, 3, 4))
                return t[:, :, :2] if (n == "xref" and not solve) else t

            assert torch.equal(cut(outs[83][n], slice(0, 17)), cut(outs[17][n], slice(None))), (k, n)
            assert torch.equal(cut(outs[83][n], slice(82, 83)), cut(outs[1][n], slice(None))), (k, n)
    # (K - 1 = 59 does not solve: rows >= 2 of the quad form's footstep table wait for the next solving iteration, on every handle alike)
    _same_state(engs[83], engs[17], [(0, 0), (16, 16)])
    _same_state(engs[83], engs[1], [(82, 0)])
    for e in engs.values():
        e.close()
