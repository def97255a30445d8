"""The ADMM loop of the MPC solve runs in check-free blocks: an outer round is [factorisation, if asked for] + 25 plain
iterations + the check on the 25th iterate, and every decision that leaves or redirects the loop is a scalar
(csrc/mpc_kernel.hip, docs/HISTORY.md 6b).  No arithmetic instruction changed, so the solver must reproduce the build before
the change BIT FOR BIT -- results, iteration counts, status, rho -- and keep its parity with the CPU oracle.  The cases are the
loop's edges, not the workload: an exit at the very first check, rho refactorisations followed by further intervals, solves
that end exactly on an adaptive-rho test, the max-iter exit with its 10x re-check, the runtime-horizon instantiation
(N = 12, N = 5), and N = 32 in its plain, time-sliced and sequence forms.

The fixtures tests/golden/loop_blocks/loop_blocks_parent_*.npz were recorded on an MI355X from the build of the parent commit
by tests/golden/make_loop_blocks_parent.py, which runs the cases below.  (A directory of their own: tests/test_golden.py takes
every tests/golden/*.npz for an oracle fixture of its schema.)  Every seed was chosen with the CPU oracle alone."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_blocks")
SOLVED, SOLVED_INACCURATE, MAX_ITER = 1, 2, -2

# name -> (generator, N, batch, gaits, seed0, num_iter of every call): the inputs of call c are the generator's step(c), so a
# repeated number solves the same inputs again on the warm-started handle.  What each case is for (oracle, CPU):
#   n16   call 0 cold (rho 0.1 -> ~4e-4: refactorisations, then further intervals), instance 3 ends at 600 = 3 x 200; calls 1, 2
#         run to 1750 iterations; the repeat of call 2 ends at the first check (25) in every instance
#   n12   runtime horizon: an instance ends at exactly 200 in calls 1 and 2, rho updates in calls 1 and 2; repeat: 25
#   n5    runtime horizon, short chains: rho updates in calls 1 and 2; repeat: 25
#   n32   two wavefronts: 2875 iterations in call 1, instance 3 runs into max_iter in call 2 and passes the 10x re-check
#         (solved inaccurate); the repeat of call 2 takes 175 iterations there and 25 elsewhere
#   maxit random contact tables (synth.RandomContactTables, the generator of tests/test_gpu_mpc_random_tables.py) at N = 32 -- at
#         N = 16 none of 4000 oracle solves of that generator reaches max_iter: three solves end at max_iter, two fail the 10x
#         re-check (max iterations) and one passes it (solved inaccurate)
CASES = {
    "n16": ("synth", 16, 8, ("walk", "trot", "bounding"), 20800000, (0, 1, 2, 2)),
    "n12": ("synth", 12, 8, ("trot", "walk"), 20800000, (0, 1, 2, 2)),
    "n5": ("synth", 5, 8, ("trot", "walk"), 20800000, (0, 1, 2, 2)),
    "n32": ("synth", 32, 4, ("walk", "trot", "bounding"), 20800001, (0, 1, 2, 2)),
    "maxit": ("rand", 32, 4, None, 20820200, (0, 1, 2)),
}


def _n_gait(N):
    return max(20, N + 4)


def case_inputs(name):
    import synth

    kind, N, B, gaits, seed0, calls = CASES[name]
    if kind == "synth":
        gen = synth.SyntheticBatch(B, N, N_gait=_n_gait(N), gaits=gaits, seed0=seed0)
    else:
        gen = synth.RandomContactTables(B, N, N_gait=_n_gait(N), seed0=seed0)
    steps = {c: gen.step(c) for c in sorted(set(calls))}
    return [(c, steps[c]["xref"], steps[c]["fsteps"]) for c in calls]


def _plain_engine(N, B):
    """A handle whose N > 16 solves take the plain launch (the time slicing is switched off for it)."""
    import qrw_hip

    old = os.environ.get("QRW_PREEMPT_CHUNK")
    os.environ["QRW_PREEMPT_CHUNK"] = "0"
    try:
        return qrw_hip.Batch(B, n_steps=N, N_gait=_n_gait(N), T_gait=0.02 * N)
    finally:
        if old is None:
            del os.environ["QRW_PREEMPT_CHUNK"]
        else:
            os.environ["QRW_PREEMPT_CHUNK"] = old


def run_case(name):
    """Every call's result (calls, B, 24, N) float64, iteration counts, status (int) and rho (float64), each (calls, B)."""
    _, N, B, _, _, _ = CASES[name]
    eng = _plain_engine(N, B)
    res = dict(out=[], iters=[], status=[], rho=[])
    for c, xref, fsteps in case_inputs(name):
        res["out"].append(eng.mpc_solve_host(xref, fsteps, c).copy())
        st = eng.mpc_stats()
        for key in ("iters", "status", "rho"):
            res[key].append(np.array(st[key]).copy())
    eng.close()
    return {k: np.stack(v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The same calls through the strict build of the CPU oracle, computed once and shared (read-only) by the tests."""
    import oracle

    oracle.build()
    _, N, B, _, _, _ = CASES[name]
    ref = oracle.MPCBatch(B, 0.02, N, 0.02 * N, _n_gait(N), fast=False)
    res = dict(out=[], iters=[], status=[], rho=[])
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    for c, xref, fsteps in case_inputs(name):
        res["out"].append(ref.run(c, xref, fsteps, threads).copy())
        it, st = ref.iters()
        res["iters"].append(it.copy())
        res["status"].append(st.copy())
        res["rho"].append(np.array([ref._lib.mpc_oracle_rho(h) for h in ref._hs]))
    res = {k: np.stack(v) for k, v in res.items()}
    for v in res.values():
        v.setflags(write=False)
    return res


def rel_err(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-12)


def oracle_parity(got, ref):
    """The usual parity, in the very expressions of run_sequence (tests/test_gpu_mpc.py:44-49): identical iteration counts and
    status, rho np.isclose(rtol=1e-9), results to 1e-4 relative.  Prints the worst deviations (the parent build's own, printed by
    the generator when it recorded the fixtures: rho 9e-11 .. 7.0e-9 relative, results 4e-13 .. 2.2e-11)."""
    assert np.array_equal(got["iters"], ref["iters"]), (got["iters"].tolist(), ref["iters"].tolist())
    assert np.array_equal(got["status"], ref["status"])
    rho_dev = np.abs(got["rho"] / ref["rho"] - 1).max()
    worst = 0.0
    for c in range(got["out"].shape[0]):
        for b in range(got["out"].shape[1]):
            worst = max(worst, rel_err(got["out"][c, b, :12], ref["out"][c, b, :12]), rel_err(got["out"][c, b, 12:], ref["out"][c, b, 12:]))
    print("oracle parity: rho to %.2e relative, results to %.2e" % (rho_dev, worst))
    assert np.isclose(got["rho"], ref["rho"], rtol=1e-9).all(), rho_dev
    assert worst < 1e-4, worst
    return rho_dev, worst


def rho_updated(rec):
    """(calls, B) bool: rho left the call different from how it entered it -- only the adaptive-rho test changes it (the first
    call enters with OSQP's 0.1)."""
    before = np.concatenate([np.full((1,) + rec["rho"].shape[1:], 0.1), rec["rho"][:-1]])
    return rec["rho"] != before


@pytest.mark.parametrize("name", sorted(CASES))
def test_bitwise_identical_to_the_parent_build_and_at_parity_with_the_oracle(name):
    want = np.load(os.path.join(GOLDEN, "loop_blocks_parent_%s.npz" % name))
    got = run_case(name)
    print("%s: iteration counts %s, status %s" % (name, got["iters"].tolist(), got["status"].tolist()))
    assert want["out"].dtype == np.float64 and got["out"].dtype == np.float64
    assert np.array_equal(got["iters"], want["iters"])
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["rho"], want["rho"])
    assert np.array_equal(got["out"], want["out"], equal_nan=True)
    oracle_parity(got, oracle_case(name))


def test_recordings_hold_the_edges_of_the_loop():
    """What the cases are for is in the RECORDINGS (and so, by the test above, in what this build does)."""
    rec = {name: np.load(os.path.join(GOLDEN, "loop_blocks_parent_%s.npz" % name)) for name in CASES}
    for name in ("n16", "n12", "n5"):
        # exit at the first check: the warm-started repeat of the last call
        assert (rec[name]["iters"][3] == 25).all() and (rec[name]["status"][3] == SOLVED).all(), name
    for name in CASES:
        # refactorisation: a rho update, and further intervals behind it (the update is decided at a multiple of 200; a solve
        # that goes on ends later than that)
        upd = rho_updated(rec[name])
        assert (upd & (rec[name]["iters"] > 200) & (rec[name]["iters"] % 200 != 0)).any(), name
    for name in ("n16", "n12"):
        # a solve that ends exactly on an adaptive-rho test
        it = rec[name]["iters"]
        assert ((it % 200 == 0) & (it < 4000)).any(), name
    # max_iter: the last interval is a full one, the 10x re-check decides the status -- both outcomes
    it, st = rec["n32"]["iters"], rec["n32"]["status"]
    assert (it == 4000).any() and set(st[it == 4000].tolist()) == {SOLVED_INACCURATE}
    assert (it[it != 4000] % 25 == 0).all() and (st[it != 4000] == SOLVED).all()
    it, st = rec["maxit"]["iters"], rec["maxit"]["status"]
    assert set(st[it == 4000].tolist()) == {SOLVED_INACCURATE, MAX_ITER}


def test_n32_time_sliced_launch_equals_the_plain_one(monkeypatch):
    """mpc_solve_kernel<2, true, false, true>: slices of 200 iterations (every resume is interval-aligned) on the smallest batch
    the slicing accepts, against the plain launch of the same inputs: exact equality, and at least one solve is resumed."""
    import qrw_hip
    import synth

    N, B = 32, 2
    sb = synth.SyntheticBatch(B, N, N_gait=_n_gait(N), gaits=("walk", "trot", "bounding"), seed0=20800000)
    plain = _plain_engine(N, B)
    monkeypatch.setenv("QRW_PREEMPT_MIN_BATCH", "1")
    monkeypatch.setenv("QRW_PREEMPT_CHUNK", "200")
    sliced = qrw_hip.Batch(B, n_steps=N, N_gait=_n_gait(N), T_gait=0.02 * N)
    resumed = 0
    for s in range(2):
        d = sb.step(s)
        a = plain.mpc_solve_host(d["xref"], d["fsteps"], s)
        b = sliced.mpc_solve_host(d["xref"], d["fsteps"], s)
        sa, sb_ = plain.mpc_stats(), sliced.mpc_stats()
        for key in ("iters", "status", "rho"):
            assert np.array_equal(sa[key], sb_[key]), (s, key)
        assert np.array_equal(a, b), s
        st = sliced.mpc_slice_stats()
        assert st["chunk"] == 200 and st["finished"] == B, st  # the time-sliced kernel did run
        # resumed: a taker workgroup took a parked solve (a solve that merely goes on in place behind a refused park would
        # have more than 200 iterations too, but would never enter the kernel with the loop state of a parked one)
        print("call %d: iterations %s, parks per level %s, takers %d" % (s, sb_["iters"].tolist(), st["parks_per_level"].tolist(), st["takers"]))
        assert st["takers"] <= st["parks_per_level"].sum()
        resumed += int(st["takers"])
    assert resumed > 0, "no parked solve was taken up by another workgroup"
    plain.close()
    sliced.close()


@pytest.mark.parametrize("N", [16, 32])
def test_sequence_launch_equals_plain_calls(N):
    """mpc_solve_kernel<NW, true, true> (K = 2 calls of 2 instances in one launch) against K plain launches: exact equality."""
    import torch

    import synth

    B, K = 2, 2
    sb = synth.SyntheticBatch(B, N, N_gait=_n_gait(N), gaits=("trot", "walk"), seed0=20800000 + 300 + N)
    steps = [sb.step(s) for s in range(K)]
    a, b = _plain_engine(N, B), _plain_engine(N, B)
    dev = torch.device("cuda", 0)
    xs = torch.from_numpy(np.stack([st["xref"] for st in steps])).to(dev)
    fs = torch.from_numpy(np.stack([st["fsteps"] for st in steps])).to(dev)
    ref_out, ref_it = [], []
    for s in range(K):
        ref_out.append(a.mpc_solve(xs[s], fs[s], s).cpu().numpy())
        ref_it.append(a.mpc_stats()["iters"].copy())
    its = torch.zeros((K, B), dtype=torch.int32, device=dev)
    out = b.mpc_solve_sequence(xs, fs, 0, iters=its)
    torch.cuda.synchronize()
    assert not b.mpc_sequence_timed_out()
    assert np.array_equal(its.cpu().numpy(), np.stack(ref_it))
    assert np.array_equal(out.cpu().numpy(), np.stack(ref_out))
    sa, sb_ = a.mpc_stats(), b.mpc_stats()
    for key in ("iters", "status", "rho"):
        assert np.array_equal(sa[key], sb_[key]), key
    a.close()
    b.close()
