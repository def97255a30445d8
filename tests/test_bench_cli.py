"""bench.py's command line: a plain run is the headline figure alone, `--full` is behind its flag, `--dump-outputs DIR`
writes the last timed step's results, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "accuracy", "torque_max_abs_err", "two_stream_groups", "pipelined_sequence", "closed_loop_sequence",
             "secondary_ratio_1_10", "secondary_ratio_1_10_async", "realtime_slot", "batch_1", "batch_256_mpc_only",
             "config4_n32_mixed")


def _bench(env, *flags):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(flags), env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_plumbing_on_the_cpu_stub(tmp_path):
    """QRW_BENCH_STUB=1 (no kernels, the line's value means nothing): `--steps` sets the number of timed steps, the line
    carries `ms_per_step`, and the dump holds float64 arrays of the stub's last step (step index W + K - 1 = 4), identical
    in a second run."""
    dumps = []
    for d in ("a", "b"):
        line = _bench({"QRW_BENCH_STUB": "1"}, "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "8",
                      "--dump-outputs", str(tmp_path / d))
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        assert abs(line["value"] - 8 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]
        assert not [k for k in FULL_ONLY if k in line]
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert set(a) == {"mpc_out", "f_cmd", "tau_ff", "f_with_delta"}
    assert all(v.dtype == np.float64 for v in a.values()) and a["mpc_out"].shape == (8, 24, 16)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    expected = np.arange(8)[:, None] * 1e-3 + 4 + np.arange(12)[None, :] * 1e-6   # StubEngine.wbc_compute at s = 4
    np.testing.assert_allclose(a["tau_ff"], expected, rtol=0, atol=1e-12)


def test_dump_sample_of_a_large_output_is_fixed_and_within_the_cap(tmp_path):
    """An array beyond its share of the 64 MB cap is cut to a seeded sample of its instances: the same rows in every call."""
    import importlib.util

    import torch

    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    big = torch.arange(3000, dtype=torch.float64)[:, None].expand(3000, 4096).contiguous()   # 98 MB, row b holds b
    small = torch.ones((3000, 12), dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and a.shape[1] == 4096 and 0 < a.shape[0] < 3000
    assert (np.diff(a[:, 0]) > 0).all() and (a == a[:, :1]).all()               # whole rows of the original, ascending
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and s.shape == (3000, 12)
    assert a.nbytes + s.nbytes <= bench.DUMP_CAP_BYTES


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_what_the_path_computed(tmp_path, synth_mod):
    """The real HIP path, batch 64: the plain line has the headline's keys and none of the `--full` legs; the dumped arrays are
    bit for bit what the same calls on a fresh handle return for the last timed step (the inputs are seeded)."""
    import torch
    import qrw_hip

    B, N, W, K = 64, 16, 2, 3
    line = _bench({}, "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--batch", str(B), "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in line
    assert line["steps"] == K and line["roofline"]["launches"] == K and not [k for k in FULL_ONLY if k in line]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"mpc_out", "f_cmd", "tau_ff", "qdes", "vdes", "f_with_delta", "ddq_res", "feet"}
    sb = synth_mod.SyntheticBatch(B, N, N_gait=20, gaits=("trot",), n_seq=W + K)
    eng = qrw_hip.Batch(B, n_steps=N, N_gait=20, dt_mpc=0.02, T_gait=0.02 * N, dt_wbc=0.002)
    for s in range(W + K):
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in sb.step(s).items()}
        out = eng.mpc_solve(t["xref"], t["fsteps"], s)
        f_cmd = out[:, 12:, 0].contiguous()
        w = eng.wbc_compute(t["q"], t["dq"], f_cmd, t["contacts"], t["pgoals"], t["vgoals"], t["agoals"])
    torch.cuda.synchronize()
    ref = dict({k: v.cpu().numpy() for k, v in w.items()}, mpc_out=out.cpu().numpy(), f_cmd=f_cmd.cpu().numpy())
    for k in ref:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], ref[k]), k


def test_full_is_an_option_that_is_off_by_default(monkeypatch):
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_cli_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse_args()
    assert a.full is False and a.dump_outputs is None and a.steps == 5
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "x"
