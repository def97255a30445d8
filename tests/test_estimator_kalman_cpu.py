"""What a machine without a GPU can check of the Kalman variant of the state estimator: the dense numpy checker's own properties
(tests/estimator_kalman_numpy.py), csrc/kalman_filter.h built for the host and run against that checker, the compiler's resource
report of both instantiations of the estimator kernel, and the surface (header, binding, Controller_batch's option)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc")
DT = 0.002
H_INIT = 0.22294615
Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])
IDENT = np.array([0.0, 0.0, 0.0, 1.0])
# scripts/kalman_tolerance.py: (a) 4.2e-15, (b) 2.1e-13, (c) 4.3e-13 on the GPU tests' sequences -> 100 x 4.3e-13
# (tests/test_gpu_estimator_kalman.py holds the same literal)
KALMAN_BOUND = 4.3e-11


@pytest.fixture(scope="module")
def ekn(oracle_mod):
    import estimator_kalman_numpy

    return estimator_kalman_numpy


def _err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


# ------------------------------------------------------------------------------------------------ the checker's own properties
def test_checker_structure_over_a_trot(oracle_mod, synth_mod, ekn):
    """400 ticks of a trot table at dt = 0.002 with noisy sensors: the cross-axis entries of the dense P are exactly 0.0 (the
    filter is three 6-state filters), its diagonal is > 0, and it is symmetric to 1e-12 of its largest entry although the
    reference never symmetrises it."""
    sen = synth_mod.SyntheticSensors(1, 3)
    est = ekn.Estimator(DT, H_INIT)
    goals = np.zeros((3, 4))
    axis = np.arange(18) % 3
    cross = axis[:, None] != axis[None, :]
    period = synth_mod.gait_pattern("trot", 16)
    seen = set()
    for k in range(400):
        gait = np.zeros((20, 4))
        gait[:16] = np.roll(period, -(k // 10), axis=0)
        seen.add(tuple(gait[0]))
        d = sen.step(k)
        est.run_filter(gait, goals, d["lin_acc"][0], d["ang_vel"][0], d["quat"][0], d["q_mes"][0], d["v_mes"][0])
        P = est.P
        assert P.shape == (18, 18) and est.X.shape == (18,) and est.Z.shape == (16,)
        assert not P[cross].any(), k
        assert (np.diag(P) > 0).all(), k
        assert np.abs(P - P.T).max() <= 1e-12 * np.abs(P).max(), k
        assert not est.Z[12:].any()
    assert seen == {(1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0)}
    # the complementary filters are not stepped in this mode; the shared part is
    assert not est.filter_xyz_vel.HP_x.any() and not est.filter_xyz_pos.LP_x.any() and est.k_log == 400 and est.FK_xyz[2] != H_INIT


def test_checker_converges_in_four_foot_stance(oracle_mod, ekn):
    """All four feet in stance, zero acceleration, constant joint angles: base minus foot converges to the measured offset,
    X[0:3] - X[6+3i:9+3i] -> Z[3i:3i+3], and the foot heights X[6+3i+2] -> 0.  A constant measurement of a static state is
    averaged, so the residual falls like 1 / ticks: after 400 ticks it is below a hundredth of the first tick's, and it never
    rises between checkpoints."""
    est = ekn.Estimator(DT, H_INIT)
    gait = np.zeros((20, 4))
    gait[:16] = 1
    res, height = [], []
    for k in range(400):
        est.run_filter(gait, np.zeros((3, 4)), np.zeros(3), np.zeros(3), IDENT, Q_INIT, np.zeros(12))
        if k % 50 == 0 or k == 399:
            X, Z = est.X, est.Z
            res.append(max(np.abs(X[0:3] - X[6 + 3 * i:9 + 3 * i] - Z[3 * i:3 * i + 3]).max() for i in range(4)))
            height.append(max(abs(X[6 + 3 * i + 2]) for i in range(4)))
    assert all(b < a for a, b in zip(res, res[1:])) and all(b < a for a, b in zip(height, height[1:]))
    assert res[-1] < res[0] / 100 and height[-1] < height[0] / 100, (res, height)
    assert res[-1] < 1e-5 and height[-1] < 1e-4


@pytest.mark.parametrize("status", [[1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 1, 0]])
def test_update_coeffs_closed_forms(ekn, status):
    """R = sigma_kin^2 / trust and sigma_h^2 / trust, Q = sigma_dp^2 (1 + exp(gamma (0.5 - trust))) dt^2 on a foot's states and
    sigma_a^2 dt^2 on the velocity states, 0 on the position states; trust 1 in stance, 0.01 in swing; nothing off the diagonal."""
    tune = dict(sigma_kin=0.1, sigma_h=1.0, sigma_a=0.1, sigma_dp=0.1, gamma=30.0)
    for tuning in (tune, dict(sigma_kin=0.07, sigma_h=0.6, sigma_a=0.25, sigma_dp=0.04, gamma=12.0)):
        kf = ekn.KFilterBis(DT, **tuning)
        kf.update_coeffs([1, 1, 1, 1] if status != [1, 1, 1, 1] else [0, 0, 0, 0])  # (overwritten by the next call: not state)
        kf.update_coeffs(status)
        r, q = np.zeros(16), np.zeros(18)
        for i, s in enumerate(status):
            trust = 1.0 if s else 0.01
            r[3 * i:3 * i + 3] = tuning["sigma_kin"]**2 / trust
            r[12 + i] = tuning["sigma_h"]**2 / trust
            q[6 + 3 * i:9 + 3 * i] = tuning["sigma_dp"]**2 * (1 + np.exp(tuning["gamma"] * (0.5 - trust))) * DT**2
        q[3:6] = tuning["sigma_a"]**2 * DT**2
        assert np.allclose(np.diag(kf.R), r, rtol=1e-15, atol=0) and np.allclose(np.diag(kf.Q), q, rtol=1e-15, atol=0)
        assert not (kf.R - np.diag(np.diag(kf.R))).any() and not (kf.Q - np.diag(np.diag(kf.Q))).any()
    swing, stance = 0.1**2 * (1 + np.exp(30 * 0.49)) * DT**2, 0.1**2 * (1 + np.exp(-15.0)) * DT**2
    assert swing / stance > 1e6  # a swinging foot is free to move, a standing one is not


# ------------------------------------------------------------------------------------------------ kalman_filter.h on the host
HOST_PROGRAM = r"""
// reads: dt h_init sigma_kin sigma_h sigma_a sigma_dp gamma ticks, then per tick U (3), Z (16), feet status (4);
// prints per tick X (18) and the dense P (324)
#include <cstdio>
#include "kalman_filter.h"
int main(int argc, char** argv) {
  using namespace qrw::kf;
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  double dt, h_init;
  Tuning t;
  int ticks;
  if (fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %d", &dt, &h_init, &t.sigma_kin, &t.sigma_h, &t.sigma_a, &t.sigma_dp, &t.gamma, &ticks) != 8)
    return 3;
  Filter kf;
  filter_init(kf, h_init);
  for (int k = 0; k < ticks; k++) {
    double u[3], z[kMeas], status[4], X[kStates], P[kStates * kStates];
    for (double& v : u) if (fscanf(f, "%lf", &v) != 1) return 4;
    for (double& v : z) if (fscanf(f, "%lf", &v) != 1) return 4;
    for (double& v : status) if (fscanf(f, "%lf", &v) != 1) return 4;
    filter_step(kf, t, dt, u, z, status);
    filter_state(kf, X);
    filter_covariance(kf, P);
    for (double v : X) printf("%.17g ", v);
    for (double v : P) printf("%.17g ", v);
    printf("\n");
  }
  return 0;
}
"""


def _host_inputs(ticks=300):
    """U, Z and the feet status per tick: a trot that switches every 20 ticks, with the all-swing row (ticks 100..119) and the
    all-stance row (ticks 200..239) in it; Z around a standing robot's foot offsets, moving, with noise."""
    rng = np.random.default_rng(17)
    feet = np.array([[-0.08, -0.15, 0.26], [-0.08, 0.15, 0.26], [0.31, -0.15, 0.26], [0.31, 0.15, 0.26]])
    U, Z, S = rng.uniform(-0.5, 0.5, (ticks, 3)), np.zeros((ticks, 16)), np.zeros((ticks, 4))
    for k in range(ticks):
        S[k] = [1, 0, 0, 1] if (k // 20) % 2 == 0 else [0, 1, 1, 0]
        if 100 <= k < 120:
            S[k] = 0
        if 200 <= k < 240:
            S[k] = 1
        Z[k, :12] = (feet + 0.02 * np.sin(0.05 * k + np.arange(12).reshape(4, 3)) + rng.normal(0, 0.003, (4, 3))).ravel()
    return U, Z, S


@pytest.mark.parametrize("tuning", [dict(sigma_kin=0.1, sigma_h=1.0, sigma_a=0.1, sigma_dp=0.1, gamma=30.0),
                                    dict(sigma_kin=0.07, sigma_h=0.6, sigma_a=0.25, sigma_dp=0.04, gamma=12.0)])
def test_host_build_of_the_filter_matches_the_dense_checker(tmp_path, ekn, tuning):
    """csrc/kalman_filter.h -- the text the kernel compiles -- as a stand-alone g++ program: 300 ticks with stance switches, the
    all-swing and the all-stance row, X and P on every tick against the dense checker (18 x 18 P, inv) within the measured
    bound; exact zeros between the axes."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src, exe, data = tmp_path / "kalman_host.cpp", tmp_path / "kalman_host", tmp_path / "inputs.txt"
    src.write_text(HOST_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    U, Z, S = _host_inputs()
    names = ("sigma_kin", "sigma_h", "sigma_a", "sigma_dp", "gamma")
    with open(data, "w") as f:
        f.write(" ".join(repr(float(v)) for v in [DT, H_INIT] + [tuning[n] for n in names]) + " %d\n" % len(U))
        for k in range(len(U)):
            f.write(" ".join(repr(float(v)) for v in np.concatenate([U[k], Z[k], S[k]])) + "\n")
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    got = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines()])
    assert got.shape == (len(U), 18 + 324)
    kf = ekn.KFilterBis(DT, **tuning)
    kf.X[2] = H_INIT
    axis = np.arange(18) % 3
    cross = axis[:, None] != axis[None, :]
    worst = 0.0
    for k in range(len(U)):
        kf.update_coeffs(S[k])
        kf.predict(U[k])
        kf.correct(Z[k])
        X, P = got[k, :18], got[k, 18:].reshape(18, 18)
        assert not P[cross].any(), k
        e = max(_err(X, kf.X), float(np.abs(P - kf.P).max() / np.abs(kf.P).max()))
        worst = max(worst, e)
        assert e <= KALMAN_BOUND, (k, e)
    print("host build against the dense checker: worst %.3g (bound %.3g)" % (worst, KALMAN_BOUND))


def test_host_header_index_maps(ekn):
    """The per-axis index maps kalman_filter.h documents are H's structure: axis j touches the states {j, 3+j, 6+3i+j} and the
    measurement rows {3i+j} (and 12+i for j = 2)."""
    H = ekn.KFilterBis(DT).H
    for j in range(3):
        states = [j, 3 + j] + [6 + 3 * i + j for i in range(4)]
        rows = [3 * i + j for i in range(4)] + ([12 + i for i in range(4)] if j == 2 else [])
        others = [s for s in range(18) if s not in states]
        assert not H[np.ix_(rows, others)].any()
        assert all(H[3 * i + j, j] == 1.0 and H[3 * i + j, 6 + 3 * i + j] == -1.0 for i in range(4))
    text = open(os.path.join(CSRC, "kalman_filter.h")).read()
    assert "k < 2 ? 3 * k + axis : 6 + 3 * (k - 2) + axis" in text and "return 3 * foot + axis" in text and "return 12 + foot" in text


# ------------------------------------------------------------------------------------------------ resource report
def test_both_estimator_instantiations_use_no_scratch(tmp_path):
    """The compiler's own resource report (-Rpass-analysis=kernel-resource-usage) of estimator_kernel.hip for gfx950: the
    complementary and the Kalman instantiation both with ScratchSize 0 and no spilled VGPR (the Kalman one keeps a 6 x 6 block of
    P per lane in registers: an index the compiler cannot resolve would send the block to scratch)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "estimator_kernel.hip"), "-o",
                        str(tmp_path / "estimator.s")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for part in r.stderr.split("Function Name: ")[1:]:
        name = part.splitlines()[0].split()[0]
        m = re.search(r"estimator_kernelILb([01])E", name)
        if not m:
            continue
        seen[m.group(1)] = tuple(int(re.search(pat + r": (\d+)", part).group(1))
                                 for pat in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"VGPRs", r"AGPRs", r"Occupancy \[waves/SIMD\]"))
    assert sorted(seen) == ["0", "1"], seen
    for which, (scratch, spill, vgprs, agprs, occupancy) in seen.items():
        print("estimator_kernel<%s>: %d VGPRs, %d AGPRs, scratch %d, spilled %d, occupancy %d"
              % ("true" if which == "1" else "false", vgprs, agprs, scratch, spill, occupancy))
        assert scratch == 0 and spill == 0, (which, scratch, spill)


# ------------------------------------------------------------------------------------------------ surface
def test_header_and_binding_have_the_two_entry_points():
    import __graft_entry__ as g

    g.build()
    import qrw_hip

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrw_hip.h")).read(), flags=re.S)
    lib = qrw_hip.load_library()
    for name in ("qrw_estimator_init_kalman", "qrw_estimator_kalman_get_host"):
        assert re.search(r"\bint\s+%s\s*\(\s*qrw_handle\s+h\b" % name, text), name
        assert name in qrw_hip.SIGNATURES and hasattr(lib, name)
    assert re.search(r"double\s+sigma_kin;.*double\s+sigma_h;.*double\s+sigma_a;.*double\s+sigma_dp;.*double\s+gamma;.*\}\s*qrw_kalman_config",
                     text, flags=re.S)
    assert [n for n, _ in qrw_hip._KalmanConfig._fields_] == ["sigma_kin", "sigma_h", "sigma_a", "sigma_dp", "gamma"]
    kc = qrw_hip.kalman_config(True)
    assert [getattr(kc, n) for n in qrw_hip.KALMAN_DEFAULTS] == [0.1, 1.0, 0.1, 0.1, 30.0]
    assert qrw_hip.kalman_config(dict(gamma=5)).gamma == 5.0 and qrw_hip.kalman_config(dict(gamma=5)).sigma_h == 1.0
    with pytest.raises(qrw_hip.QrwError, match=r"kalman=: unknown keys \['sigma'\] \(sigma_kin, sigma_h, sigma_a, sigma_dp, gamma\)"):
        qrw_hip.kalman_config(dict(sigma=1.0))
    assert qrw_hip.KALMAN_ITEMS == {"X": (0, (18,)), "P": (1, (18, 18)), "Z": (2, (16,))}


@pytest.mark.parametrize("groups", [None, 2])
def test_controller_rejects_unknown_estimator_options_before_it_makes_a_handle(monkeypatch, groups):
    import qrw_hip
    from Controller import Controller_batch

    made = []
    monkeypatch.setattr(qrw_hip, "Batch", lambda *a, **k: made.append(a) or (_ for _ in ()).throw(AssertionError("a handle was made")))
    with pytest.raises(qrw_hip.QrwError, match=r"kalman=: unknown keys \['sigma_x'\]"):
        Controller_batch(4, Q_INIT, groups=groups, estimator=dict(h_init=H_INIT, kalman=dict(sigma_x=1.0)))
    with pytest.raises(qrw_hip.QrwError, match=r"estimator=: unknown keys \['kalmann'\] \(h_init, perfect, kalman\)"):
        Controller_batch(4, Q_INIT, groups=groups, estimator=dict(h_init=H_INIT, kalmann=True))
    assert not made
