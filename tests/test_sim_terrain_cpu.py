"""What a machine without a GPU can check of the simulator's heightfield terrain: the numpy checker's own properties
(tests/sim_terrain_numpy.py against tests/sim_numpy.py), the states of the GPU tests (clear of every switch of the contact law,
spreads as recorded), Simulator.reference_rough_ground(), csrc/sim_terrain.h as a stand-alone program under the address and
undefined-behaviour sanitizers, and the compiler's resource report of both instantiations of sim_kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc")
# scripts/sim_tolerance.py / tests/test_gpu_sim.py: one tick of the flat checker with its state moved by one ulp, x 100
FLAT_TICK_BOUND = 3.53e-9


@pytest.fixture(scope="module")
def stn(oracle_mod):
    import sim_terrain_numpy

    return sim_terrain_numpy


@pytest.fixture(scope="module")
def gpu_cases(stn):
    import test_gpu_sim_terrain

    return test_gpu_sim_terrain


def _command(k, rng_phase):
    return (3.0, 0.2, np.asarray([0.0, 0.7, -1.4, 0.0, 0.7, -1.4, 0.0, -0.7, 1.4, 0.0, -0.7, 1.4]) + 0.15 * np.sin(0.2 * k + rng_phase),
            0.03 * np.cos(0.2 * k + rng_phase), 0.2 * np.sin(0.13 * k + 2.0 * rng_phase))


def _start(stn, seed, z):
    rng = np.random.default_rng(seed)
    quat = np.array([0.02, -0.015, 0.1, 1.0])
    q = np.concatenate([[0.013, -0.021, z], quat / np.linalg.norm(quat), stn.Q_STANCE + 0.05 * rng.normal(size=12)])
    return q, rng.uniform(0, 2 * np.pi, 12)


# ------------------------------------------------------------------------------------------------ the checker's own properties
def test_zero_field_is_sim_numpy_exactly(stn):
    """H = 0: 60 ticks of the terrain checker equal tests/sim_numpy.py bit for bit, state and every output, in and out of contact."""
    sn = stn.sn
    T = stn.Terrain(np.zeros((5, 7)), 0.3, 0.25, -0.8, -0.6)
    for seed, z in ((1, 0.24), (2, 0.28)):
        q, phase = _start(stn, seed, z)
        a, b = sn.SimNumpy(q), stn.SimTerrainNumpy(q, T)
        touched = 0.0
        for k in range(60):
            fe = None if k % 3 else np.array([1.0, -2.0, 0.5, 0.1, 0.05, -0.1])
            a.step(*_command(k, phase), f_ext=fe)
            b.step(*_command(k, phase), f_ext=fe)
            assert np.array_equal(a.q, b.q) and np.array_equal(a.v, b.v) and np.array_equal(a.prev, b.prev) and a.tick == b.tick == k + 1
            assert all(np.array_equal(a.out[n], b.out[n]) for n in a.out), k
            touched = max(touched, a.out["contact_forces"][:, 2].max())
        assert touched > 1.0 and a.min_abs_d == b.min_abs_d
    assert sn.contact_forces.__module__ == "sim_numpy"  # (the checker put sim_numpy's own law back after every step)


def test_constant_field_is_the_plane_with_the_base_lowered(stn):
    """H = c: the run from a base c higher equals the flat run within the flat tick bound (heights after taking c out)."""
    sn = stn.sn
    c = 0.0371
    T = stn.Terrain(np.full((4, 3), c), 0.6, 0.5, -0.6, -0.75)
    q, phase = _start(stn, 3, 0.245)
    up = q.copy()
    up[2] += c
    a, b = sn.SimNumpy(q), stn.SimTerrainNumpy(up, T)
    worst = 0.0
    for k in range(60):  # (teacher-forced: every tick starts from the flat run's state, c higher)
        b.set_state(np.concatenate([a.q[:2], [a.q[2] + c], a.q[3:]]), a.v, a.prev, a.tick)
        a.step(*_command(k, phase))
        b.step(*_command(k, phase))
        qb = b.q.copy()
        qb[2] -= c
        pairs = [(a.q, qb), (a.v, b.v), (a.prev, b.prev)] + [(a.out[n], b.out[n] - ([0, 0, c] if n == "true_pos" else 0)) for n in a.out]
        worst = max(worst, max(np.abs(x - y).max() / max(1.0, np.abs(x).max()) for x, y in pairs))
    print("H = c against the lowered base: worst relative difference %.3g (bound %.3g)" % (worst, FLAT_TICK_BOUND))
    assert worst <= FLAT_TICK_BOUND and a.out["contact_forces"][:, 2].max() > 1.0


def test_shifting_the_field_and_the_origin_together_changes_nothing(stn, gpu_cases):
    """x0, y0 and the origin moved by the same (exactly representable) amount: the same cells, fractions, forces and ticks."""
    T = gpu_cases.rough_field(stn)
    moved = stn.Terrain(T.H, T.dx, T.dy, T.x0 + 8.0, T.y0 - 4.0)
    _, states = gpu_cases._fd_states(stn, "rough")
    for q, v, tau, fe, origin, _, _ in states[:10]:  # (the in-field states: 8 and -4 are absorbed without rounding there)
        ca, cb = [], []
        a = stn.forward_dynamics(q, v, tau, T, origin, f_ext=fe, cells=ca)
        b = stn.forward_dynamics(q, v, tau, moved, origin + [8.0, -4.0], f_ext=fe, cells=cb)
        assert [c[:2] for c in ca] == [c[:2] for c in cb]
        assert np.allclose([c[2:] for c in ca], [c[2:] for c in cb], rtol=0, atol=1e-13)
        assert all(np.allclose(x, y, rtol=1e-9, atol=1e-9) for x, y in zip(a, b))
    # ... and a free run of 10 ticks on the moved field stays with the run on the field where it was
    P = stn.Terrain(T.H, 0.0625, 0.0625, -0.25, -0.25)
    Pm = stn.Terrain(T.H, 0.0625, 0.0625, -0.25 + 8.0, -0.25 - 4.0)
    q, phase = _start(stn, 5, 0.27)
    q[:2] = [0.015625, -0.0078125]
    a, b = stn.SimTerrainNumpy(q, P, (0.0, 0.0)), stn.SimTerrainNumpy(q, Pm, (8.0, -4.0))
    for k in range(10):
        a.step(*_command(k, phase))
        b.step(*_command(k, phase))
    assert np.abs(a.q - b.q).max() < 1e-12 and np.abs(a.out["contact_forces"] - b.out["contact_forces"]).max() < 1e-9
    assert np.abs(a.out["contact_forces"]).sum() > 0


def test_static_force_on_an_inclined_plane(stn):
    """h = s x: a foot at rest whose centre is foot_radius - delta from the plane feels exactly kn delta n; nothing once delta < 0;
    the same on either triangle of a cell."""
    prm = stn.DEFAULTS
    for s in (0.5, -0.2, 2.0):
        x = -0.3 + 0.1 * np.arange(7)
        T = stn.Terrain(np.tile(s * x, (5, 1)), 0.1, 0.2, -0.3, -0.4)
        n = np.array([-s, 0.0, 1.0]) / np.sqrt(s * s + 1.0)
        for (X, Y), kind in (((0.0712, 0.013), "lower"), ((0.0212, 0.093), "upper")):
            h, gx, gy, (_, _, fu, fv) = T.surface(X, Y)
            assert (fu >= fv) == (kind == "lower") and abs(h - s * X) < 1e-15 and abs(gx - s) < 1e-14 and abs(gy) < 1e-14
            for delta in (0.003, 0.0155, 0.04, -0.001):
                centre = np.array([X, Y, s * X]) + (prm["foot_radius"] - delta) * n
                hh, gx, gy, _ = T.surface(centre[0], centre[1])
                f, d = stn.foot_force(hh, gx, gy, centre[2], np.zeros(3), prm)
                assert abs(d - delta) < 1e-15
                want = prm["kn"] * max(delta, 0.0) * n
                assert np.abs(f - want).max() <= 1e-12 * prm["kn"] * abs(delta), (s, kind, delta, f, want)


def test_lookup_clamps_outside_the_field_and_survives_any_coordinate(stn):
    T = stn.Terrain(np.arange(12.0).reshape(3, 4), 0.5, 0.25, 1.0, -1.0)  # x in [1, 2.5], y in [-1, -0.5]
    assert T.cell(1.6, -0.8) == (0, 1, pytest.approx(0.2), pytest.approx(0.8))
    assert T.cell(0.0, -0.8)[1:3] == (0, 0.0) and T.cell(9.0, -0.8)[1:3] == (2, 1.0)
    assert T.cell(1.6, -5.0)[0::3] == (0, 0.0) and T.cell(1.6, 5.0)[0::3] == (1, 1.0)
    assert T.surface(0.0, -0.8)[0] == T.surface(1.0, -0.8)[0]  # the clamped point of the edge cell
    for big in (1e300, -1e300, np.inf, -np.inf):
        r, c, fu, fv = T.cell(big, -big)
        assert (c, fu) == ((2, 1.0) if big > 0 else (0, 0.0)) and (r, fv) == ((0, 0.0) if big > 0 else (1, 1.0))
    r, c, fu, fv = T.cell(np.nan, np.nan)
    assert (r, c) == (0, 0) and np.isnan(fu) and np.isnan(fv) and np.isnan(T.surface(np.nan, 0.0)[0])


# ------------------------------------------------------------------------------------------------ the GPU tests' states
def test_gpu_states_are_clear_of_the_switches_and_the_spreads_are_as_recorded(stn, gpu_cases):
    """The states tests/test_gpu_sim_terrain.py compares on: no foot nearer than 1e-9 to d = 0, to the diagonal or (the
    deliberately out-of-field states apart) to a cell edge; the wanted numbers of contacts; the checker's free run of the
    teacher-forced case sees 0 .. 4 feet in contact and both triangle kinds; the spreads are the literals of that file."""
    g = gpu_cases
    for which in g.FIELDS:
        T, states = g._fd_states(stn, which)
        contacts, kinds = [], set()
        for i, (q, v, tau, fe, origin, want, outside) in enumerate(states):
            cells = []
            _, _, d = stn.forward_dynamics(q, v, tau, T, origin, cells=cells)
            kinds |= g.check_switches(d, cells, outside)
            clamped = any(f in (0.0, 1.0) for c in cells for f in c[2:])
            assert clamped == outside, (which, i, cells)
            contacts.append(int((d > 0).sum()))
            assert want is None or contacts[-1] == want, (which, i, d)
        assert {0, 1, 4} <= set(contacts) and (kinds == {"lower", "upper"} or which == "ramp"), (contacts, kinds)
        g.check_identical_robots(stn, T, states)
    solve, ulp = g.fd_spread(stn)
    spread, d_min, diag_min, edge_min, seen, kinds = g.tick_spread(stn)
    print("fd spread %.3g (solve %.3g), tick spread %.3g; smallest |d| %.3g, |fu - fv| %.3g, edge %.3g" % (ulp, solve, spread, d_min, diag_min, edge_min))
    assert min(d_min, diag_min, edge_min) > g.MIN_SWITCH and seen == {0, 1, 2, 3, 4} and kinds == {"lower", "upper"}
    # the recorded literals are these measurements (to their three digits; libm differences between machines stay far below 2x)
    assert 0.5 * g.FD_SPREAD <= ulp <= 2.0 * g.FD_SPREAD and solve < ulp, (solve, ulp)
    assert 0.5 * g.TICK_SPREAD <= spread <= 2.0 * g.TICK_SPREAD, spread
    assert g.FD_BOUND == pytest.approx(100 * g.FD_SPREAD) and g.TICK_BOUND == pytest.approx(100 * g.TICK_SPREAD)


# ------------------------------------------------------------------------------------------------ the reference's rough ground
def test_reference_rough_ground():
    """Simulator.reference_rough_ground(): 512 x 512 samples at 0.05 m centred on the origin, raw values within [0, 0.05], the
    row-pair and interleave structure of scripts/PyBulletSimulator.py:57-60, sample values pinned from a run of this code, the
    centring switch, and the caller's global random state left alone."""
    import random

    import Simulator

    random.seed(7)
    before = random.random()
    random.seed(7)
    raw = Simulator.reference_rough_ground(center=False)
    assert random.random() == before
    H = raw["heights"]
    assert H.shape == (512, 512) and H.dtype == np.float64
    assert (raw["dx"], raw["dy"]) == (0.05, 0.05) and raw["x0"] == raw["y0"] == -0.05 * 511 / 2
    assert 0.0 <= H.min() < 1e-5 and 0.05 - 1e-5 < H.max() <= 0.05
    assert np.array_equal(H[0::2], H[1::2])                                   # (:57/:59 and :58/:60: rows come in equal pairs
    draws = H[0::2, 1::2]                                                      # (:58) the odd columns hold the draws themselves
    prev = np.concatenate([[0.0], draws.ravel()[:-1]]).reshape(draws.shape)    # (:51, :61) the draw before, across the row ends too
    assert np.array_equal(H[0::2, 0::2], (draws + prev) * 0.5)                 # (:57) the even columns the mean with the draw before
    assert len(np.unique(draws)) == draws.size
    pinned = {(0, 0): 0.009525517249894287, (0, 1): 0.019051034499788573, (2, 1): 0.020732362419352453, (511, 511): 0.04572880939958991,
              (300, 201): 0.00012789002421859097, (137, 400): 0.03200550731169257}
    for (r, c), want in pinned.items():
        assert H[r, c] == want, (r, c, repr(H[r, c]))
    rng = random.Random(41)
    assert H[0, 1] == rng.uniform(0, 0.05) and H[0, 3] == rng.uniform(0, 0.05)  # (:44, :52-55: the order of the draws)
    centred = Simulator.reference_rough_ground()
    mid = 0.5 * (H.min() + H.max())
    assert np.array_equal(centred["heights"], H - mid) and centred["heights"].max() == pytest.approx(-centred["heights"].min(), abs=1e-17)
    assert {k: v for k, v in centred.items() if k != "heights"} == {k: v for k, v in raw.items() if k != "heights"}
    with pytest.raises(ValueError, match="terrain=: unknown keys"):
        Simulator.check_terrain(dict(centred, nx=3), None)
    assert Simulator.check_terrain(None, None) is None and set(Simulator.check_terrain(centred, None)) == set(centred)


# ------------------------------------------------------------------------------------------------ sim_terrain.h under sanitizers
HOST_PROGRAM = r"""
// csrc/sim_terrain.h alone, queried at every coordinate a foot could come with.  The field's heights sit in a heap block of
// exactly rows * cols doubles, so that AddressSanitizer sees any index outside it; prints one line per query.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "sim_terrain.h"
using namespace qrw::terrain;
static int run(int rows, int cols, double x0, double y0, double dx, double dy) {
  double* H = (double*)malloc(sizeof(double) * rows * cols);
  for (int i = 0; i < rows * cols; i++) H[i] = 0.01 * ((i * 37) % 11) - 0.02;
  const Field T{H, rows, cols, x0, y0, dx, dy};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double x1 = x0 + dx * (cols - 1), y1 = y0 + dy * (rows - 1);
  const double xs[] = {x0 + 0.3 * dx, 0.5 * (x0 + x1), x1 - 0.2 * dx, x0, x1, x0 + dx, x0 - 1e-12, x1 + 1e-12, x0 - 50.0, x1 + 50.0,
                       1e300, -1e300, inf, -inf, nan};
  const double ys[] = {y0 + 0.6 * dy, 0.5 * (y0 + y1), y1 - 0.7 * dy, y0, y1, y0 + dy, y0 - 1e-12, y1 + 1e-12, y0 - 50.0, y1 + 50.0,
                       1e300, -1e300, inf, -inf, nan};
  int bad = 0;
  for (double X : xs)
    for (double Y : ys) {
      const Axis u = axis_cell(X, T.x0, T.dx, T.cols), v = axis_cell(Y, T.y0, T.dy, T.rows);
      const bool in_range = u.i >= 0 && u.i <= cols - 2 && v.i >= 0 && v.i <= rows - 2;
      const bool fractions = (std::isnan(X) ? std::isnan(u.f) : (u.f >= 0.0 && u.f <= 1.0)) &&
                             (std::isnan(Y) ? std::isnan(v.f) : (v.f >= 0.0 && v.f <= 1.0));
      const Plane s = surface(T, X, Y);  // (reads the four corners)
      const bool finite = (std::isnan(X) || std::isnan(Y)) ? !std::isfinite(s.h) : std::isfinite(s.h);
      if (!in_range || !fractions || !finite) bad++;
      printf("%d %d %.17g %.17g %d %d %.17g %.17g %.17g %.17g %.17g\n", rows, cols, X, Y, v.i, u.i, u.f, v.f, s.h, s.gx, s.gy);
    }
  free(H);
  return bad;
}
int main() {
  int bad = run(6, 9, -0.225, 0.1, 0.05, 0.075);
  bad += run(2, 2, 1.0, -2.0, 0.5, 0.25);
  bad += run(2, 5, -1e3, 1e3, 1e-3, 10.0);
  fprintf(stderr, "bad queries: %d\n", bad);
  return bad ? 1 : 0;
}
"""


def test_terrain_lookup_under_the_sanitizers(tmp_path, stn):
    """csrc/sim_terrain.h -- the text the kernel compiles -- as a stand-alone g++ program under -fsanitize=address,undefined,float-cast-overflow:
    in-field
    points, points on every edge, far outside on all four sides, +-1e300, +-inf and NaN, on a 6 x 9, a 2 x 2 and a 2 x 5 field.
    Every query leaves the indices in range and the run is clean; every line agrees with the numpy checker's lookup."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "terrain_host.cpp", tmp_path / "terrain_host"
    src.write_text(HOST_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined,float-cast-overflow",
                        "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr.strip() == "bad queries: 0", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * 15 * 15
    fields = {}
    for rows, cols, x0, y0, dx, dy in ((6, 9, -0.225, 0.1, 0.05, 0.075), (2, 2, 1.0, -2.0, 0.5, 0.25), (2, 5, -1e3, 1e3, 1e-3, 10.0)):
        H = np.array([0.01 * ((i * 37) % 11) - 0.02 for i in range(rows * cols)]).reshape(rows, cols)
        fields[(rows, cols)] = stn.Terrain(H, dx, dy, x0, y0)
    for line in lines:
        w = line.split()
        T = fields[(int(w[0]), int(w[1]))]
        X, Y = float(w[2]), float(w[3])
        h, gx, gy, (rr, cc, fu, fv) = T.surface(X, Y)
        assert (rr, cc) == (int(w[4]), int(w[5])), line
        assert np.array_equal([fu, fv, h, gx, gy], [float(x) for x in w[6:]], equal_nan=True), (line, fu, fv, h, gx, gy)


# ------------------------------------------------------------------------------------------------ resource report
def test_both_sim_kernel_instantiations_use_no_scratch(tmp_path):
    """The compiler's own resource report (-Rpass-analysis=kernel-resource-usage) of sim_kernel.hip for gfx950.  The flat
    instantiation is what DESIGN.md 4.7 records for the kernel before it had a terrain: 256 VGPRs + 130 AGPRs, no LDS, no
    scratch, nothing spilled.  The terrain instantiation's figures are printed; it reached 0 bytes of scratch too, and keeps it."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "sim_kernel.hip"), "-o", str(tmp_path / "sim.s")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for part in r.stderr.split("Function Name: ")[1:]:
        m = re.search(r"sim_kernelILb([01])E", part.splitlines()[0])
        if not m:
            continue
        seen[m.group(1)] = {key: int(re.search(pat + r": (\d+)", part).group(1))
                            for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]"), ("spill", r"VGPRs Spill"), ("vgprs", r"VGPRs"),
                                             ("agprs", r"AGPRs"), ("lds", r"LDS Size \[bytes/block\]"))}
    assert sorted(seen) == ["0", "1"], seen
    for which, s in sorted(seen.items()):
        print("sim_kernel<%s>: %d VGPRs, %d AGPRs, scratch %d, spilled %d, LDS %d"
              % ("terrain" if which == "1" else "flat", s["vgprs"], s["agprs"], s["scratch"], s["spill"], s["lds"]))
    assert seen["0"] == dict(scratch=0, spill=0, vgprs=256, agprs=130, lds=0), seen["0"]
    assert seen["1"]["scratch"] == 0 and seen["1"]["lds"] == 0, seen["1"]
