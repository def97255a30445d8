"""What a machine without a GPU can check of the joystick stage: the numpy checker's own properties (tests/joystick_numpy.py),
csrc/joystick_profile.h -- the text the kernel compiles -- as a stand-alone program under the address and undefined-behaviour
sanitizers, bit for bit against the checker, and the compiler's resource report of the three instantiations of joystick_kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import joystick_cases as jc
import joystick_numpy as jn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the checker's own properties
def test_a_segment_starts_at_v0_and_ends_at_v1():
    """ev = 0 gives v0 exactly; the polynomial at ev = t1 equals v1 to rounding; the first difference vanishes to first order at
    both ends (the blend has zero slope there: a difference of order 1/t1^2 of the step, not 1/t1)."""
    rng = np.random.default_rng(0)
    for t1 in (7, 500, 4096, 1 << 17):
        v = rng.normal(size=(6, 2))
        r = jn.JoystickNumpy(k_switch=[0, t1, t1 + 5], v_switch=np.concatenate([v, v[:, 1:]], axis=1))
        r.handle_v_switch(0)
        assert np.array_equal(r.v_ref, v[:, 0])
        r.apply_velocity_change(t1, 1)  # (the scan never evaluates a segment at its end: the polynomial itself, at ev = t1)
        step = np.abs(v[:, 1] - v[:, 0])
        # (six rounded operations on intermediates no larger than |v0| + 3 step + 2 step: 3 eps of that; 16 is margin)
        assert np.all(np.abs(r.v_ref - v[:, 1]) <= 16 * np.finfo(float).eps * (np.abs(v).max() + 5 * step.max()))
        r.handle_v_switch(1)
        first = np.abs(r.v_ref - v[:, 0])
        r.handle_v_switch(t1 - 1)
        last = np.abs(r.v_ref - v[:, 1])
        # |v(1) - v(0)| = step (3 / t1^2 - 2 / t1^3) and the same at the far end
        bound = step * 3.0 / t1**2 + 8 * np.finfo(float).eps * np.abs(v).max()
        assert np.all(first <= bound) and np.all(last <= bound), (t1, first, last, bound)


def test_the_hold_after_the_last_switch_is_the_tick_before_it():
    ks, vs = [0, 10, 30], np.arange(18.0).reshape(6, 3)
    r = jn.JoystickNumpy(k_switch=ks, v_switch=vs)
    for k in range(30):
        r.update_v_ref(k)
    held = r.v_ref.copy()
    for k in range(30, 50):
        r.update_v_ref(k)
        assert np.array_equal(r.v_ref, held)
    one = jn.JoystickNumpy(k_switch=[0], v_switch=np.ones((6, 1)))  # n_switch = 1: never evaluated
    one.update_v_ref(0)
    one.update_v_ref(99)
    assert np.array_equal(one.v_ref, np.zeros(6))


def test_the_bell_is_zero_at_both_ends_and_one_in_the_middle():
    for t1 in (1, 2, 7, 500, 1 << 13):
        assert jn.bell(0, t1) == 0.0
        assert abs(jn.bell(t1, t1)) <= 128 * np.finfo(float).eps  # (16 - 32 + 16, each term within 1.5 eps of itself: < 100 eps)
        if t1 % 2 == 0:
            assert jn.bell(t1 // 2, t1) == 1.0
    r = jn.JoystickNumpy(gamepad=True, pushes=[(5, 10, np.ones(3), np.ones(3))])
    assert np.array_equal(r.apply_external_forces(4), np.zeros(6)) and np.array_equal(r.apply_external_forces(16), np.zeros(6))
    assert np.array_equal(r.apply_external_forces(10), np.ones(6))


def test_the_ramp_reaches_exactly_one_and_stays():
    V = jc.ramp_speeds(6, 1)
    for b in range(6):
        r = jn.JoystickNumpy(ramp=V[b], k_start=480)
        r.update_v_ref(479)
        assert np.array_equal(r.v_ref, np.zeros(6) * np.concatenate([V[b, :2], [0, 0, 0], V[b, 2:]]))
        for k in (480 + 12000, 480 + 12001, 10**6):
            r.update_v_ref(k)
            assert np.array_equal(r.v_ref, [V[b, 0], V[b, 1], 0.0, 0.0, 0.0, V[b, 2]])


def test_the_dead_band_is_strict():
    r = jn.JoystickNumpy(gamepad=True)
    for target in jc.DEADBAND_NEIGHBOURS:
        r.v_ref = np.zeros(6)
        r.update_v_ref_gamepad([jc.command_for(target, r.alpha), 0, 0, 0, 0, 0])
        assert r.v_ref[0] == (target if abs(target) == 0.005 else 0.0), (target, r.v_ref[0])


def test_codes_are_one_shot_and_the_later_pair_wins():
    r = jn.JoystickNumpy(gamepad=True, codes=[(20, 2), (7, 5), (20, 4)])
    got = [r.update_v_ref(k, np.zeros(6))[1] for k in range(30)]
    assert got == [4 if k == 20 else 5 if k == 7 else 0 for k in range(30)]


# ------------------------------------------------------------------------------------------------ joystick_profile.h on the host
HOST_PROGRAM = r"""
// csrc/joystick_profile.h alone.  Reads one fleet from the file named on the command line (robot-major tables, doubles as hex),
// asks the header's own checks, lays the tables out item-major in heap blocks of EXACTLY their size -- so that AddressSanitizer
// sees any index outside them --, evaluates every tick for every robot and prints v_ref, code and f_ext as hex doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "joystick_profile.h"
using namespace qrw::joy;
static double rd(FILE* f) { char w[64]; if (fscanf(f, "%63s", w) != 1) exit(3); return strtod(w, nullptr); }
static long ri(FILE* f) { long v; if (fscanf(f, "%ld", &v) != 1) exit(3); return v; }
template <class T> static T* block(size_t n) { return (T*)malloc(sizeof(T) * (n ? n : 1)); }
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  const int mode = (int)ri(f), B = (int)ri(f), ns = (int)ri(f), nc = (int)ri(f), np = (int)ri(f), nt = (int)ri(f);
  Tables T{};
  T.B = B; T.n_switch = ns; T.n_codes = nc; T.n_pushes = np;
  T.k_start = (int32_t)ri(f); T.gp_alpha = rd(f); T.gp_deadband = rd(f);
  const size_t Bz = (size_t)B;
  int32_t *ksw = block<int32_t>(ns * Bz), *ck = block<int32_t>(nc * Bz), *cv = block<int32_t>(nc * Bz), *ps = block<int32_t>(np * Bz),
          *pd = block<int32_t>(np * Bz);
  double *vsw = block<double>(ns * 6 * Bz), *rv = block<double>(3 * Bz), *pw = block<double>(np * 6 * Bz);
  std::vector<int32_t> row(64);
  for (int b = 0; b < B; b++) {
    int entry = 0;
    for (int i = 0; i < ns; i++) ksw[i * Bz + b] = row[i] = (int32_t)ri(f);
    if (ns && check_profile(row.data(), ns, &entry)) { fprintf(stderr, "robot %d k_switch entry %d\n", b, entry); return 4; }
    for (int c = 0; c < 6; c++) for (int i = 0; i < ns; i++) vsw[((size_t)i * 6 + c) * Bz + b] = rd(f);
    double V[3];
    for (int c = 0; c < 3; c++) rv[c * Bz + b] = V[c] = rd(f);
    if (check_ramp(V, &entry)) { fprintf(stderr, "robot %d ramp entry %d\n", b, entry); return 4; }
    for (int e = 0; e < nc; e++) { ck[e * Bz + b] = (int32_t)ri(f); cv[e * Bz + b] = (int32_t)ri(f); }
    for (int e = 0; e < np; e++) {
      ps[e * Bz + b] = (int32_t)ri(f); pd[e * Bz + b] = row[e] = (int32_t)ri(f);
      for (int c = 0; c < 6; c++) pw[((size_t)e * 6 + c) * Bz + b] = rd(f);
    }
    if (check_push(row.data(), np, &entry)) { fprintf(stderr, "robot %d push entry %d\n", b, entry); return 4; }
  }
  T.k_switch = ksw; T.v_switch = vsw; T.ramp_v = rv; T.code_k = ck; T.code_v = cv; T.push_start = ps; T.push_dur = pd; T.push_w = pw;
  std::vector<double> state(6 * Bz, 0.0);
  for (int t = 0; t < nt; t++) {
    const int32_t k = (int32_t)ri(f);
    for (int b = 0; b < B; b++) {
      double v[6], w[6];
      if (mode == kProfile) profile_eval(T, b, k, v);
      else if (mode == kRamp) ramp_eval(T, b, k, v);
      else for (int c = 0; c < 6; c++) v[c] = state[6 * b + c] = gamepad_filter(T.gp_alpha, T.gp_deadband, rd(f), state[6 * b + c]);
      push_sum(T, b, k, w);
      for (int c = 0; c < 6; c++) printf("%a ", v[c]);
      printf("%d", (int)code_at(T, b, k));
      for (int c = 0; c < 6; c++) printf(" %a", w[c]);
      printf("\n");
    }
  }
  free(ksw); free(ck); free(cv); free(ps); free(pd); free(vsw); free(rv); free(pw);
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("joystick_host")
    src, exe = d / "joystick_host.cpp", d / "joystick_host"
    src.write_text(HOST_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def run_host(exe, path, mode, B, ticks, profiles=None, ramp=None, k_start=0, alpha=0.1, deadband=0.005, codes=None, pushes=None,
             v_gp=None):
    """The fleet through the host program (padded exactly as Joystick.Joystick_batch pads it); v_ref, code, f_ext (T,B,..)."""
    import Joystick

    ns = 0
    if profiles is not None:
        K, V = Joystick.pad_profiles(profiles, B)
        ns = K.shape[1]
    CK, CV = Joystick.pad_codes(codes if codes is not None else [[]] * B, B)
    PK, PW = Joystick.pad_pushes(pushes if pushes is not None else [[]] * B, B)
    hx = lambda a: " ".join(float(x).hex() for x in np.asarray(a).reshape(-1))
    lines = ["%d %d %d %d %d %d %d %s %s" % (mode, B, ns, CK.shape[1], PK.shape[1], len(ticks), k_start, float(alpha).hex(),
                                               float(deadband).hex())]
    for b in range(B):
        if ns:
            lines.append(" ".join(str(int(x)) for x in K[b]))
            lines.append(hx(V[b]))
        lines.append(hx(ramp[b] if ramp is not None else np.zeros(3)))
        lines.append(" ".join("%d %d" % (CK[b, e], CV[b, e]) for e in range(CK.shape[1])))
        for e in range(PK.shape[1]):
            lines.append("%d %d %s" % (PK[b, e, 0], PK[b, e, 1], hx(PW[b, e])))
    for i, k in enumerate(ticks):
        lines.append(str(int(k)) + ("" if v_gp is None else " " + hx(v_gp[i])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])  # (a sanitizer report goes to stderr)
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(ticks) * B
    v = np.array([[float.fromhex(x) for x in w[:6]] for w in rows]).reshape(len(ticks), B, 6)
    c = np.array([int(w[6]) for w in rows]).reshape(len(ticks), B)
    fe = np.array([[float.fromhex(x) for x in w[7:]] for w in rows]).reshape(len(ticks), B, 6)
    return v, c, fe


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n_cols", [2, 5, 32])
def test_host_profiles_equal_the_checker_bit_for_bit(host_exe, tmp_path, n_cols):
    """Tables of 2, 5 and 32 columns (padded ones among them), codes and pushes at their maximum lengths beside them, at every
    switch +- 1, every middle, 0 and 1000 ticks past the end; the checker is stepped through every tick."""
    B = 5
    prof, codes, pushes = jc.profile_tables(B, n_cols, 10 + n_cols), jc.code_tables(B, 16, 3), jc.push_tables(B, 8, 4)
    ticks = sorted(set(jc.profile_ticks(prof)) | set(jc.code_ticks(codes)) | set(jc.push_ticks(pushes)))
    want = jc.expected(jc.robots(B, profiles=prof, codes=codes, pushes=pushes), ticks)
    got = run_host(host_exe, tmp_path / "case.txt", 0, B, ticks, profiles=prof, codes=codes, pushes=pushes)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    assert (np.abs(want[0]).max(axis=(0, 1)) > 0).all()  # all six components move
    assert np.abs(want[2]).max() > 0 and want[1].max() > 0


def test_host_limits_equal_the_checker_bit_for_bit(host_exe, tmp_path):
    """n_switch = 1 (zeros), ticks far past the last switch (2^31 - 1 among them), the largest legal segment (2^17 ticks) and the
    largest legal push (2^13 ticks).  The long tables are stepped through the listed ticks only: they hold k_switch[-1] - 1, the
    one tick the hold after the end takes its value from."""
    rng = np.random.default_rng(5)
    big, bigp = 1 << 17, 1 << 13
    prof = [([0], rng.normal(size=(6, 1))), ([0, big], rng.normal(size=(6, 2))), ([0, 3, 3 + big, 3 + big + 1], rng.normal(size=(6, 4)))]
    pushes = [[(7, bigp, rng.normal(size=3), rng.normal(size=3))], [(0, 1, np.ones(3), -np.ones(3))], []]
    ticks = sorted({0, 1, 2, 3, 4, 7, 8, 7 + bigp // 2, 7 + bigp - 1, 7 + bigp, 7 + bigp + 1, big // 2, big // 2 + 1, big - 2, big - 1, big,
                    big + 1, big + 2, big + 3, big + 4, big + 1000, (1 << 31) - 1})
    want = jc.expected(jc.robots(3, profiles=prof, pushes=pushes), ticks, every_tick=False)
    got = run_host(host_exe, tmp_path / "case.txt", 0, 3, ticks, profiles=prof, pushes=pushes)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    assert np.array_equal(want[0][:, 0], np.zeros((len(ticks), 6)))


def test_host_ramp_and_gamepad_equal_the_checker_bit_for_bit(host_exe, tmp_path):
    B, k_start = 6, 480
    V = jc.ramp_speeds(B, 2)
    ticks = jc.ramp_ticks(V, k_start)
    want = jc.expected(jc.robots(B, ramp=V, k_start=k_start), ticks, every_tick=False)  # (the ramp overwrites v_ref from k alone)
    got = run_host(host_exe, tmp_path / "ramp.txt", 1, B, ticks, ramp=V, k_start=k_start)
    assert same_bits(got[0], want[0]) and (want[0][-1][:, [0, 1, 5]] == V).all()
    T = 120
    g = jc.gamepad_commands(B, T, 6)
    fleet = jc.robots(B, gamepad={})
    want_v = jn.run(fleet, range(T), g)[0]
    got = run_host(host_exe, tmp_path / "gp.txt", 2, B, list(range(T)), alpha=fleet[0].alpha, v_gp=g)
    assert same_bits(got[0], want_v)
    assert [want_v[0, b, 0] for b in range(4)] == [0.005, -0.005, 0.0, 0.0]


def test_host_checks_refuse_what_the_limits_exclude(host_exe, tmp_path):
    """check_profile / check_push as the init entry point asks them: decreasing k_switch, a segment of 2^17 + 1 ticks, a table
    that starts after tick 0, push durations 0 and 2^13 + 1."""
    import Joystick

    v2 = np.zeros((6, 2))
    for prof, pushes, text in (([([0, 5, 4], np.zeros((6, 3)))], None, "robot 0 k_switch entry 2"),
                               ([([0, (1 << 17) + 1], v2)], None, "robot 0 k_switch entry 1"),
                               ([([1, 5], v2)], None, "robot 0 k_switch entry 0"),
                               ([([0, 5], v2)], [[(0, 3, np.zeros(3), np.zeros(3)), (0, 0, np.zeros(3), np.zeros(3))]], "robot 0 push entry 1"),
                               ([([0, 5], v2)], [[(0, (1 << 13) + 1, np.zeros(3), np.zeros(3))]], "robot 0 push entry 0")):
        with pytest.raises(AssertionError, match=text):
            run_host(host_exe, tmp_path / "bad.txt", 0, 1, [0], profiles=prof, pushes=pushes)
    assert Joystick.PUSH_PAD[0] + Joystick.PUSH_PAD[1] < 0


# ------------------------------------------------------------------------------------------------ Python helpers
def test_for_analysis_tables_and_the_stick_mapping():
    """for_analysis's tables are those of main_solo12_control.py:113-119 + update_for_analysis; gamepad_command is :94-103."""
    import Joystick

    built = {}

    class Capture(Joystick.Joystick_batch):
        def __init__(self, controller, profiles=None, **kw):
            built["profiles"] = profiles

    des = np.zeros((3, 6))
    des[0, 0], des[1, 5], des[2, 1] = 0.8, -1.2, 0.05
    _, n_sim = Capture.for_analysis(None, des, 0.002)
    for b, n_analysis in enumerate((int(0.8 / 0.1 / 0.002) + 1, int(1.2 / 0.1 / 0.002) + 1, int(0.05 / 0.1 / 0.002) + 1)):
        ks, vs = built["profiles"][b]
        assert list(ks) == [0, 500, max(n_analysis, 500), n_analysis + 1500]
        assert np.array_equal(vs, np.stack([np.zeros(6), np.zeros(6), des[b], des[b]], axis=1))
    assert n_sim == int(1.2 / 0.1 / 0.002) + 1 + 1500
    # the slow target: the reference's out-of-order table [0, 500, ~251, ~1751] and the ordered one give the same values on every tick
    n_slow = int(0.05 / 0.1 / 0.002) + 1
    assert n_slow < 500
    ref = jn.JoystickNumpy(k_switch=[0, 500, n_slow, n_slow + 1500], v_switch=built["profiles"][2][1])
    mine = jn.JoystickNumpy(k_switch=built["profiles"][2][0], v_switch=built["profiles"][2][1])
    for k in range(1800):
        assert same_bits(ref.update_v_ref(k)[0], mine.update_v_ref(k)[0]), k
    assert np.allclose(Joystick.gamepad_command(0.5, -1.0, 0.25), [1.2, -0.3, 0.0, 0.0, 0.0, -0.4], rtol=1e-15, atol=0)
    assert np.allclose(Joystick.gamepad_command(0.5, -1.0, 0.25, l1=True), [0.0, 0.0, -0.1, -1.5, 2.4, 0.0], rtol=1e-15, atol=0)
    assert Joystick.gamepad_command(np.zeros(4), np.ones(4), np.zeros(4)).shape == (4, 6)


# ------------------------------------------------------------------------------------------------ resource report
def test_the_three_joystick_kernel_instantiations_use_no_scratch_and_no_lds(tmp_path):
    """The compiler's own resource report (-Rpass-analysis=kernel-resource-usage) of joystick_kernel.hip for gfx950: 0 bytes of
    scratch, nothing spilled, no LDS, in every mode (DESIGN.md 4.8 records the figures)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "joystick_kernel.hip"), "-o", str(tmp_path / "joy.s")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for part in r.stderr.split("Function Name: ")[1:]:
        m = re.search(r"joystick_kernelILi([012])E", part.splitlines()[0])
        if not m:
            continue
        seen[m.group(1)] = {key: int(re.search(pat + r": (\d+)", part).group(1))
                            for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]"), ("spill", r"VGPRs Spill"), ("sspill", r"SGPRs Spill"),
                                             ("vgprs", r"VGPRs"), ("lds", r"LDS Size \[bytes/block\]"))}
    assert sorted(seen) == ["0", "1", "2"], seen
    for which, s in sorted(seen.items()):
        print("joystick_kernel<%s>: %d VGPRs, scratch %d, spilled %d + %d, LDS %d"
              % (("profile", "ramp", "gamepad")[int(which)], s["vgprs"], s["scratch"], s["spill"], s["sspill"], s["lds"]))
        assert s["scratch"] == 0 and s["spill"] == 0 and s["sspill"] == 0 and s["lds"] == 0, (which, s)
