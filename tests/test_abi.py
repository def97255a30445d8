"""The C-ABI library loads without a GPU and exports every symbol include/qrw_hip.h declares;
the product path fails loudly (no CPU fallback) when no HIP device is present."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="qrw_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qrw_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    import qrw_hip

    return qrw_hip.load_library()


def test_header_and_binding_agree(lib):
    import qrw_hip

    decl = declared_symbols()
    assert decl, "no symbols parsed from include/qrw_hip.h"
    assert sorted(qrw_hip.SIGNATURES) == decl
    for name in decl:
        assert hasattr(lib, name), name
    # the product header declares nothing that exists for the test suite only; those live in include/qrw_hip_test.h
    assert not [n for n in decl if n.startswith("qrw_test_")]
    tdecl = declared_symbols("qrw_hip_test.h")
    assert tdecl and all(n.startswith("qrw_test_") for n in tdecl) and sorted(qrw_hip.TEST_SIGNATURES) == tdecl
    for name in tdecl:
        assert hasattr(lib, name), name


def test_every_handle_entry_point_refuses_a_null_handle(lib):
    """Every entry point that takes a handle answers a null one (all other arguments zero / NULL) with -1 and an error text that
    begins with its own name, before it touches a device.  qrw_destroy and qrw_state_bytes accept it: 0, error text untouched."""
    import qrw_hip

    no_handle = {"qrw_create", "qrw_last_error", "qrw_selftest_sweeps", "qrw_device_cu_count", "qrw_stream_create",
                 "qrw_stream_destroy", "qrw_test_known_answer", "qrw_test_poison_probe"}
    tolerant = {"qrw_destroy", "qrw_state_bytes"}
    sigs = {**qrw_hip.SIGNATURES, **qrw_hip.TEST_SIGNATURES}
    names = sorted(n for n in sigs if n not in no_handle and n not in tolerant)
    assert len(names) > 30 and all(sigs[n][1][0] is qrw_hip._vp for n in names)
    for name in names:
        rc = getattr(lib, name)(*[t() for t in sigs[name][1]])
        text = lib.qrw_last_error().decode()
        assert rc == -1 and text.startswith(name + ":"), (name, rc, text)
        for t in sorted(tolerant):
            assert getattr(lib, t)(None) == 0 and lib.qrw_last_error().decode() == text, (t, name)


def test_shipped_sources_hold_no_experiment_paths(tmp_path):
    """What lost its A/B is NOT in the translation units of libqrw_hip.so.  The timing experiments that compute wrong results on
    purpose (what a re-arrangement of the sweeps could gain at most) live in scripts/experiments/timing_experiments.patch, applied
    to a copy of the sources by build_timing_experiment.sh, whose output's name the loader refuses; the parity-green forms that
    measured slower (the dissected N = 32 solve with its self-test, the conflict-free LDS layout, plain sweep loads, compiler-
    allocated Delta^-1 rows) live in slower_forms.patch / build_slower_form.sh.  Both patches must still
    apply to today's sources, without fuzz (otherwise the recorded experiments cannot be repeated)."""
    import shutil
    import subprocess

    csrc = os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip")) or f == "Makefile":
            text = open(os.path.join(csrc, f)).read()
            for word in ("EXPERIMENT", "QRW_N32_DISSECT", "BANK_FREE", "CHAIN_READ2", "QRW_NO_ACCD", "dissect_selftest"):
                assert word not in text, (f, word)
    assert not os.path.exists(os.path.join(csrc, "dissect.h"))
    if shutil.which("patch") is None:
        pytest.skip("patch not available")
    for name in ("timing_experiments.patch", "slower_forms.patch"):
        work = tmp_path / name.split(".")[0]
        work.mkdir()
        for f in os.listdir(csrc):
            if f.endswith((".h", ".hip")):
                shutil.copy(os.path.join(csrc, f), work / f)
        r = subprocess.run(["patch", "-p1", "--dry-run", "-F", "0", "-i", os.path.join(ROOT, "scripts", "experiments", name)],
                           cwd=work, capture_output=True, text=True)
        assert r.returncode == 0 and "fuzz" not in r.stdout, (name, r.stdout[-1500:])


def test_loader_refuses_a_wrong_results_build(tmp_path, monkeypatch):
    import shutil

    import qrw_hip

    pkg = os.path.join(ROOT, "quadruped-reactive-walking_amd")
    fake = tmp_path / "WRONG_RESULTS_x.so"
    shutil.copy(os.path.join(pkg, "libqrw_hip.so"), fake)
    monkeypatch.setattr(qrw_hip, "_LIB_PATH", str(fake))
    monkeypatch.setattr(qrw_hip, "_lib", None)
    monkeypatch.delenv("QRW_ALLOW_WRONG_RESULTS", raising=False)
    with pytest.raises(qrw_hip.QrwError):
        qrw_hip.load_library()
    monkeypatch.setenv("QRW_ALLOW_WRONG_RESULTS", "1")
    assert qrw_hip.load_library() is not None


def test_no_cpu_fallback(lib):
    import torch

    import qrw_hip

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(qrw_hip.QrwError):
        qrw_hip.Batch(2)
    import MPC_Wrapper

    with pytest.raises(qrw_hip.QrwError):
        import numpy as np

        q = np.zeros((19, 1))
        q[6, 0] = 1.0
        MPC_Wrapper.MPC_Wrapper(True, 0.02, 16, 10, 0.32, 20, q)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "quadruped-reactive-walking_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "qrw_oracle" not in src and "osqp_restate" not in src, f


def test_shipped_mpc_kernel_spills_nothing_to_scratch(tmp_path):
    """The MPC kernel lives at the edge of the register file (256 VGPRs + ~254 AGPRs).  The one build on record that
    computed wrong results (docs/HISTORY.md 6b) was one in which the allocator ran out of accumulation registers and went to
    scratch while inline-asm-pinned values (AccD) were live; the shipped flags must leave EVERY instantiation with no
    scratch, and the N = 16 one with AGPRs to spare.  On top of the compiler's own resource report, the listing is scanned
    (scripts/isa_accd_scan.py): no scratch instruction, every AGPR the asm blocks read is parked by an asm block, and --
    in a listing with phase markers -- on the hot path of an ADMM iteration no compiler-generated instruction writes an
    AGPR the asm blocks of that path read (the Delta^-1 rows stay put between factorisations) and nothing goes to scratch."""
    import re
    import shutil
    import subprocess
    import sys

    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "quadruped-reactive-walking_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    mpcflags = re.search(r"^MPCFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    base = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-pass-failed"] + mpcflags
    ship = str(tmp_path / "mpc_ship.s")
    r = subprocess.run(base + ["-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "mpc_kernel.hip"), "-o", ship],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blk = r.stderr.split("mpc_solve_kernelILi1ELb1ELb0E")[1]
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
    agprs = int(re.search(r"AGPRs: (\d+)", blk).group(1))
    vspill = int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))
    assert scratch == 0 and vspill == 0 and agprs < 256, (scratch, vspill, agprs)
    # every other instantiation of the kernel (N < 16, N = 32 / 17..31 with two wavefronts, the sequence and the
    # time-sliced forms): no scratch either (round 3: two lambdas around the neighbour exchange were enough to push the
    # N = 32 sequence kernel to 256 AGPRs + 28 B of scratch)
    seen = 0
    for part in r.stderr.split("Function Name: ")[1:]:
        if "mpc_solve_kernelILi" not in part.splitlines()[0]:
            continue
        seen += 1
        name = part.splitlines()[0].split()[0]
        sc = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", part).group(1))
        ag = int(re.search(r"AGPRs: (\d+)", part).group(1))
        vs = int(re.search(r"VGPRs Spill: (\d+)", part).group(1))
        assert sc == 0 and vs == 0 and ag <= 256, (name, sc, vs, ag)
    assert seen == 10, seen  # plain + sequence forms of <1,full>, <1,short>, <2,full>, <2,short>, time-sliced forms of the <2,*>
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_accd_scan

    res = isa_accd_scan.scan_file(ship)
    assert len(res) == 10
    for name, findings, st in res:
        assert not findings, findings[:3]
        assert st["asm_read"] == 120 and st["scratch"] == 0, (name, st)
    # the hot-path check needs the phase markers (asm comments) in the listing: a second build with -DQRW_MARK_PHASES
    mark = str(tmp_path / "mpc_mark.s")
    r = subprocess.run(base + ["-DQRW_MARK_PHASES", os.path.join(csrc, "mpc_kernel.hip"), "-o", mark], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = isa_accd_scan.scan_file(mark)
    assert len(res) == 10
    for name, findings, st in res:
        hot = [f for f in findings if "hot path" in f or "phase markers" in f or "no asm block writes" in f]
        assert not hot, hot[:3]  # (the markers themselves may cost the tightest variant a spill outside the hot path)
        assert st["hot"] and st["hot"]["asm_read"] == 72, (name, st)


def _build_cabi_demo(tmp_path):
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pkg = os.path.join(ROOT, "quadruped-reactive-walking_amd")
    if not os.path.exists(os.path.join(pkg, "libqrw_hip.so")):
        pytest.skip("libqrw_hip.so not built")
    exe = str(tmp_path / "cabi_demo")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "cabi_demo.c"), "-o", exe, "-L" + pkg, "-lqrw_hip", "-lm",
                        "-Wl,-rpath," + pkg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_header_is_plain_c_and_links_without_python(tmp_path):
    """include/qrw_hip.h compiles as C99 with gcc and a plain C program links against libqrw_hip.so (no Python, torch or
    HIP headers on the caller's side): examples/cabi_demo.c.  Without a GPU the library must refuse loudly (no CPU path)."""
    import subprocess

    exe = _build_cabi_demo(tmp_path)
    r = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-500:])
    if r.returncode == 3:
        assert "no HIP device" in r.stderr


@pytest.mark.gpu
def test_plain_c_caller_gets_the_reference_known_answer(tmp_path):
    """The reference's four-stance known answer (scripts/test_mpc.py:54-85) through the C ABI from a plain C program."""
    import subprocess

    exe = _build_cabi_demo(tmp_path)
    r = subprocess.run([exe, "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-500:])
    assert r.stdout.count(" ok") == 5 and "MISMATCH" not in r.stdout
