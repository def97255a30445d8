"""pytest configuration: markers, import paths, shared fixtures."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "quadruped-reactive-walking_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

# The suite's one process creates dozens of streams, and tests of the multi-stream modes assert that work on different streams
# overlaps: that needs the streams on different hardware queues.  qrw_hip.load_library() only raises HIP's default of four where
# the caller's environment does not say anything (a deployment's own setting wins); the suite must not depend on what its
# caller happened to export, so it sets the eight queues the library asks for itself -- before anything touches the GPU.
os.environ["GPU_MAX_HW_QUEUES"] = "8"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle_mod():
    import oracle  # oracle/oracle.py (test infrastructure)

    oracle.build()
    return oracle


@pytest.fixture(scope="session")
def synth_mod():
    import synth

    return synth
