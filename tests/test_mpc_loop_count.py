"""Regression guard of the MPC kernel's ADMM loop: the instructions ONE plain iteration issues (no factorisation, no check),
counted in a listing compiled with the shipped flags by scripts/loop_count.py.  The kernel is issue-bound with one wavefront
per SIMD: every instruction on this path is a share of the headline.

The reference is the PARENT of the commit that made the loop run in check-free blocks: 910 instructions on the path of the
N = 16 FULL instantiation, 16 of them EXEC-mask bookkeeping (profiles/r8_loop_instructions.txt, counted by the same script in
that commit's listing).  The new build's own figure is deliberately not pinned."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_PLAIN_ITERATION = 910  # <1,true,false,false>, path following, parent commit


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import loop_count

    listing = loop_count.compile_listing(str(tmp_path_factory.mktemp("loop_count") / "mpc_ship.s"))
    return loop_count.report(open(listing).read())


def test_plain_iteration_is_shorter_than_the_parents(counts):
    full = counts["<1,true,false,false>"]
    print("plain iteration: %d instructions (parent %d), %s" % (full["path_total"], PARENT_PLAIN_ITERATION, dict(full["path"])))
    assert full["path_total"] < PARENT_PLAIN_ITERATION
    # the two ways of finding the path agree: the innermost loop holds the plain iteration and nothing else
    assert full["path_total"] == full["loop_total"], (full["path_total"], full["loop_total"])
    # one compare-and-branch for the interval counter, nothing else scalar decides anything
    assert sum(1 for t in full["branches"] if t.startswith("s_cbranch_scc")) == 1, full["branches"]


def test_plain_iteration_has_no_exec_mask_instruction(counts):
    """No s_*saveexec*, no s_cbranch_execz / execnz, no scalar write to EXEC on the path: the loop's decisions are scalars, and the
    one lane-masked store of the iteration (the root store of the forward sweep, csrc/chain_sweep.h) goes through the sweep's
    chain-A pointer, whose other lanes store to the sink."""
    full = counts["<1,true,false,false>"]
    assert not full["exec_mask"], full["exec_mask"]
