"""The k = 2 tally case table on the CPU (``tally_cases.CASES`` drives the device parity test,
test_tally_edges_gpu.py): the pass plan of ``csrc/fc_tally_plan.h`` against the launcher's earlier
loop and the hand-written table (``tests/native/tally_plan_check.cpp``, also built with the host
sanitizers), the plan each pass-plan case is for, and each case's coverage condition taken from
the oracle.  A failure of a coverage condition means the case is wrong, not the kernel."""
import fcntl
import os
import shutil
import subprocess

import numpy as np
import pytest

import tally_cases as TC
from flipcomplexityempirical_amd.engine import FlipGraph

SAN = os.path.join(TC.HERE, "sanitize")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = TC.build_plan_check(tmp_path_factory.mktemp("tally_plan"))
    if out is None:
        pytest.skip("no host C++ toolchain")
    return out


def _checked(exe_path):
    res = subprocess.run([exe_path], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, \
        res.stdout[-2000:] + res.stderr[-4000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith("bad 0"), res.stdout
    return int(last.split()[1])


def test_plan_against_the_earlier_loop_and_the_table(exe):
    # 16 subsets x 2 limits x every (n, n_edges) pair of the sweep, two checks each, and the table
    assert _checked(exe) > 1000000


def test_plan_check_under_host_sanitizers():
    """The same stand-alone program from tests/sanitize/Makefile (address + undefined)."""
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host C++ toolchain")
    os.makedirs(os.path.join(SAN, "build"), exist_ok=True)
    with open(os.path.join(SAN, "build", ".lock"), "w") as lk:  # (test_sanitize.py builds there too)
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            subprocess.run(["make", "-s", "-C", SAN, "build/tally_plan_check"], check=True)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    assert _checked(os.path.join(SAN, "build", "tally_plan_check")) > 1000000


@pytest.mark.parametrize("name", list(TC.HAND_PLANS))
def test_plan_of_the_case(exe, name):
    """The plan a pass-plan case is for: the native program's at limit 163,840 is the hand table's."""
    case = TC.BY_NAME[name]
    spec = case.spec
    got = TC.native_plan(exe, TC.ALL, spec.n, spec.n_edges, TC.LIMIT)
    passes, gmask = TC.HAND_PLANS[name]
    assert got == {"limit": TC.LIMIT, "passes": passes, "global_mask": gmask}


def test_table_covers_the_plan_branches(exe):
    """More than one pass; arrays 6-8 without 0-5; EDGE in a pass other than the first; global
    atomics with and without LDS passes; a pass of exactly the limit."""
    plans = {n: TC.HAND_PLANS[n] for n in TC.HAND_PLANS}
    assert len(plans["sec11"][0]) == 1 and plans["sec11"][1] == 0
    assert plans["grid48x48"][0][1][0] == TC.FCN | TC.OCC | TC.LA
    assert not plans["grid70x70"][0][0][0] & TC.EDGE and plans["grid70x70"][0][1][0] & TC.EDGE
    assert plans["grid104x104"][1] == TC.CUT | TC.EDGE and len(plans["grid104x104"][0]) == 7
    assert all(b == TC.LIMIT for _, b in plans["grid160x128"][0])
    assert plans["grid144x144"] == ([(0, 0)], 511)
    # the subsets of the 48 x 48 grid: one pass each, the two pairs with a hole in the array order
    spec = TC.BY_NAME["grid48x48"].spec
    masks = {v[0]: TC.native_plan(exe, v[1], spec.n, spec.n_edges, TC.LIMIT)["passes"] for v in TC.SUBSETS}
    assert [m[0][0] for m in masks.values()] == [3, 4, 56, 448, 3 | 448, 4 | 448] and all(len(m) == 1 for m in masks.values())


def test_ring16_graph():
    """Rings of 16 cells, every node decided by the run rule, and the per-edge arrays above the limit;
    its plan is the native program's (asserted on the device)."""
    spec = TC.delaunay7000()
    fg = FlipGraph(spec)
    assert fg.info["ring_max"] == 16 and fg.info["n_exact"] == spec.n
    fg.close()
    assert 8 * (spec.n_edges + 1) > TC.LIMIT and 8 * spec.n_edges > TC.LIMIT and 8 * (spec.n + 1) <= TC.LIMIT
    wide = FlipGraph(TC.delaunay_wide())
    assert wide.info["ring_max"] == 16
    wide.close()


@pytest.mark.parametrize("name", list(TC.BY_NAME))
def test_case_reaches_what_it_is_for(name):
    case = TC.BY_NAME[name]
    assert sum(case.launch_steps()) == case.steps and min(case.launch_steps()) > 0
    assert {"plan": [700, 1, 799], "ring16": [700, 1, 799], "overflow": [7, 300, 1693]}.get(
        case.group, [case.steps]) == case.launch_steps()
    for c in range(case.n_chains):
        ref = case.oracle(c)
        assert case.chain_ok(case, c, ref), (name, c, ref["stats"])
        assert int(ref["cut_hist"].sum()) == int(ref["nb_hist"].sum()) == case.steps + 1
        assert int(ref["flip_count"].sum()) == ref["stats"]["accepted"]
    if case.group == "overflow":
        # more entries than a 64-entry log holds in the launches of 300 and 1,693 steps
        assert min(case.oracle(c)["stats"]["accepted"] for c in range(case.n_chains)) > 3 * 64


def test_long_runs_measured():
    """The numbers DESIGN.md records for the long case (seed 77, chains 0-3)."""
    case = TC.BY_NAME["long grid6x6"]
    runs = [TC.run_lengths(case, case.oracle(c)) for c in range(case.n_chains)]
    assert [case.oracle(c)["stats"]["accepted"] for c in range(4)] == [416, 480, 200, 626]
    assert [int(r.max()) for r in runs] == [226739, 276084, 417515, 246815]
    assert all(int(r.sum()) == case.steps + 1 for r in runs)
    assert all(r.max() < 1 << 24 for r in runs)  # the run field's 24 bits
