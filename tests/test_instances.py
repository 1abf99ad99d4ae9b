"""Which kernel instance a run launches (``csrc/fc_instance.h``), executed on the CPU: the choice
against the launchers' earlier ladders over every combination of its inputs, the refusals, and a
hand-written table of the names the GPU tests assert (``tests/native/instance_check.cpp``); and
the planner's "at most four neighbours" fact on three graphs.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from flipcomplexityempirical_amd import graphs as G

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    out = str(tmp_path_factory.mktemp("instances") / "instance_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", out,
                    os.path.join(HERE, "native", "instance_check.cpp"), os.path.join(CSRC, "fc_plan.cpp"),
                    os.path.join(CSRC, "fc_graph.cpp")], check=True)
    return out


def test_instance_choice(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("checked ") and last.endswith("bad 0"), res.stdout
    assert int(last.split()[1]) > 100000, res.stdout  # every combination was visited


@pytest.mark.parametrize("name, nbr4, ring", [("grid", 1, 8), ("triangular", 0, 8), ("delaunay", 0, 16)])
def test_four_neighbour_fact(exe, tmp_path, name, nbr4, ring):
    """RunShape.nbr4 (KParams.flags kFlagNbr4, the lean k = 2 kernel's neighbour-list body) as the
    planner computes it from the records, against the degrees of the CSR."""
    spec = {"grid": lambda: G.grid_graph(7, 5), "triangular": lambda: G.triangular_graph(6, 9),
            "delaunay": lambda: G.delaunay_graph(400, seed=0)}[name]()
    plan = G.bisection_plan(spec, 2)
    assert (int(spec.degree().max()) <= 4) == bool(nbr4)
    path = str(tmp_path / f"{name}.bin")
    with open(path, "wb") as f:
        np.asarray([spec.n, spec.col_idx.size], dtype=np.int32).tofile(f)
        for a in (spec.row_ptr, spec.col_idx, spec.pop):
            np.asarray(a, dtype=np.int32).tofile(f)
        np.asarray(spec.pos, dtype=np.float64).reshape(-1).tofile(f)
        spec.assignment_array(plan, [0, 1]).tofile(f)
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    words = res.stdout.split()
    assert words[:4] == ["ring", str(ring), "nbr4", str(nbr4)], res.stdout
    assert res.stdout.strip().endswith(f"fc::flip2_kernel<{ring}, 4, false, false, false, false>"), res.stdout
