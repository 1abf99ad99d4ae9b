"""The k = 2 ring-verdict table (``csrc/fc_ring_table.h``) on the host: every entry of every class
against the slot evaluation stated the long way, the class ids, the cap and the planner's use of
the table (``tests/native/ring_table_check.cpp``), on a 3 x 3 grid (corner rings of 3 cells, side
rings of 5, the centre's 8), a 9 x 7 grid, sec11, and a 12 x 12 grid with seeded edge deletions
that keep the graph connected.  The program is also built with the address and undefined-behaviour
sanitizers and run stand-alone.  Each graph's class count is printed (``-s`` shows it).  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from flipcomplexityempirical_amd import graphs as G

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


def thinned_grid(nx=12, ny=12, seed=11, tries=60):
    """A 12 x 12 grid without some of its edges: seeded deletions, each kept only if both halves of
    the column plan (and with them the graph) stay connected.  Deleting edges only lowers degrees,
    so every node keeps at most four neighbours; the rings fall into many more classes than a
    lattice's."""
    import networkx as nx_
    spec = G.grid_graph(nx, ny)
    plan = G.threshold_plan(spec.nodes, 0, nx / 2 - 0.5)
    g = nx_.Graph()
    g.add_nodes_from(spec.nodes)
    e = spec.edges()
    g.add_edges_from((spec.nodes[u], spec.nodes[v]) for u, v in e)
    rng = np.random.default_rng(seed)
    halves = [[u for u in spec.nodes if plan[u] == d] for d in sorted(set(plan.values()))]
    removed = 0
    for i in rng.permutation(len(e))[:tries]:
        u, v = spec.nodes[e[i, 0]], spec.nodes[e[i, 1]]
        g.remove_edge(u, v)
        if all(nx_.is_connected(g.subgraph(h)) for h in halves) and nx_.is_connected(g):
            removed += 1
        else:
            g.add_edge(u, v)
    assert removed >= 20
    for u in g.nodes:
        g.nodes[u]["population"] = 1
    out = G.from_networkx(g, pos={u: (float(u[0]), float(u[1])) for u in g.nodes})
    assert int(out.degree().max()) <= 4 and int(out.degree().min()) >= 1
    return out, {u: plan[u] for u in out.nodes}


def graphs():
    g33, g97, sec = G.grid_graph(3, 3), G.grid_graph(9, 7), G.sec11_graph()
    thin, thin_plan = thinned_grid()
    return {
        "grid3x3": (g33, G.threshold_plan(g33.nodes, 0, 0.5)),
        "grid9x7": (g97, G.threshold_plan(g97.nodes, 0, 3.5)),
        "sec11": (sec, G.sec11_plan(0, sec.nodes)),
        "grid12x12_thinned": (thin, thin_plan),
    }


def write_graph(path, spec, plan):
    labels = sorted(set(plan.values()))
    with open(path, "wb") as f:
        np.asarray([spec.n, spec.col_idx.size], dtype=np.int32).tofile(f)
        for a in (spec.row_ptr, spec.col_idx, spec.pop):
            np.asarray(a, dtype=np.int32).tofile(f)
        np.asarray(spec.pos, dtype=np.float64).reshape(-1).tofile(f)
        spec.assignment_array(plan, labels).astype(np.int8).tofile(f)


def _build(out, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *extra, "-I", CSRC, "-o", out,
                    os.path.join(HERE, "native", "ring_table_check.cpp"), os.path.join(CSRC, "fc_plan.cpp"),
                    os.path.join(CSRC, "fc_graph.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ring_table_graphs")
    out = {}
    for name, (spec, plan) in graphs().items():
        out[name] = (str(d / f"{name}.bin"), spec)
        write_graph(out[name][0], spec, plan)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    return _build(str(tmp_path_factory.mktemp("ring_table") / "ring_table_check"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    return _build(str(tmp_path_factory.mktemp("ring_table_san") / "ring_table_check_san"),
                  ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))


NAMES = ("grid3x3", "grid9x7", "sec11", "grid12x12_thinned")


def _run(exe, path, spec):
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    head, last = lines[0].split(), lines[-1].split()
    assert head[:2] == ["graph", "n"] and int(head[2]) == spec.n and head[3:5] == ["ring", "8"] and head[5:7] == ["nbr4", "1"], res.stdout
    classes = int(head[8])
    assert last[0] == "checked" and last[2:] == ["bad", "0"], res.stdout
    assert int(last[1]) >= classes * 256  # every class x every ring byte was compared
    print(f"ring table: {os.path.basename(path)} n {spec.n} classes {classes} checks {last[1]}")
    return classes


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_matches_the_long_way(exe, files, name):
    path, spec = files[name]
    classes = _run(exe, path, spec)
    assert 1 <= classes <= spec.n
    if name == "grid3x3":  # corners, sides and the centre differ in ring length alone
        assert classes >= 3
    if name in ("grid9x7", "sec11"):  # a lattice: "a handful", well under the default cap
        assert classes <= 64


@pytest.mark.parametrize("name", NAMES)
def test_sanitized_stand_alone_program(exe_san, files, name):
    path, spec = files[name]
    _run(exe_san, path, spec)
